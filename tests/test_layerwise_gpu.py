"""LAMB and LARS: per-variable trust ratios formed on the device (csrc/layerwise.h,
csrc/kernels/optim_layerwise.hip, MnistEngine.set_lamb / set_lars): the segmented norms exactly, the
exact cases of both updates through the flat ops, the guards and flags, both ops against the fp64
definitions within the bounds derived in layerwise.h, and the engine's step -- against the fp64 applier,
captured graphs, EMA, clipping, forced data-parallel schedules at world 1, two ranks over IPC, the
sharded schedules' refusal and the untouched default step.

Engines run at batch 5 on a synthetic 64-row dataset, on a side stream.
"""
import math

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import LW_ADAPT, LW_DECAY, schedule_args

from dist_util import run_ranks

pytestmark = pytest.mark.gpu

B, ROWS = 5, 64
U = 2.0 ** -24  # fp32 unit roundoff
BOTH = LW_DECAY | LW_ADAPT
# hyper-parameters that fp32 holds exactly, so the fp64 definition and the device read the same numbers
B1, B2, EPS, WD, LR = 0.875, 1.0 - 2.0 ** -8, 2.0 ** -20, 2.0 ** -6, 2.0 ** -7
MU, EETA = 0.875, 2.0 ** -3
SCHED = O.PiecewiseConstant([2, 5], [2.0 ** -7, 2.0 ** -9, 2.0 ** -11])  # both boundaries inside a 4-step graph
NAMES = ["wc1", "bc1", "wc2", "bc2", "wd1", "bd1", "out", "out_b"]


def _chunk():
    return int(torch.ops.tfd.layerwise_chunk())


def _segs(rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def _table(lengths, flags=None, gaps=(0, 4, 8, 0, 12)):
    """Segments of the given lengths, each begin a multiple of 4, gaps[i % len] spare elements between."""
    rows, pos = [], 0
    for i, n in enumerate(lengths):
        rows.append((pos, n, BOTH if flags is None else flags[i % len(flags)]))
        pos = (pos + n + 3) // 4 * 4 + gaps[i % len(gaps)]
    return rows, pos + 8  # a tail that belongs to no variable


def _tables():
    c = _chunk()
    mixed = [BOTH, BOTH, 0, LW_DECAY, LW_ADAPT]
    return {
        "ragged": _table([1, 3, 4, 5, 255, c - 1, c, c + 1, 3 * c + 2], mixed),
        "ones": _table([1] * 16, gaps=(0,)),  # length-1 segments at stride 4
        "s300": _table([(37 * i) % 301 + 1 for i in range(300)], mixed),
        "mnist": (M.segments(True), M.TOTAL),
    }


# ---------------------------------------------------------------- 1. norms, exact
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["ragged", "ones", "s300", "mnist"])
def test_layer_norms_of_powers_of_two_are_exact(cuda, name, dt):
    """Every element of variable i is 2^-(i % 5): every fp32 sum is exact in any order, so the norm is
    sqrt(count) * value bit for bit. The gaps hold 2^10, which no norm may see."""
    rows, numel = _tables()[name]
    x = torch.full((numel,), 1024.0, device=cuda)
    want = []
    for i, (b, n, _) in enumerate(rows):
        v = 2.0 ** -(i % 5)
        x[b:b + n] = v
        want.append(np.float32(math.sqrt(n * v * v)))
    got = torch.ops.tfd.layer_norms(x.to(dt), _segs(rows))
    assert got.dtype == torch.float32 and got.shape == (len(rows),)
    assert got.cpu().numpy().tobytes() == np.array(want, dtype=np.float32).tobytes(), (name, got[:10], want[:10])


@pytest.mark.parametrize("name", ["ragged", "mnist"])
def test_one_element_moves_its_own_norm_only(cuda, name):
    rows, numel = _tables()[name]
    segs = _segs(rows)
    mid = len(rows) // 2
    spots = [(k, e) for k in (0, mid, len(rows) - 1) for e in (rows[k][0], rows[k][0] + rows[k][1] - 1)]
    tail = rows[-1][0] + rows[-1][1]  # the tail belongs to no variable
    assert tail < numel
    # ... and neither does a gap between two variables (the MNIST table has none: its variables abut)
    inner = [b + n for (b, n, _), (b2, _, _) in zip(rows, rows[1:]) if b + n < b2]
    assert bool(inner) == (name == "ragged")
    for k, e in spots + [(None, tail)] + [(None, g) for g in inner[:1] + inner[-1:]]:
        x = torch.zeros(numel, device=cuda)
        x[e] = 2.0
        want = [2.0 if i == k else 0.0 for i in range(len(rows))]
        assert torch.ops.tfd.layer_norms(x, segs).tolist() == want, (name, k, e)


def test_layer_norms_are_bit_identical_run_to_run(cuda):
    for name, (rows, numel) in _tables().items():
        x = torch.randn(numel, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
        a = torch.ops.tfd.layer_norms(x, _segs(rows))
        b = torch.ops.tfd.layer_norms(x, _segs(rows))
        assert torch.equal(a, b), name
        ref = torch.stack([x[s:s + n].double().norm() for s, n, _ in rows])
        assert ((a.double() - ref).abs() <= 9 * U * ref).all(), name  # kLwNormUlps


def test_bad_tables_raise(cuda):
    x = torch.zeros(64, device=cuda)
    for rows, what in (([(8, 4, 3), (0, 4, 3)], "sorted"), ([(0, 8, 3), (4, 4, 3)], "overlaps"), ([(2, 4, 3)], "multiple of 4"),
                       ([(0, 0, 3)], "empty"), ([(60, 8, 3)], "outside"), ([(0, 4, 7)], "flags")):
        with pytest.raises(RuntimeError, match=what):
            torch.ops.tfd.layer_norms(x, _segs(rows))


# ---------------------------------------------------------------- 2. LARS and LAMB, exact
N1 = 4096
ONE = [(0, N1, BOTH)]


def _lars(p, acc, g, pbf, rows, lr, mu, wd, eeta, eps, **kw):
    return torch.ops.tfd.lars_flat(p, acc, g, pbf, _segs(rows), lr, mu, wd, eeta, eps, **kw)


def _lamb(p, m, v, g, pbf, rows, lr, b1, b2, eps, wd, **kw):
    return torch.ops.tfd.lamb_flat(p, m, v, g, pbf, _segs(rows), lr, b1, b2, eps, wd, **kw)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_lars_exact_case(cuda, gdt):
    """p = 0.5, g = 0.25, eeta = 2^-3, eps = 0, lr = 0.5, mu = 0: |p| = 32, |g| = 16; lambda = 0 gives
    r = 0.25, lambda = 0.5 gives r = 0.125; accum' = 2^-5 and p' = 0.46875 either way."""
    for wd, r in ((0.0, 0.25), (0.5, 0.125)):
        p, acc = torch.full((N1,), 0.5, device=cuda), torch.zeros(N1, device=cuda)
        g = torch.full((N1,), 0.25, device=cuda).to(gdt)
        pbf = torch.zeros(N1, device=cuda, dtype=torch.bfloat16)
        out = _lars(p, acc, g, pbf, ONE, 0.5, 0.0, wd, 2.0 ** -3, 0.0)
        assert out.tolist() == [[32.0, 16.0, r]]
        assert torch.equal(acc, torch.full_like(acc, 2.0 ** -5)) and torch.equal(p, torch.full_like(p, 0.46875))
        assert torch.equal(pbf, p.to(torch.bfloat16))
    # mu = 0.5 over two steps: every quantity stays a short binary fraction
    p, acc = torch.full((N1,), 0.5, device=cuda), torch.zeros(N1, device=cuda)
    g = torch.full((N1,), 0.25, device=cuda).to(gdt)
    rp, ra = p.double(), acc.double()
    for i in range(2):
        out = _lars(p, acc, g, None, ONE, 0.5, 0.5, 0.0, 2.0 ** -3, 0.0)
        rp, ra, nr = O.lars_update(rp, ra, g, 0.5, 0.5, 0.0, 2.0 ** -3, 0.0)
        assert out.double().tolist() == [list(nr)], (i, out, nr)
        assert torch.equal(p.double(), rp) and torch.equal(acc.double(), ra), i
    assert p[0].item() == 0.423828125 and acc[0].item() == 0.044921875


def test_lamb_exact_case_at_t1(cuda):
    """b1 = 0.5, b2 = 0.75, eps = 0, lambda = 0, lr = 0.25, g = +-0.25: m' = +-2^-3, v' = 2^-6, c_t = 1 (the
    device powf(b, 1) returns b), u = +-1, |u| = 64, |p| = 32, r = 0.5, p' = 0.5 -+ 0.125. Equality."""
    sign = torch.ones(N1, device=cuda)
    sign[1::2] = -1
    for step, off in ((None, 1), (torch.zeros(1, dtype=torch.int64, device=cuda), 1),
                      (torch.ones(1, dtype=torch.int64, device=cuda), 0)):
        p, m, v = torch.full((N1,), 0.5, device=cuda), torch.zeros(N1, device=cuda), torch.zeros(N1, device=cuda)
        out = _lamb(p, m, v, 0.25 * sign, None, ONE, 0.25, 0.5, 0.75, 0.0, 0.0, step=step, t_offset=off)
        assert out.tolist() == [[32.0, 64.0, 0.5]]
        assert torch.equal(m, 0.125 * sign) and torch.equal(v, torch.full_like(v, 2.0 ** -6))
        assert torch.equal(p, 0.5 - 0.125 * sign)


# ---------------------------------------------------------------- 3. guards and flags
def _guard_inputs(cuda, numel=4104):
    g = torch.Generator(device=cuda).manual_seed(5)
    p = torch.randn(numel, device=cuda, generator=g)
    grad = torch.randn(numel, device=cuda, generator=g)
    return p, grad


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_guards_flags_and_untouched_elements(cuda, kind):
    rows = [(0, 1000, BOTH), (1000, 1000, BOTH), (2000, 1001, LW_DECAY), (3004, 1000, LW_ADAPT)]  # gap [3001, 3004)
    numel = 4104  # and [4004, 4104) belongs to no variable
    p0, grad = _guard_inputs(cuda, numel)
    p0[0:1000] = 0       # |p| = 0
    grad[1000:2000] = 0  # |g| = 0
    outside = torch.ones(numel, dtype=torch.bool, device=cuda)
    for b, n, _ in rows:
        outside[b:b + n] = False

    def run(wd, rws):
        p, s1, s2 = p0.clone(), torch.full((numel,), 0.25, device=cuda), torch.full((numel,), 0.5, device=cuda)
        pbf = torch.full((numel,), 3.0, device=cuda, dtype=torch.bfloat16)
        ema = torch.full((numel,), 7.0, device=cuda)
        if kind == "lamb":
            out = _lamb(p, s1, s2, grad, pbf, rws, LR, B1, B2, EPS, wd, ema=ema, ema_decay=0.5)
        else:
            s1.zero_()
            out = _lars(p, s1, grad, pbf, rws, LR, MU, wd, EETA, 0.0, ema=ema, ema_decay=0.5)
        return p, s1, s2, pbf, ema, out

    p, s1, s2, pbf, ema, out = run(WD, rows)
    assert out[0].tolist()[0] == 0.0 and out[0].tolist()[2] == 1.0  # |p| = 0: r = 1 ...
    assert (p[0:1000] != 0).any()                                    # ... and the variable still moves
    if kind == "lars":
        assert out[1].tolist()[1] == 0.0 and out[1].tolist()[2] == 1.0  # |g| = 0: r = 1
    assert out[2].tolist()[2] == 1.0 and out[2].tolist()[0] > 0         # not adapted: r = 1 exactly
    assert out[3].tolist()[2] != 1.0
    # elements outside every variable: no buffer is touched
    assert torch.equal(p[outside], p0[outside])
    assert (s1[outside] == (0.25 if kind == "lamb" else 0.0)).all() and (s2[outside] == 0.5).all()
    assert (pbf[outside] == 3.0).all() and (ema[outside] == 7.0).all()
    assert not (ema[~outside] == 7.0).all() and torch.equal(pbf[~outside], p[~outside].to(torch.bfloat16))
    # a variable without LW_DECAY equals lambda = 0 bit for bit
    rows0 = [(b, n, BOTH) for b, n, _ in rows]
    q, t1, t2, qbf, qema, out0 = run(0.0, rows0)
    sl = slice(3004, 4004)
    assert torch.equal(p[sl], q[sl]) and torch.equal(s1[sl], t1[sl]) and torch.equal(s2[sl], t2[sl])
    assert torch.equal(out[3], out0[3]) and torch.equal(ema[sl], qema[sl])
    qq = run(WD, rows0)[0]
    assert not torch.equal(qq[sl], q[sl])  # the decay is felt where the flag is set


# ---------------------------------------------------------------- 4. against the fp64 definitions
# The bounds are the ones derived in csrc/layerwise.h, evaluated in fp64 on each update's own inputs: the
# reference of every update starts from the device's fp32 state before it, so the errors do not add up.
def _lamb_ref(p, m, v, g, t, lr, flags, b1=B1, b2=B2, eps=EPS, wd=WD):
    """fp64 reference and bounds of one variable: g is the fp64 gradient times its multiplier."""
    decay, adapt = bool(flags & LW_DECAY), bool(flags & LW_ADAPT)
    p2, m2, v2, (pn, un, r) = O.lamb_update(p, m, v, g, t, lr, b1, b2, eps, wd, decay, adapt)
    p, m, v = p.double(), m.double(), v.double()
    ct = math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    dm = 4 * U * (g.abs() + m.abs())
    dv = 5 * U * (g * g + v)
    s = v2.sqrt()
    den = s + eps
    dden = dv / (2 * s).clamp_min(1e-300) + 2 * U * den
    q = ct * m2 / den
    u = q + (wd if decay else 0.0) * p
    e_ct = 16 * U * (b2 ** t / (2 * (1 - b2 ** t)) + b1 ** t / (1 - b1 ** t)) + 4 * U
    du = q.abs() * (e_ct + 2 * U + dden / den) + ct * dm / den + U * u.abs()
    ndu = float(du.pow(2).sum().sqrt().item())
    e_r = (19 * U + ndu / un) if (adapt and pn > 0 and un > 0) else 0.0
    tol = {"pn": 9 * U * pn, "xn": 9 * U * un + ndu, "r": r * e_r, "m": dm + U * m2.abs(), "v": dv + U * v2.abs(),
           "p": lr * r * (du + u.abs() * (e_r + 2 * U)) + U * p2.abs()}
    return {"pn": pn, "xn": un, "r": r, "p": p2, "m": m2, "v": v2}, tol


def _lars_ref(p, acc, g, lr, flags, mu=MU, wd=WD, eeta=EETA, eps=0.0):
    decay, adapt = bool(flags & LW_DECAY), bool(flags & LW_ADAPT)
    lam = wd if decay else 0.0
    p2, a2, (pn, gn, r) = O.lars_update(p, acc, g, lr, mu, wd, eeta, eps, decay, adapt)
    p = p.double()
    e_r = 24 * U if r != 1.0 or (adapt and pn > 0 and gn > 0) else 0.0  # kLwLarsRatioUlps
    da = U * (a2.abs() + lr * r * 27 * (g + lam * p).abs() + lr * r * 2 * (g.abs() + lam * p.abs()))
    tol = {"pn": 9 * U * pn, "xn": 9 * U * gn, "r": r * e_r, "m": da, "p": da + U * p2.abs()}
    return {"pn": pn, "xn": gn, "r": r, "p": p2, "m": a2}, tol


def _check(dev, ref, tol):
    """(ok, worst error / bound) of one variable's device results against the reference."""
    worst, ok = 0.0, True
    for k in ref:
        err = (torch.as_tensor(dev[k]).double() - torch.as_tensor(ref[k]).double()).abs()
        bound = torch.as_tensor(tol[k]).double()
        ok = ok and bool((err <= bound).all().item())
        nz = bound > 0
        if bool(nz.any().item()):
            worst = max(worst, float((err[nz] / bound[nz]).max().item()))
    return ok, worst


def _dev_var(out, i, p, s1, s2, b, n):
    o = out[i].tolist()
    d = {"pn": o[0], "xn": o[1], "r": o[2], "p": p[b:b + n], "m": s1[b:b + n]}
    if s2 is not None:
        d["v"] = s2[b:b + n]
    return d


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
@pytest.mark.parametrize("name", ["ragged", "ones", "s300", "mnist"])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_flat_ops_follow_fp64(cuda, kind, name, gdt):
    """Six updates with fresh random gradients, multiplier grad_scale * *gscale = 0.5 * 0.75. Norms,
    ratios, p and the slots are held to the derived bounds; pbf is the bf16 rounding of the device's p'.
    Then a ratio off by 2 % in one variable must fail the same check."""
    rows, numel = _tables()[name]
    gen = torch.Generator(device=cuda).manual_seed(11)
    p = torch.randn(numel, device=cuda, generator=gen) * 0.05
    s1, s2 = torch.zeros(numel, device=cuda), torch.zeros(numel, device=cuda)
    pbf = torch.zeros(numel, device=cuda, dtype=torch.bfloat16)
    gscale = torch.tensor([0.75], device=cuda)
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    worst, last = 0.0, None
    inside = torch.zeros(numel, dtype=torch.bool, device=cuda)
    for b, n, _ in rows:
        inside[b:b + n] = True
    for t in range(1, 7):
        g = (torch.randn(numel, device=cuda, generator=gen) * 0.01).to(gdt)
        p0, a0, b0 = p.clone(), s1.clone(), s2.clone()
        kw = dict(step=step, t_offset=1, grad_scale=0.5, gscale=gscale)
        if kind == "lamb":
            out = _lamb(p, s1, s2, g, pbf, rows, LR, B1, B2, EPS, WD, **kw)
        else:
            out = _lars(p, s1, g, pbf, rows, LR, MU, WD, EETA, 0.0, **kw)
        step += 1
        g64 = g.double() * 0.375
        for i, (b, n, fl) in enumerate(rows):
            sl = slice(b, b + n)
            if kind == "lamb":
                ref, tol = _lamb_ref(p0[sl], a0[sl], b0[sl], g64[sl], t, LR, fl)
            else:
                ref, tol = _lars_ref(p0[sl], a0[sl], g64[sl], LR, fl)
            dev = _dev_var(out, i, p, s1, s2 if kind == "lamb" else None, b, n)
            ok, w = _check(dev, ref, tol)
            worst = max(worst, w)
            assert ok, (kind, name, t, i, w)
            if fl & LW_ADAPT:
                last = (dev, ref, tol, p0[sl], a0[sl], b0[sl], g64[sl], t, fl)
        assert torch.equal(pbf[inside], p[inside].to(torch.bfloat16)) and (pbf[~inside] == 0).all()
    print(f"layerwise {kind} {name} {gdt}: worst err / bound {worst:.4f}")
    assert 0 < worst <= 1
    # mutation: the same variable's reference with its ratio 2 % off
    dev, ref, tol, p0, a0, b0, g64, t, fl = last
    bad = dict(ref)
    bad["r"] = ref["r"] * 1.02
    bad["p"] = p0.double() + (ref["p"] - p0.double()) * 1.02
    ok, _ = _check(dev, bad, tol)
    assert not ok
    ok, _ = _check({**dev, "r": dev["r"] * 1.02}, ref, tol)
    assert not ok


# ---------------------------------------------------------------- 5. the engine
def _dataset(cuda, rows=ROWS, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(rows, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=cuda, generator=g)
    perm = torch.randperm(rows, device=cuda, generator=g).to(torch.int32)
    return data, labels, perm


def _set_opt(e, kind, sched=False):
    if kind == "lamb":
        e.set_lamb(LR, B1, B2, EPS, WD, True)
    elif kind == "lars":
        e.set_lars(LR, MU, WD, EETA, 0.0, True)
    else:
        e.set_adam(LR, 0.9, 0.999, 1e-8)
    if sched:
        e.set_lr_schedule(*schedule_args(SCHED))


def _engine(cuda, ds, dtype="bf16", kind="lamb", sched=False, ema=None, clip=None, keep=0.75, batch=B):
    e = torch.classes.tfd.MnistEngine(batch, 0, keep, 1234, 0)
    e.set_dtype(dtype)
    _set_opt(e, kind, sched)
    if clip is not None:
        e.set_clip_norm(clip)
    e.params().copy_(M.flat_from_dict(M.init_params(13)).to(cuda) * 0.05)
    e.sync_shadow()
    e.set_dataset(*ds)
    e.set_input_mode(1)
    if ema is not None:
        e.set_ema(ema, True)
    return e


def _state(e, ema=False, lw=True):
    s = {"params": e.params().clone(), "adam_m": e.adam_m().clone(), "adam_v": e.adam_v().clone(),
         "params_bf16": e.params_bf16().clone(), "step": e.step_tensor().clone(), "loss": e.loss_rows().clone()}
    if lw:
        s["layer_norms"] = e.layer_norms().clone()
    if ema:
        s["ema"] = e.ema_params().clone()
    return s


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())


def _opt_config(kind):
    if kind == "lamb":
        return O.LAMBOptimizer(LR, B1, B2, EPS, WD)
    return O.LARSOptimizer(LR, MU, WD, EETA, 0.0)


def _check_engine_update(kind, before, after, g64, t, lr=LR):
    """One engine update against the fp64 definitions, variable by variable: before / after are _state()s,
    g64 the fp64 gradient the optimizer consumed. Returns the worst error / bound."""
    worst = 0.0
    for i, (b, n, fl) in enumerate(M.segments(True)):
        sl = slice(b, b + n)
        if kind == "lamb":
            ref, tol = _lamb_ref(before["params"][sl], before["adam_m"][sl], before["adam_v"][sl], g64[sl], t, lr, fl)
        else:
            ref, tol = _lars_ref(before["params"][sl], before["adam_m"][sl], g64[sl], lr, fl)
        dev = _dev_var(after["layer_norms"], i, after["params"], after["adam_m"],
                       after["adam_v"] if kind == "lamb" else None, b, n)
        ok, w = _check(dev, ref, tol)
        assert ok, (kind, NAMES[i], t, w)
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_step_follows_the_fp64_applier(cuda, dtype, kind):
    """Three eager steps: after each, layer_norms(), params and the slots are within the derived bounds of
    the fp64 definitions fed the engine's own grads() and its state before the step; FlatApplier (the
    CPU workers' implementation, fp64 per variable) lands on the same values; padding stays untouched."""
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), dtype, kind)
        e.params()[M.NUM_PARAMS:] = 3.0  # the padding belongs to no variable
        e.sync_shadow()
        applier = O.FlatApplier(_opt_config(kind), M.TOTAL, cuda, M.segments(True))
        worst = 0.0
        for t in range(1, 4):
            before = _state(e)
            e.train_step()
            after = _state(e)
            g = e.grads().clone()
            worst = max(worst, _check_engine_update(kind, before, after, g.double(), t))
            # the applier from the same state: its fp32 results are the fp64 values rounded once
            applier.t = t - 1
            applier.m.copy_(before["adam_m"])
            if kind == "lamb":
                applier.v.copy_(before["adam_v"])
            q = before["params"].clone()
            applier.apply(q, g)
            tol = 1e-4 * LR  # |u| <= a few units: far above the derived bounds, far below one update
            assert (q - after["params"]).abs().max().item() <= tol
            for (pn, xn, r), row in zip(applier.last_layer_norms, after["layer_norms"].tolist()):
                assert abs(row[2] - r) <= 1e-3 * r and abs(row[0] - pn) <= 1e-5 * pn
            assert (after["params"][M.NUM_PARAMS:] == 3.0).all() and (after["adam_m"][M.NUM_PARAMS:] == 0).all()
            assert torch.equal(after["params_bf16"], after["params"].to(torch.bfloat16))
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 3
    ln = e.layer_norms().tolist()
    assert [row[2] == 1.0 for row in ln] == [False, True] * 4, ln  # biases are not adapted
    print(f"layerwise engine {kind} {dtype}: worst err / bound {worst:.4f}; ratios {[round(r[2], 5) for r in ln]}")


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graphs_equal_eager_under_a_schedule(cuda, dtype, kind):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        make = lambda: _engine(cuda, ds, dtype, kind, sched=True)  # noqa: E731
        eager, one, four = make(), make(), make()
        for _ in range(8):
            eager.train_step()
        one.train_step()
        one.capture_train_step("g1")
        one.replay("g1", 7)
        four.capture_train_steps("g4", 4)
        four.replay("g4", 2)
        const = _engine(cuda, ds, dtype, kind)
        for _ in range(8):
            const.train_step()
    torch.cuda.synchronize()
    for e in (one, four):
        assert int(e.step_tensor().item()) == 8
        _same(_state(e), _state(eager))
    assert not torch.equal(const.params(), eager.params())  # the schedule is felt


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ema_and_clip_compose(cuda, dtype, kind):
    """EMA: the shadow equals ema_flat applied after the step, bit for bit, and changes nothing else. An
    inactive clip changes no bit; an active one equals the update whose grad_scale carries the factor."""
    ops = torch.ops.tfd
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        plain = _engine(cuda, ds, dtype, kind)
        on = _engine(cuda, ds, dtype, kind, ema=0.9)
        loose = _engine(cuda, ds, dtype, kind, clip=1e6)
        ref = on.ema_params().clone()
        for _ in range(4):
            plain.train_step()
            loose.train_step()
            on.train_step()
            ops.ema_flat(ref, on.params(), 0.9, True, on.step_tensor(), 0)
            assert torch.equal(on.ema_params(), ref)
        _same(_state(on), _state(plain))
        _same(_state(loose), _state(plain))
        assert loose.grad_norm().tolist()[1] == 1.0 and not torch.equal(ref, on.params())
        # active clip, one more step from the same state
        norm = float(loose.grad_norm().tolist()[0])
        tight = _engine(cuda, ds, dtype, kind, clip=0.25 * norm)
        for k, src in (("params", plain.params()), ("adam_m", plain.adam_m()), ("adam_v", plain.adam_v())):
            getattr(tight, k)().copy_(src)
        tight.sync_shadow()
        tight.step_tensor().copy_(plain.step_tensor())
        before = _state(tight)
        tight.train_step()
        after = _state(tight)
        scale = float(tight.grad_norm().tolist()[1])
        assert 0 < scale < 1
        p, m, v, pbf = (before[k].clone() for k in ("params", "adam_m", "adam_v", "params_bf16"))
        kw = dict(step=tight.step_tensor(), t_offset=0, grad_scale=scale)
        segs = M.segments(True)
        if kind == "lamb":
            out = _lamb(p, m, v, tight.grads(), pbf, segs, LR, B1, B2, EPS, WD, **kw)
        else:
            out = _lars(p, m, tight.grads(), pbf, segs, LR, MU, WD, EETA, 0.0, **kw)
        _same({"params": p, "adam_m": m, "adam_v": v, "params_bf16": pbf, "layer_norms": out},
              {k: after[k] for k in ("params", "adam_m", "adam_v", "params_bf16", "layer_norms")})
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("mode,wire,dtype", [("ipc", "bf16", "bf16"), ("ipc", "fp32", "bf16"), ("rccl", "bf16", "bf16"),
                                             ("ipc", "fp32", "fp32")])
def test_forced_dp_world1_graph_equals_eager(cuda, mode, wire, dtype, kind):
    """The all-reduce schedule over a world-1 communicator; the norms are of the buffer the optimizer
    reads, the bf16 wire buffer when there is one."""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    ds = _dataset(cuda)
    trs = []

    def make():
        e = _engine(cuda, ds, dtype, kind, sched=True)
        trs.append(attach_engine(e, 0, 1, cuda, mode=mode, force_dp=True, bf16=wire == "bf16"))
        assert e.dp()
        return e

    with torch.cuda.stream(torch.cuda.Stream()):
        eager, graph = make(), make()
        for _ in range(7):
            eager.train_step()
        before = _state(eager)
        eager.train_step()
        after = _state(eager)
        graph.capture_train_steps("g", 4)
        graph.replay("g", 2)
        torch.cuda.synchronize()
        _same(_state(graph), after)
        buf = eager.grads_bf16() if wire == "bf16" else eager.grads()
        _check_engine_update(kind, before, after, buf.double(), 8, lr=O.lr_at(SCHED, 7))
    for tr in trs:
        tr.check()
        tr.close()


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("which", ["sfb", "zero"])
def test_sharded_schedules_raise_before_launching(cuda, which, kind):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), "bf16", kind)
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, sfb=which == "sfb", zero=which == "zero")
        if which == "zero":
            e.set_zero(True)
        before = _state(e)
        with pytest.raises(RuntimeError, match=f"set_{kind} conflicts with"):
            e.train_step()
        torch.cuda.synchronize()
        _same(_state(e), before)
        assert int(e.step_tensor().item()) == 0
        e.set_adam(LR, 0.9, 0.999, 1e-8)  # a flat optimizer again: the sharded schedule steps
        e.train_step()
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 1
    tr.check()
    tr.close()


# ---------------------------------------------------------------- 6. two ranks sharing the GPU over IPC
def _feeds(world):
    g = torch.Generator().manual_seed(7)
    return torch.rand(world * B, 784, generator=g), torch.randint(0, 10, (world * B,), generator=g, dtype=torch.int32)


def _ipc_worker(rank, world, kind):
    from tensorflow_distributed_amd.parallel.ipc import make_ipc_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = make_ipc_comm(rank, world, 0, M.TOTAL)
    eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 5, rank)
    _set_opt(eng, kind)
    eng.set_ipc(comm, 1 << 30, False)  # fp32 wire
    x, y = _feeds(world)
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.params().copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()}).to(dev))
        eng.sync_shadow()
        eng.feed_x().copy_(x[rank * B:(rank + 1) * B].to(dev))
        eng.feed_y().copy_(y[rank * B:(rank + 1) * B].to(dev))
        eng.train_step()
    torch.cuda.synchronize()
    out = (eng.params().cpu(), eng.adam_m().cpu(), eng.adam_v().cpu(), eng.layer_norms().cpu(), eng.grads().cpu(),
           int(eng.step_tensor().item()), comm.error(), eng.world())
    comm.close()
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_two_ranks_equal_each_other_and_one_rank_at_twice_the_batch(cuda, kind):
    """Both ranks form the norms of the same all-reduced gradient: identical ratios, identical replicas.
    Against one rank at batch 10 (dropout off): each run is within the derived bounds of the fp64
    definitions fed its own aggregated gradient, so the two differ by at most the two bounds plus the
    distance of the two fp64 results, which is evaluated here (the gradients of the two runs differ by
    the order of their fp32 sums, and in the bf16 step by the bf16 roundings those orders move).
    What catches what: a wrong aggregation inside the optimizer (local instead of aggregated norms, a
    wrong 1 / world) fails _check_engine_update(..., g2), which holds the two-rank result to the fp64
    definition of the AGGREGATED gradient within the derived bounds. The direct comparison of the two
    runs cannot be tighter than the gradient kernels' own agreement, which is not this file's subject:
    its `gap` term follows the two gradients, and the 1e-2 / 2e-2 checks on them and on the ratios only
    say that the two runs did train on the same ten images. run_ranks waits for each child under a
    timeout."""
    res = run_ranks(_ipc_worker, 2, kind, timeout=120)
    for r in res:
        assert r[6] == 0 and r[7] == 2 and r[5] == 1
        for a, b in zip(r[:5], res[0][:5]):
            assert torch.isfinite(a).all() and torch.equal(a, b), "replicas diverged"
    x, y = _feeds(2)
    with torch.cuda.stream(torch.cuda.Stream()):
        one = torch.classes.tfd.MnistEngine(2 * B, 0, 1.0, 5, 0)
        _set_opt(one, kind)
        one.params().copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()}).to(cuda))
        one.sync_shadow()
        one.feed_x().copy_(x.to(cuda))
        one.feed_y().copy_(y.to(cuda))
        before = _state(one)
        one.train_step()
        after = _state(one)
    torch.cuda.synchronize()
    g1 = one.grads().double()
    g2 = res[0][4].to(cuda).double() * 0.5  # the ranks' sum, times the 1 / world the optimizer applies
    assert float((g1 - g2).norm() / g1.norm()) < 1e-2  # the same gradient up to the order of its sums
    two = {"params": res[0][0].to(cuda), "adam_m": res[0][1].to(cuda), "adam_v": res[0][2].to(cuda),
           "layer_norms": res[0][3].to(cuda)}
    _check_engine_update(kind, before, after, g1, 1)
    _check_engine_update(kind, before, two, g2, 1)  # the norms are of the AGGREGATED gradient
    for i, (b, n, fl) in enumerate(M.segments(True)):
        sl = slice(b, b + n)
        refs = []
        for g in (g1, g2):
            if kind == "lamb":
                refs.append(_lamb_ref(before["params"][sl], before["adam_m"][sl], before["adam_v"][sl], g[sl], 1, LR, fl))
            else:
                refs.append(_lars_ref(before["params"][sl], before["adam_m"][sl], g[sl], LR, fl))
        (ra, ta), (rb, tb) = refs
        gap = (ra["p"] - rb["p"]).abs()
        err = (after["params"][sl].double() - two["params"][sl].double()).abs()
        assert (err <= ta["p"] + tb["p"] + gap).all(), (kind, NAMES[i])
        # and the ratios are those of one rank at twice the batch
        r1, r2 = after["layer_norms"][i, 2].item(), two["layer_norms"][i, 2].item()
        assert abs(r1 - r2) <= 2e-2 * r1, (kind, NAMES[i], r1, r2)


# ---------------------------------------------------------------- 7. the default is untouched
# capture_topology(1) of the default one-GPU bf16 Adam step at B = 32 (the list pinned by
# tests/test_clip_norm_gpu.py): six kernel nodes in a chain
PARENT_TOPOLOGY = ['node 0 0', 'node 1 0', 'node 2 0', 'node 3 0', 'node 4 0', 'node 5 0',
                   'edge 0 1', 'edge 1 2', 'edge 2 3', 'edge 3 4', 'edge 4 5',
                   'tag conv_fwd@0 0', 'tag fc_fwd@0 1 2', 'tag fc_bwd@0 3', 'tag conv_bwd@0 4', 'tag opt@0 5']


def test_default_step_is_what_it_was(cuda):
    ds = _dataset(cuda, rows=256)
    with torch.cuda.stream(torch.cuda.Stream()):
        never = _engine(cuda, ds, kind="adam", batch=32)
        back = _engine(cuda, ds, kind="lamb", batch=32)
        back.set_adam(LR, 0.9, 0.999, 1e-8)  # a layer-wise optimizer was chosen, then Adam again
        lw = _engine(cuda, ds, kind="lamb", batch=32)
        topo = {}
        for name, e in (("never", never), ("back", back), ("lw", lw)):
            e.capture_train_steps("g", 3)
            e.replay("g", 1)
            topo[name] = list(e.capture_topology(1))
    torch.cuda.synchronize()
    print("layer-wise topology:", topo["lw"])
    assert topo["never"] == PARENT_TOPOLOGY and topo["back"] == PARENT_TOPOLOGY
    assert topo["lw"] != PARENT_TOPOLOGY  # the serial schedule: slab reduce and the three stages are nodes
    assert int(never.step_tensor().item()) == 3
    _same(_state(never, lw=False), _state(back, lw=False))
    with pytest.raises(RuntimeError, match="set_lamb or set_lars first"):
        never.layer_norms()


# ---------------------------------------------------------------- 8. the runner
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_native_runner_takes_the_configs_and_round_trips(cuda, kind):
    """Slots under the optimizer's name by TF's slot-variable rule, no beta powers, last_layer_norms() by
    variable; a run resumed from the checkpoint is bit-identical to the uninterrupted one."""
    from tensorflow_distributed_amd.models.mnist_runner import NativeMnistRunner

    g = torch.Generator().manual_seed(5)
    xs = torch.rand(5, B, 784, generator=g)
    ys = torch.randint(0, 10, (5, B), generator=g, dtype=torch.int32)
    opt = O.LAMBOptimizer(LR, B1, B2, EPS, WD) if kind == "lamb" else O.LARSOptimizer(LR, MU, WD, EETA, 0.0)

    def runner():
        r = NativeMnistRunner(B, opt, keep_prob=0.75, seed=3, device=cuda)
        r.load_flat(M.flat_from_dict(M.init_params(13)) * 0.05, {}, 0)
        return r

    a = runner()
    assert a.last_layer_norms() == {}
    for i in range(3):
        a.train_step(xs[i], ys[i])
    ln = a.last_layer_norms()
    assert list(ln) == NAMES and [v[2] == 1.0 for v in ln.values()] == [False, True] * 4
    sd = a.state_dict_tf()
    slots = sorted(k for k in sd if "/" in k)
    names = ["/LAMB", "/LAMB_1"] if kind == "lamb" else ["/LARS"]
    assert slots == sorted(n + s for _, n, _ in M.PARAM_SPECS for s in names)
    assert "beta1_power" not in sd and int(sd["global_step"]) == 3
    b = runner()
    b.load_state_dict_tf(sd)
    for i in range(3, 5):
        a.train_step(xs[i], ys[i])
        b.train_step(xs[i], ys[i])
    assert a.global_step() == b.global_step() == 5
    assert torch.equal(a.params(), b.params()) and a.last_layer_norms() == b.last_layer_norms()
    for k, v in a.slot_tensors().items():
        assert torch.equal(v, b.slot_tensors()[k]), k
