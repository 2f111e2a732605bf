"""RMSProp and Adagrad on the device (csrc/optim_rules.h, csrc/kernels/optim_rules.hip, tfd::rmsprop_flat /
adagrad_flat, MnistEngine.set_rmsprop / set_adagrad): the exact cases through the flat ops, every size at
which the kernel takes another path with guard bands around every buffer, six updates against the fp64
definitions within bounds derived below, the guard / clip / EMA arguments, bad arguments, and the engine's
step -- against the fp64 applier, captured graphs, clipping, EMA, the non-finite guard, accumulation,
forced data-parallel schedules at world 1 -- and the runner's TF-named checkpoint.

Engines run at batch 8 on a synthetic 64-row dataset, on a side stream.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import schedule_args

pytestmark = pytest.mark.gpu

B, ROWS = 8, 64
U = 2.0 ** -24  # fp32 unit roundoff
LR, DECAY, MOM, EPS, ACC0 = 0.01, 0.9, 0.9, 1e-10, 0.1
SCHED = O.PiecewiseConstant([1, 2], [2.0 ** -7, 2.0 ** -9, 2.0 ** -11])  # both boundaries inside a 4-step graph
# the five instantiations: (momentum, centered)
KINDS = {"rms": (0.0, False), "rms_mom": (MOM, False), "cen": (0.0, True), "cen_mom": (MOM, True), "adagrad": None}
SLOTS = {"rms": ("ms", "mom"), "rms_mom": ("ms", "mom"), "cen": ("ms", "mom", "mg"), "cen_mom": ("ms", "mom", "mg"),
         "adagrad": ("accum",)}
GUARD = 8  # guard-band elements on either side: 32 B of fp32, 16 B of bf16, so the inner view stays aligned


def _apply(kind, p, s, g, pbf, lr=LR, decay=DECAY, eps=EPS, momentum=None, **kw):
    """The flat op of `kind` over the slot dict s."""
    ops = torch.ops.tfd
    if kind == "adagrad":
        return ops.adagrad_flat(p, s["accum"], g, pbf, lr, **kw)
    mom, centered = KINDS[kind]
    return ops.rmsprop_flat(p, s["ms"], s["mom"], g, pbf, lr, decay, mom if momentum is None else momentum, eps,
                            s.get("mg") if centered else None, **kw)


# ---------------------------------------------------------------- the bounds
# Per element, to first order, U = 2^-24. The device's g is the wire gradient times the fp32 multiplier:
# g (1 + e), |e| <= U (one rounding fewer where the compiler contracts the product into what follows).
# Every count below holds with or without contraction of the remaining operations: a contraction removes a
# rounding, and each line counts the separate form.
#
#   c = 1 - decay in fp32: fp32(decay) is within U decay of decay, the subtraction rounds once (not at
#     all for decay >= 0.5): E_c = (decay / (1 - decay) + 1) U relative -- 10 U at decay = 0.9, the term
#     a count of the update's own roundings misses
#   a = g g - ms:      |da|   <= 3 U g g + U |a|                (g twice, the product, the difference)
#   ms' = ms + a c:    |dms'| <= c |da| + |a| c (E_c + U) + U |ms'|
#   b = g - mg:        |db|   <= U |g| + U |b|
#   mg' = mg + b c:    |dmg'| <= c |db| + |b| c (E_c + U) + U |mg'|
#   d = ms' + eps:     |dd|   <= |dms'| + U eps + U |d|
#   centered d = ms' - mg' mg' + eps:
#                      |dd|   <= |dms'| + 2 |mg'| |dmg'| + U mg' mg' + U |ms' - mg' mg'| + U eps + U |d|
#     -- an absolute error: through the square root it is divided by d, NOT by ms', which is what the
#     cancellation in ms' - mg' mg' costs
#   delta = lr g / sqrt(d): relative  5 U + |dd| / (2 d)        (lr, g, the product, the root, the quotient)
#   mom' = momentum mom + delta: |dmom'| <= 2 U |momentum mom| + |delta| (5 U + |dd| / (2 d)) + U |mom'|
#   p' = p - mom':     |dp'|  <= |dmom'| + U |p'|
#   Adagrad: accum' = accum + g g: |daccum'| <= 3 U g g + U |accum'|; d = accum', delta and p' as above.
def _rule_ref(kind, p, s, g64, lr, decay=DECAY, eps=EPS):
    """(reference, bounds) of one update in fp64 from the fp32 state p, s and the fp64 gradient g64."""
    p = p.double()
    if kind == "adagrad":
        p2, a2 = O.adagrad_update(p, s["accum"], g64, lr)
        dacc = U * (3 * g64 ** 2 + a2.abs())
        delta = lr * g64 / a2.sqrt()
        return {"p": p2, "accum": a2}, {"p": delta.abs() * (5 * U + dacc / (2 * a2)) + U * p2.abs(), "accum": dacc}
    momentum, centered = KINDS[kind]
    ms, mom = s["ms"].double(), s["mom"].double()
    mg = s["mg"].double() if centered else None
    out = O.rmsprop_update(p, ms, mom, g64, lr, decay, momentum, eps, mg)
    p2, ms2, mom2 = out[:3]
    c = 1.0 - decay
    ec = (decay / c + 1.0) * U
    a = g64 ** 2 - ms
    dms = c * (3 * U * g64 ** 2 + U * a.abs()) + a.abs() * c * (ec + U) + U * ms2.abs()
    ref, tol = {"p": p2, "ms": ms2, "mom": mom2}, {"ms": dms}
    if centered:
        mg2 = out[3]
        b = g64 - mg
        dmg = c * U * (g64.abs() + b.abs()) + b.abs() * c * (ec + U) + U * mg2.abs()
        d = ms2 - mg2 ** 2 + eps
        dd = dms + 2 * mg2.abs() * dmg + U * (mg2 ** 2 + (ms2 - mg2 ** 2).abs() + eps + d.abs())
        ref["mg"], tol["mg"] = mg2, dmg
    else:
        d = ms2 + eps
        dd = dms + U * (eps + d.abs())
    delta = lr * g64 / d.sqrt()
    tol["mom"] = 2 * U * (momentum * mom).abs() + delta.abs() * (5 * U + dd / (2 * d)) + U * mom2.abs()
    tol["p"] = tol["mom"] + U * p2.abs()
    return ref, tol


def _check(dev, ref, tol, extra=None, by_key=None):
    """(ok, worst error / bound) of the device results against the reference; extra: a further absolute
    allowance per key (the fp32 rounding of a reference that was itself stored in fp32); by_key: a dict that
    collects the worst ratio of each quantity. The overall worst is p's and sits just under 1 whenever some p'
    lies right above a power of two: there U |p'|, the final rounding of p' alone, is all but the whole bound
    and half an ulp is all but U |p'|. The slots' ratios are the ones that speak about the rule's arithmetic."""
    worst, ok = 0.0, True
    for k in ref:
        err = (dev[k].double() - ref[k].double()).abs()
        bound = tol[k].double() + (extra[k].double() if extra else 0.0)
        ok = ok and bool((err <= bound).all().item())
        nz = bound > 0
        if bool(nz.any().item()):
            w = float((err[nz] / bound[nz]).max().item())
            worst = max(worst, w)
            if by_key is not None:
                by_key[k] = max(by_key.get(k, 0.0), w)
    return ok, worst


def _fresh_slots(kind, n, cuda):
    if kind == "adagrad":
        return {"accum": torch.full((n,), ACC0, device=cuda)}
    s = {"ms": torch.ones(n, device=cuda), "mom": torch.zeros(n, device=cuda)}
    if KINDS[kind][1]:
        s["mg"] = torch.zeros(n, device=cuda)
    return s


# ---------------------------------------------------------------- 1. exact cases
def _step_kw(cuda, mode, lr):
    """t = 1 from t_offset alone, or t = 2 from a device step of 5 and t_offset = -3 under a schedule whose rate
    is the case's only while s = t - 1 <= 2 (a kernel that ignored t_offset would read half the rate)."""
    if mode == "t_offset":
        return {}
    return dict(step=torch.full((1,), 5, dtype=torch.int64, device=cuda), t_offset=-3, lr_kind="piecewise",
                lr_params=[lr], lr_boundaries=[2], lr_values=[lr, lr / 2])


@pytest.mark.parametrize("with_pbf", [False, True], ids=["no_pbf", "pbf"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_exact_cases_through_the_flat_ops(cuda, gdt, with_pbf):
    """Every quantity is a short binary fraction, so fp32 is exact whatever is contracted. Equality."""
    n = 4099  # float4 items of more than one block, and a scalar tail
    full = lambda v, dt=torch.float32: torch.full((n,), v, device=cuda, dtype=dt)  # noqa: E731
    for label in ("t_offset", "device_step"):
        kw = _step_kw(cuda, label, 0.25)
        pbf = full(9.0, torch.bfloat16) if with_pbf else None
        # RMSProp with momentum: p=1, ms=.25, mom=0, g=.5, lr=.25, decay=.5, momentum=.5, eps=0, two updates
        p, s = full(1.0), {"ms": full(0.25), "mom": full(0.0)}
        for want in ((0.75, 0.25, 0.25), (0.375, 0.25, 0.375)):
            _apply("rms_mom", p, s, full(0.5, gdt), pbf, lr=0.25, decay=0.5, eps=0.0, momentum=0.5, **kw)
            got = (p, s["ms"], s["mom"])
            assert all(torch.equal(x, full(w)) for x, w in zip(got, want)), (label, [x[0].item() for x in got], want)
            assert pbf is None or torch.equal(pbf, p.to(torch.bfloat16))
        # centered, momentum 0: p=1, ms=1.5, mg=0, g=1, lr=.25, decay=.5: ms'=1.25, mg'=.5, d=1, mom'=.25, p'=.75
        p, s = full(1.0), {"ms": full(1.5), "mom": full(0.0), "mg": full(0.0)}
        _apply("cen", p, s, full(1.0, gdt), pbf, lr=0.25, decay=0.5, eps=0.0, **kw)
        got = (p, s["ms"], s["mg"], s["mom"])
        assert all(torch.equal(x, full(w)) for x, w in zip(got, (0.75, 1.25, 0.5, 0.25))), (label, [x[0].item() for x in got])
        assert pbf is None or torch.equal(pbf, p.to(torch.bfloat16))
        # Adagrad: accum=.1875, g=.25, lr=.5, p=1: accum'=.25, p'=.75
        p, s = full(1.0), {"accum": full(0.1875)}
        _apply("adagrad", p, s, full(0.25, gdt), pbf, lr=0.5, **_step_kw(cuda, label, 0.5))
        assert torch.equal(p, full(0.75)) and torch.equal(s["accum"], full(0.25)), (label, p[0].item())
        assert pbf is None or torch.equal(pbf, p.to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["rms", "cen"])
def test_momentum_zero_neither_reads_nor_skips_the_mom_slot(cuda, kind):
    """momentum == 0: the result does not depend on what mom held -- inf included -- and mom' is stored."""
    n = 1031
    runs = []
    for sentinel in (7.0, float("inf"), float("nan")):
        p = torch.full((n,), 1.0, device=cuda)
        s = {"ms": torch.full((n,), 0.25 if kind == "rms" else 1.5, device=cuda), "mom": torch.full((n,), sentinel, device=cuda),
             "mg": torch.zeros(n, device=cuda)}
        g = torch.full((n,), 0.5 if kind == "rms" else 1.0, device=cuda)
        _apply(kind, p, s, g, None, lr=0.25, decay=0.5, eps=0.0)
        runs.append((p, s["ms"], s["mom"]))
        assert torch.equal(s["mom"], torch.full_like(p, 0.25)) and torch.equal(p, torch.full_like(p, 0.75)), sentinel
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))


# ---------------------------------------------------------------- 2. sizes and guard bands
def _sizes():
    return [1, 3, 4, 5, 1023, 4099, int(torch.ops.tfd.rules_grid_elems()) + 1027]


def _banded(n, value_fn, cuda, dt=torch.float32, band=123.0):
    """A buffer of GUARD + n + GUARD elements, the bands holding `band`, and its inner view."""
    buf = torch.full((n + 2 * GUARD,), band, device=cuda, dtype=dt)
    buf[GUARD:GUARD + n] = value_fn().to(dt)
    return buf, buf[GUARD:GUARD + n]


def _bands_intact(buf, n, band=123.0):
    return bool((buf[:GUARD] == band).all().item() and (buf[GUARD + n:] == band).all().item())


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_size_stays_inside_its_buffers(cuda, kind, gdt):
    """One update at each size, the last one above the largest grid x 256 x 4 with a ragged end, so that the
    second grid-stride pass and the scalar tail both run: every element within the derived bounds, every guard
    band bit for bit."""
    assert _sizes()[-1] == 2048 * 256 * 4 + 1027
    gen = torch.Generator(device=cuda).manual_seed(3)
    rnd = lambda n, sc: (lambda: torch.randn(n, device=cuda, generator=gen) * sc)  # noqa: E731
    for n in _sizes():
        bufs = {"p": _banded(n, rnd(n, 0.05), cuda), "g": _banded(n, rnd(n, 0.01), cuda, gdt),
                "pbf": _banded(n, lambda: torch.zeros(n, device=cuda), cuda, torch.bfloat16),
                "ema": _banded(n, rnd(n, 0.05), cuda)}
        for name in SLOTS[kind]:  # slots as after some updates: positive ms / accum, small mom / mg
            fn = (lambda: torch.rand(n, device=cuda, generator=gen) * 1e-3 + 1e-4) if name in ("ms", "accum") else rnd(n, 1e-3)
            bufs[name] = _banded(n, fn, cuda)
        p, g, pbf, ema = (bufs[k][1] for k in ("p", "g", "pbf", "ema"))
        s = {k: bufs[k][1] for k in SLOTS[kind]}
        if "mg" in s:  # a variance estimate: ms >= mg^2 with room
            s["mg"].mul_(0.1)
        p0, s0, e0 = p.clone(), {k: v.clone() for k, v in s.items()}, ema.clone()
        _apply(kind, p, s, g, pbf, ema=ema, ema_decay=0.75)
        ref, tol = _rule_ref(kind, p0, s0, g.double(), LR)
        ok, worst = _check({"p": p, **s}, ref, tol)
        assert ok, (kind, n, worst)
        assert torch.equal(pbf, p.to(torch.bfloat16)), (kind, n)
        want_e = e0.clone()
        torch.ops.tfd.ema_flat(want_e, p, 0.75)
        assert torch.equal(ema, want_e), (kind, n)
        for k, (buf, _) in bufs.items():
            assert _bands_intact(buf, n), (kind, n, k)


# ---------------------------------------------------------------- 3. six updates against fp64
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_flat_ops_follow_fp64(cuda, kind, gdt):
    """Six updates with fresh random gradients, multiplier grad_scale * *gscale = 0.5 * 0.75; the reference
    restarts from the device's previous state each step. p and every slot are held to the derived bounds; pbf
    is the bf16 rounding of the device's p'. Then a reference whose lr, or decay, is 2 % off must fail."""
    n = 20003
    gen = torch.Generator(device=cuda).manual_seed(11)
    p = torch.randn(n, device=cuda, generator=gen) * 0.05
    s = _fresh_slots(kind, n, cuda)
    pbf = torch.zeros(n, device=cuda, dtype=torch.bfloat16)
    gscale = torch.tensor([0.75], device=cuda)
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    worst, keys = 0.0, {}
    for t in range(1, 7):
        g = (torch.randn(n, device=cuda, generator=gen) * 0.01).to(gdt)
        p0, s0 = p.clone(), {k: v.clone() for k, v in s.items()}
        _apply(kind, p, s, g, pbf, step=step, t_offset=1, grad_scale=0.5, gscale=gscale)
        step += 1
        g64 = g.double() * 0.375
        ref, tol = _rule_ref(kind, p0, s0, g64, LR)
        dev = {"p": p, **s}
        ok, w = _check(dev, ref, tol, by_key=keys)
        worst = max(worst, w)
        assert ok, (kind, t, w)
        assert torch.equal(pbf, p.to(torch.bfloat16))
    print(f"rules flat {kind} {str(gdt).split('.')[-1]}: worst err / bound {worst:.4f}; by quantity "
          + ", ".join(f"{k} {v:.4f}" for k, v in keys.items()))
    assert 0 < worst <= 1
    # mutations, against the last update: the same check must refuse a reference that is 2 % off
    bad, _ = _rule_ref(kind, p0, s0, g64, LR * 1.02)
    assert not _check(dev, bad, tol)[0]
    if kind != "adagrad":
        bad, _ = _rule_ref(kind, p0, s0, g64, LR, decay=DECAY * 1.02)
        assert not _check(dev, bad, tol)[0]


# ---------------------------------------------------------------- 4. guard, clip and EMA arguments
def _inputs(kind, n, cuda, seed=5):
    gen = torch.Generator(device=cuda).manual_seed(seed)
    p = torch.randn(n, device=cuda, generator=gen) * 0.05
    g = torch.randn(n, device=cuda, generator=gen) * 0.01
    return p, _fresh_slots(kind, n, cuda), g


@pytest.mark.parametrize("kind", list(KINDS))
def test_guard_clip_and_ema_arguments(cuda, kind):
    n = 4101
    ops = torch.ops.tfd

    def run(**kw):
        p, s, g = _inputs(kind, n, cuda)
        pbf = torch.full((n,), 3.0, device=cuda, dtype=torch.bfloat16)
        _apply(kind, p, s, g, pbf, **kw)
        return {"p": p, "pbf": pbf, **s}

    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)  # noqa: E731
    plain = run()
    p0, s0, _ = _inputs(kind, n, cuda)
    assert not torch.equal(plain["p"], p0)
    # guard = 1 (the [3] result's ok, and a one-element view) equals no guard; gscale = 1.0 equals no clip
    ok3 = torch.tensor([2.0, 1.0, 1.0], device=cuda)
    assert same(run(guard=ok3), plain) and same(run(guard=ok3[2:]), plain)
    assert same(run(gscale=torch.ones(1, device=cuda)), plain)
    # a clip factor is a multiplier of the gradient: 0.5 through gscale equals 0.5 through grad_scale
    assert same(run(gscale=torch.full((1,), 0.5, device=cuda)), run(grad_scale=0.5))
    assert not same(run(grad_scale=0.5), plain)
    # guard = 0 stores nothing: every buffer and the shadow keep their bits
    ema = torch.full((n,), 7.0, device=cuda)
    skipped = run(guard=torch.tensor([float("inf"), 0.0, 0.0], device=cuda), ema=ema, ema_decay=0.5)
    assert torch.equal(skipped["p"], p0) and (skipped["pbf"] == 3.0).all() and (ema == 7.0).all()
    assert all(torch.equal(skipped[k], s0[k]) for k in s0)
    # the shadow equals ema_flat applied after the same update, and the update does not feel it
    for nu in (False, True):
        step = torch.full((1,), 4, dtype=torch.int64, device=cuda)
        ema = p0.clone() + 0.01
        want = ema.clone()
        got = run(ema=ema, ema_decay=0.9, ema_num_updates=nu, step=step, t_offset=1)
        assert same(got, plain)
        ops.ema_flat(want, got["p"], 0.9, nu, step, 1)
        assert torch.equal(ema, want) and not torch.equal(ema, p0 + 0.01)


def test_bad_arguments_raise_before_launching(cuda):
    n = 64
    z = lambda dt=torch.float32, dev=cuda, m=n: torch.zeros(m, dtype=dt, device=dev)  # noqa: E731
    ops = torch.ops.tfd
    ones = torch.ones(n, device=cuda)

    def rms(p=None, ms=None, mom=None, g=None, pbf=None, mg=None, **kw):
        p = z() if p is None else p
        ops.rmsprop_flat(p, ones.clone() if ms is None else ms, z() if mom is None else mom, z() if g is None else g, pbf,
                         LR, DECAY, 0.0, EPS, mg, **kw)
        return p

    rms()  # the baseline call is fine
    bad = [dict(p=z(torch.float64)), dict(ms=z(torch.float64)), dict(g=z(torch.float16)), dict(pbf=z(torch.float32)),
           dict(g=z(dev="cpu")), dict(mom=z(dev="cpu")),
           dict(p=z(m=2 * n)[::2]), dict(g=z(m=2 * n)[::2]), dict(ms=z(m=2 * n)[::2]),
           dict(ms=z(m=n + 4)), dict(g=z(m=n - 4)), dict(pbf=z(torch.bfloat16, m=n + 4)), dict(mg=z(m=n + 4)),
           dict(mg=z(torch.float64)), dict(mg=z(dev="cpu")),  # mg given is the centered rule: it is checked as a slot
           dict(p=z(m=n + 1)[1:], ms=z(m=n + 1)[1:], mom=z(m=n + 1)[1:], g=z(m=n + 1)[1:]),  # 4-byte aligned only
           dict(ema=z(), ema_decay=1.5), dict(ema=z(m=n + 4), ema_decay=0.5),
           dict(lr_kind="piecewise", lr_params=[LR], lr_boundaries=[2], lr_values=[LR, LR / 2]),  # a schedule needs step
           dict(step=torch.zeros(1, dtype=torch.int32, device=cuda)), dict(gscale=torch.ones(2, device=cuda)),
           dict(guard=torch.ones(2, device=cuda)), dict(guard=torch.ones(1)), dict(gscale=torch.ones(1)),
           dict(step=torch.zeros(1, dtype=torch.int64))]  # on the host
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            rms(**kw)
    for kw in (dict(accum=z(torch.float64)), dict(accum=z(m=n + 4)), dict(g=z(m=n + 4)), dict(accum=z(dev="cpu"))):
        args = dict(accum=ones.clone(), g=z())
        args.update(kw)
        with pytest.raises((RuntimeError, NotImplementedError)):
            ops.adagrad_flat(z(), args["accum"], args["g"], None, LR)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. the engine
ENGINE_KINDS = ["rms", "cen_mom", "adagrad"]


def _dataset(cuda, rows=ROWS, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(rows, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=cuda, generator=g)
    perm = torch.randperm(rows, device=cuda, generator=g).to(torch.int32)
    return data, labels, perm


def _set_opt(e, kind, sched=False):
    if kind == "adagrad":
        e.set_adagrad(LR, ACC0)
    else:
        e.set_rmsprop(LR, DECAY, KINDS[kind][0], EPS, KINDS[kind][1])
    if sched:
        e.set_lr_schedule(*schedule_args(SCHED))


def _config(kind, **kw):
    if kind == "adagrad":
        return O.AdagradOptimizer(LR, ACC0, **kw)
    return O.RMSPropOptimizer(LR, DECAY, KINDS[kind][0], EPS, KINDS[kind][1], **kw)


def _engine(cuda, ds, dtype="bf16", kind="rms", sched=False, ema=None, clip=None, guard=False, accum=1, batch=B):
    e = torch.classes.tfd.MnistEngine(batch, 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    _set_opt(e, kind, sched)
    if clip is not None:
        e.set_clip_norm(clip)
    if guard:
        e.set_skip_nonfinite(True)
    e.params().copy_(M.flat_from_dict(M.init_params(13)).to(cuda) * 0.05)
    e.sync_shadow()
    if accum > 1:
        e.set_grad_accum(accum)
    if ds is not None:
        e.set_dataset(*ds)
        e.set_input_mode(1)
    if ema is not None:
        e.set_ema(ema, True)
    return e


def _eng_slots(e, kind):
    """The engine's slots under the names of the definitions."""
    if kind == "adagrad":
        return {"accum": e.adam_v()}
    s = {"ms": e.adam_v(), "mom": e.adam_m()}
    if KINDS[kind][1]:
        s["mg"] = e.slot3()
    return s


def _state(e, kind, ema=False):
    s = {"params": e.params().clone(), "params_bf16": e.params_bf16().clone(), "step": e.step_tensor().clone(),
         "loss": e.loss_rows().clone()}
    s.update({k: v.clone() for k, v in _eng_slots(e, kind).items()})
    if ema:
        s["ema"] = e.ema_params().clone()
    return s


def _same(a, b, finite=True):
    assert a.keys() == b.keys()
    for k in a:
        assert not finite or torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())


@pytest.mark.parametrize("kind", ["rms", "cen", "adagrad"])
def test_setters_leave_the_slots_at_tfs_initial_values(cuda, kind):
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, None, "bf16", "rms_mom")
        e.adam_m().fill_(5.0)
        e.adam_v().fill_(5.0)
        _set_opt(e, kind)
        s = _eng_slots(e, kind)
    torch.cuda.synchronize()
    want = {"ms": 1.0, "mom": 0.0, "mg": 0.0, "accum": float(np.float32(ACC0))}
    for k, v in s.items():
        assert v.shape == (M.TOTAL,) and (v == want[k]).all(), k
    if kind != "cen":
        fresh = torch.classes.tfd.MnistEngine(B, 0, 0.75, 1, 0)
        with pytest.raises(RuntimeError, match="slot3"):
            fresh.slot3()


@pytest.mark.parametrize("kind", ENGINE_KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_step_follows_the_fp64_applier(cuda, dtype, kind):
    """Four eager steps: after each, params and the slots are within the derived bounds of FlatApplier (the
    fp64 definition, stored in fp32: one more rounding of each value) fed the engine's own grads() from the
    engine's state before the step. Two engines run bit-identically."""
    with torch.cuda.stream(torch.cuda.Stream()):
        ds = _dataset(cuda)
        e, twin = _engine(cuda, ds, dtype, kind), _engine(cuda, ds, dtype, kind)
        applier = O.FlatApplier(_config(kind), M.TOTAL, cuda)
        worst, keys = 0.0, {}
        for t in range(1, 5):
            before = _state(e, kind)
            e.train_step()
            twin.train_step()
            after = _state(e, kind)
            g = e.grads().clone()
            s0 = {k: before[k] for k in SLOTS[kind]}
            _, tol = _rule_ref(kind, before["params"], s0, g.double(), LR)
            applier.t = t - 1
            for k in SLOTS[kind]:
                applier.slots()[k].copy_(before[k])
            q = before["params"].clone()
            applier.apply(q, g)
            ref = {"p": q, **applier.slots()}
            ok, w = _check({"p": after["params"], **{k: after[k] for k in SLOTS[kind]}}, ref, tol,
                           extra={k: U * v.abs() for k, v in ref.items()}, by_key=keys)
            assert ok, (kind, dtype, t, w)
            worst = max(worst, w)
            assert torch.equal(after["params_bf16"], after["params"].to(torch.bfloat16))
            assert not torch.equal(after["params"], before["params"])
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 4
    _same(_state(e, kind), _state(twin, kind))
    print(f"rules engine {kind} {dtype}: worst err / bound {worst:.4f}; by quantity "
          + ", ".join(f"{k} {v:.4f}" for k, v in keys.items()))
    assert 0 < worst <= 1


@pytest.mark.parametrize("kind", ENGINE_KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graphs_equal_eager_under_a_schedule(cuda, dtype, kind):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        make = lambda: _engine(cuda, ds, dtype, kind, sched=True)  # noqa: E731
        eager, one, four = make(), make(), make()
        for _ in range(4):
            eager.train_step()
        one.train_step()
        one.capture_train_step("g1")
        one.replay("g1", 3)
        four.capture_train_steps("g4", 4)
        four.replay("g4", 1)
        const = _engine(cuda, ds, dtype, kind)
        for _ in range(4):
            const.train_step()
    torch.cuda.synchronize()
    for e in (one, four):
        assert int(e.step_tensor().item()) == 4
        _same(_state(e, kind), _state(eager, kind))
    assert not torch.equal(const.params(), eager.params())  # the schedule is felt


@pytest.mark.parametrize("kind", ENGINE_KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_clip_ema_and_accumulation_compose(cuda, dtype, kind):
    """EMA: the shadow equals ema_flat applied after each step and changes nothing else. An inactive clip
    changes no bit; an active one equals the flat op whose grad_scale carries the factor. Accumulation over two
    micro-batches: the captured graph equals eager and two runs agree."""
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
        _same(_state(on, kind), _state(plain, kind))
        _same(_state(loose, kind), _state(plain, kind))
        assert loose.grad_norm().tolist()[1] == 1.0 and not torch.equal(ref, on.params())
        # active clip, one more step from the same state
        norm = float(loose.grad_norm().tolist()[0])
        tight = _engine(cuda, ds, dtype, kind, clip=0.25 * norm)
        tight.params().copy_(plain.params())
        for k, v in _eng_slots(plain, kind).items():
            _eng_slots(tight, kind)[k].copy_(v)
        tight.sync_shadow()
        tight.step_tensor().copy_(plain.step_tensor())
        before = _state(tight, kind)
        tight.train_step()
        after = _state(tight, kind)
        scale = float(tight.grad_norm().tolist()[1])
        assert 0 < scale < 1
        p, pbf = before["params"].clone(), before["params_bf16"].clone()
        s = {k: before[k].clone() for k in SLOTS[kind]}
        _apply(kind, p, s, tight.grads(), pbf, step=tight.step_tensor(), t_offset=0, grad_scale=scale)
        _same({"params": p, "params_bf16": pbf, **s}, {k: after[k] for k in ["params", "params_bf16", *SLOTS[kind]]})
        # accumulation
        acc = [_engine(cuda, ds, dtype, kind, accum=2) for _ in range(3)]
        for _ in range(4):
            acc[0].train_step()
            acc[1].train_step()
        acc[2].capture_train_steps("g", 2)
        acc[2].replay("g", 2)
    torch.cuda.synchronize()
    for e in acc[1:]:
        assert int(e.step_tensor().item()) == 4
        _same(_state(e, kind), _state(acc[0], kind))
    assert not torch.equal(acc[0].params(), plain.params())


def _batches(k, rows=B, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(rows, 784, generator=g), torch.randint(0, 10, (rows,), generator=g, dtype=torch.int32))
            for _ in range(k)]


def _feed(e, xy, cuda):
    e.feed_x().copy_(xy[0].to(cuda))
    e.feed_y().copy_(xy[1].to(cuda))


@pytest.mark.parametrize("kind", ENGINE_KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_poisoned_step_is_an_identity_update(cuda, dtype, kind):
    """Host feed, one inf pixel in the second batch: parameters, every slot and the shadow keep their bits,
    the step is consumed and the skipped-step counter goes to 1; finite steps equal the unguarded twin's."""
    b0, b1, b2 = _batches(3)
    b1[0][2, 14 * 28 + 14] = float("inf")
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, None, dtype, kind, guard=True, ema=0.9)
        twin = _engine(cuda, None, dtype, kind, clip=1e30, ema=0.9)
        for eng in (e, twin):
            _feed(eng, b0, cuda)
            eng.train_step()
        torch.cuda.synchronize()
        before = _state(e, kind, ema=True)
        _same(before, _state(twin, kind, ema=True))
        _feed(e, b1, cuda)
        e.train_step()
        torch.cuda.synchronize()
        after = _state(e, kind, ema=True)
        assert not np.isfinite(e.grad_norm()[0].item())
        assert int(after.pop("step").item()) == int(before.pop("step").item()) + 1 == 2
        after.pop("loss"), before.pop("loss")
        _same(after, before)
        assert e.skipped_steps() == 1 and not e.last_step_ok()
        twin.step_tensor().copy_(e.step_tensor())
        twin.sync_micro_step()
        for eng in (e, twin):
            _feed(eng, b2, cuda)
            eng.train_step()
    torch.cuda.synchronize()
    _same(_state(e, kind, ema=True), _state(twin, kind, ema=True))
    assert e.skipped_steps() == 1 and e.last_step_ok() and int(e.step_tensor().item()) == 3
    assert not torch.equal(e.params(), before["params"])


@pytest.mark.parametrize("kind", ["cen_mom", "adagrad"])
@pytest.mark.parametrize("which", ["allreduce", "sfb", "zero"])
def test_forced_dp_world1_graph_equals_eager(cuda, which, kind):
    """Each DP schedule over a world-1 IPC communicator with a bf16 wire: the rule is reached through
    apply_optimizer_range, over the fc / conv regions or the ZeRO-1 shard ranges."""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    ds = _dataset(cuda)
    trs = []

    def make():
        e = _engine(cuda, ds, "bf16", kind, sched=True)
        trs.append(attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, bf16=True, sfb=which == "sfb",
                                 zero=which == "zero"))
        if which == "zero":
            e.set_zero(True)
        assert e.dp()
        return e

    def whole(e):
        e.sync_params()
        torch.cuda.synchronize()
        return _state(e, kind)

    with torch.cuda.stream(torch.cuda.Stream()):
        eager, graph = make(), make()
        start = eager.params().clone()
        for _ in range(4):
            eager.train_step()
        graph.capture_train_steps("g", 2)
        graph.replay("g", 2)
        torch.cuda.synchronize()
        a, b = whole(graph), whole(eager)
    _same(a, b)
    assert int(eager.step_tensor().item()) == 4 and not torch.equal(eager.params(), start)
    assert torch.equal(b["params_bf16"], b["params"].to(torch.bfloat16))
    for tr in trs:
        tr.check()
        tr.close()


# ---------------------------------------------------------------- 6. the runner
@pytest.mark.parametrize("kind", ["rms", "cen_mom", "adagrad"])
def test_native_runner_saves_tf_named_slots_and_resumes(cuda, kind):
    from tensorflow_distributed_amd.models.mnist_runner import NativeMnistRunner

    cfg = _config(kind)
    b = _batches(3)
    init = M.flat_from_dict(M.init_params(13)) * 0.05

    def make():
        r = NativeMnistRunner(B, cfg, keep_prob=0.75, seed=7, device=cuda, use_graph=False)
        r.load_flat(init, {}, 0)
        return r

    a = make()
    assert set(a.slot_tensors()) == set(SLOTS[kind])
    for xy in b[:2]:
        a.train_step(*xy)
    sd = a.state_dict_tf()
    suffixes = {"rms": ["/RMSProp", "/RMSProp_1"], "cen_mom": ["/RMSProp", "/RMSProp_1", "/RMSProp_2"],
                "adagrad": ["/Adagrad"]}[kind]
    slot_of = {"rms": ["ms", "mom"], "cen_mom": ["ms", "mg", "mom"], "adagrad": ["accum"]}[kind]
    for key, tf_name, _ in M.PARAM_SPECS:
        for suf, slot in zip(suffixes, slot_of):
            want = M.dict_from_flat(a.slot_tensors()[slot].detach().float().cpu())[key].numpy()
            assert np.array_equal(sd[tf_name + suf], want), (tf_name, suf)
        assert tf_name + suffixes[-1] + "x" not in sd and (tf_name + "/Adam") not in sd
    assert int(sd["global_step"]) == 2
    r = make()
    r.load_state_dict_tf(sd)
    for run in (a, r):
        run.train_step(*b[2])
    torch.cuda.synchronize()
    assert r.global_step() == a.global_step() == 3
    n = M.NUM_PARAMS  # the padding behind the variables is in no checkpoint
    assert torch.equal(r.params()[:n], a.params()[:n])
    for k in SLOTS[kind]:
        assert torch.equal(r.slot_tensors()[k][:n], a.slot_tensors()[k][:n]), k
    assert not torch.equal(a.params().cpu(), init)
