"""The flat Adam / Momentum / SGD kernels (csrc/optim_kernels.h; tfd::adam_flat, adam_ranges_flat, momentum_flat,
momentum_ema_flat) against the fp64 definitions, element by element, within the bounds derived in
tests/flat_optim_oracle.py: exact cases, every size at which a kernel takes another path with guard bands around
every buffer, the device's bias-corrected rate read bit for bit, six updates, the ranges form over its index map's
edges and MNIST's ZeRO-1 tables, the bf16 rounding every shadow equality leans on, and the ops' argument checks.

References are formed in fp64 on the device with plain torch; each update restarts from the device's previous fp32
state. Every launched call passes its op's checks.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flat_optim_oracle as FO  # noqa: E402

from tensorflow_distributed_amd.training import optimizers as O  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8  # guard-band elements on either side: 32 B of fp32, 16 B of bf16, so the inner view stays aligned
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
MOM, WD = 0.9, 1e-4
SCHED = O.PiecewiseConstant([1, 2], [2.0 ** -7, 2.0 ** -9, 2.0 ** -11])  # powers of two: the device rate is exact
PROBE_SCHED = O.PiecewiseConstant([5, 5000], [2.0 ** -7, 2.0 ** -9, 2.0 ** -11])
VARIANTS = ["plain", "clip", "ema", "guard", "ema_guard"]
GDTS = pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
SCHEDS = pytest.mark.parametrize("sched", [None, SCHED], ids=["const", "sched"])
ADAM_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, FO.GRID4 + 1027]
SGD_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, FO.GRID1 + 259, 2 * FO.GRID1 + 3]
EMA_DECAY = 0.75


def _bits(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sched_args(sched, lr):
    """(lr, kind, params, boundaries, values) as the flat ops take them."""
    if sched is None:
        return lr, "constant", [], [], []
    kind, params, bnd, vals = O.schedule_args(sched)
    return params[0], kind, params, bnd, vals


def _rate(sched, lr, t):
    """The rate of the update whose count is t: the schedule reads global_step before the update."""
    return lr if sched is None else O.lr_at(sched, t - 1)


def _adam(p, m, v, g, pbf, lr=LR, b1=B1, b2=B2, eps=EPS, step=None, t_offset=1, grad_scale=1.0, sched=None, ranges=None,
          **mods):
    lr0, kind, params, bnd, vals = _sched_args(sched, lr)
    tail = (lr0, b1, b2, eps, step, grad_scale, t_offset, kind, params, bnd, vals)
    if ranges is None:
        torch.ops.tfd.adam_flat(p, m, v, g, pbf, *tail, **mods)
    else:
        torch.ops.tfd.adam_ranges_flat(p, m, v, g, pbf, [b for b, _ in ranges], [n for _, n in ranges], *tail, **mods)


def _sgd(p, mom, g, pbf, lr=0.01, momentum=MOM, wd=WD, nesterov=False, step=None, t_offset=1, grad_scale=1.0, sched=None,
         gscale=None, guard=None, ema=None, ema_decay=EMA_DECAY):
    lr0, kind, params, bnd, vals = _sched_args(sched, lr)
    args = (p, mom, g, pbf, lr0, momentum, wd, nesterov, grad_scale, step, t_offset, kind, params, bnd, vals, gscale)
    if ema is None:
        torch.ops.tfd.momentum_flat(*args, guard)
    else:
        torch.ops.tfd.momentum_ema_flat(*args, ema=ema, ema_decay=ema_decay, ema_num_updates=False, guard=guard)


def _mods(variant, cuda, ema=None, gscale=1.0):
    """The trailing arguments of a variant; a clip factor of 1.0 and a guard of ok = 1 change no bit."""
    kw = {}
    if variant == "clip":
        kw["gscale"] = torch.full((1,), gscale, device=cuda)
    if variant in ("ema", "ema_guard"):
        kw["ema"] = ema
        kw["ema_decay"] = EMA_DECAY
    if variant in ("guard", "ema_guard"):
        kw["guard"] = torch.ones(1, device=cuda)
    return kw


def _banded(n, values, dt=torch.float32, band=123.0):
    """A buffer of GUARD + n + GUARD elements, the bands holding `band`, and its inner view."""
    buf = torch.full((n + 2 * GUARD,), band, device=values.device, dtype=dt)
    buf[GUARD:GUARD + n] = values.to(dt)
    return buf, buf[GUARD:GUARD + n]


def _bands_intact(buf, n, band=123.0):
    return bool((buf[:GUARD] == band).all().item() and (buf[GUARD + n:] == band).all().item())


def _grad(n, gen, cuda, gdt, scale=0.01):
    g = torch.randn(n, device=cuda, generator=gen) * scale
    g = torch.where(g.abs() < 1e-6, torch.full_like(g, 1e-6), g)  # |g| >= 1e-6: see the oracle
    return g.to(gdt)


def _adam_state(n, gen, cuda, gdt):
    """Banded p, m, v, g, pbf, ema as after some updates; {name: (buffer, inner view)}."""
    r = lambda sc: torch.randn(n, device=cuda, generator=gen) * sc  # noqa: E731
    return {"p": _banded(n, r(0.05)), "m": _banded(n, r(1e-3)),
            "v": _banded(n, torch.rand(n, device=cuda, generator=gen) * 1e-3 + 1e-4),
            "g": _banded(n, _grad(n, gen, cuda, gdt), gdt), "pbf": _banded(n, torch.zeros(n, device=cuda), torch.bfloat16),
            "ema": _banded(n, r(0.05))}


# ---------------------------------------------------------------- a. exact cases
def _exact_step(cuda, mode, lr, update):
    """t = 1 + update from t_offset alone, or from a device step of 4 + update and t_offset = -3 under a schedule
    whose rate is the case's only while s = t - 1 <= 2: a kernel that ignored t_offset would read half the rate."""
    if mode == "t_offset":
        return dict(step=None, t_offset=1 + update), None
    return (dict(step=torch.full((1,), 4 + update, dtype=torch.int64, device=cuda), t_offset=-3),
            O.PiecewiseConstant([2], [lr, lr / 2]))


@pytest.mark.parametrize("with_pbf", [False, True], ids=["no_pbf", "pbf"])
@GDTS
@pytest.mark.parametrize("mode", ["t_offset", "device_step"])
def test_exact_cases(cuda, mode, gdt, with_pbf):
    """Every quantity is a short binary fraction, so fp32 is exact whatever is contracted. Equality -- but for
    Adam's second update, whose lr_t holds sqrt(1 - 0.75^2): there m' and v' are exact and p' is held to its bound."""
    n = 4099  # float4 items of more than one block, and a scalar tail
    full = lambda x, dt=torch.float32: torch.full((n,), x, device=cuda, dtype=dt)  # noqa: E731
    pbf = full(9.0, torch.bfloat16) if with_pbf else None
    shadow_ok = lambda p: pbf is None or _same_bits(pbf, p.to(torch.bfloat16))  # noqa: E731
    # Adam: p = 1, m = v = 0, g = 1, lr = .25, beta1 = .5, beta2 = .75, eps = 0, t = 1: m' = .5, v' = .25, p' = .75;
    # then g = .5 at t = 2: m' = .5, v' = .25
    p, m, v = full(1.0), full(0.0), full(0.0)
    hyper = dict(lr=0.25, b1=0.5, b2=0.75, eps=0.0)
    kw, sched = _exact_step(cuda, mode, 0.25, 0)
    _adam(p, m, v, full(1.0, gdt), pbf, sched=sched, **hyper, **kw)
    assert torch.equal(m, full(0.5)) and torch.equal(v, full(0.25)), (m[0].item(), v[0].item())
    if not torch.equal(p, full(0.75)):  # m' and v' exact and p' not: powf(x, 1) != x
        print(f"exact Adam case: p' = {p[0].item()!r}, not 0.75 -- the device powf(x, 1) is not x; p' held to its bound")
        ref, tol = FO.adam_ref(full(1.0), full(0.0), full(0.0), full(1.0), 1, 0.25, 0.5, 0.75, 0.0)
        assert FO.check({"p": p}, {"p": ref["p"]}, tol)[0], p[0].item()
    assert shadow_ok(p)
    p0 = p.clone()
    kw, sched = _exact_step(cuda, mode, 0.25, 1)
    _adam(p, m, v, full(0.5, gdt), pbf, sched=sched, **hyper, **kw)
    assert torch.equal(m, full(0.5)) and torch.equal(v, full(0.25)), (m[0].item(), v[0].item())
    ref, tol = FO.adam_ref(p0, full(0.5), full(0.25), full(0.5), 2, 0.25, 0.5, 0.75, 0.0)
    assert FO.check({"p": p}, {"p": ref["p"]}, tol)[0] and shadow_ok(p), p[0].item()
    assert abs(p[0].item() - (p0[0].item() - 0.25 * 0.4375 ** 0.5 / 0.75)) < 1e-6
    # Momentum, weight decay .25: p = 1, mom = .5, g = .5, lr = .25, mu = .5: g + wd p = .75, mom' = 1, p' = .75
    # (Nesterov: p' = 1 - .25 (.75 + .5) = .6875); without a slot p' = 1 - .25 * .75 = .8125. The second update
    # is exact as well: its expected values come from the fp64 definition, which is exact on such fractions.
    for nesterov, slot, first in ((False, True, 0.75), (True, True, 0.6875), (False, False, 0.8125)):
        p, mom = full(1.0), full(0.5) if slot else None
        for update in (0, 1):
            kw, sched = _exact_step(cuda, mode, 0.25, update)
            want_p, want_mom = O.momentum_update(p, mom, full(0.5), 0.25, 0.5, 0.25, nesterov)
            _sgd(p, mom, full(0.5, gdt), pbf, lr=0.25, momentum=0.5, wd=0.25, nesterov=nesterov, sched=sched, **kw)
            assert torch.equal(p.double(), want_p), (nesterov, slot, update, p[0].item(), want_p[0].item())
            assert mom is None or torch.equal(mom.double(), want_mom), (nesterov, update, mom[0].item())
            assert update or (p[0].item() == first and (mom is None or mom[0].item() == 1.0))
            assert shadow_ok(p)


# ---------------------------------------------------------------- b. every size, inside its buffers
@GDTS
@SCHEDS
@pytest.mark.parametrize("variant", VARIANTS)
def test_adam_every_size_stays_inside_its_buffers(cuda, variant, sched, gdt):
    """One update at each size (the last one reaches the second grid-stride pass and the scalar tail together):
    p, m, v within bounds element by element, pbf the bf16 rounding of p', the shadow equal to ema_flat applied
    afterwards, every guard band bit for bit, and every variant bit-equal to the plain one at gscale = 1."""
    assert ADAM_SIZES[-1] == 2048 * 256 * 4 + 1027
    gen = torch.Generator(device=cuda).manual_seed(3)
    step = torch.full((1,), 2, dtype=torch.int64, device=cuda)  # t = 3
    worst = 0.0
    for n in ADAM_SIZES:
        bufs = _adam_state(n, gen, cuda, gdt)
        p, m, v, g, pbf, ema = (bufs[k][1] for k in ("p", "m", "v", "g", "pbf", "ema"))
        p0, m0, v0, e0 = p.clone(), m.clone(), v.clone(), ema.clone()
        _adam(p, m, v, g, pbf, step=step, grad_scale=0.5, sched=sched, **_mods(variant, cuda, ema))
        ref, tol = FO.adam_ref(p0, m0, v0, g, 3, _rate(sched, LR, 3), B1, B2, EPS, 0.5)
        ok, w = FO.check({"p": p, "m": m, "v": v}, ref, tol)
        assert ok, (variant, n, w)
        worst = max(worst, w)
        assert _same_bits(pbf, p.to(torch.bfloat16)), (variant, n)
        if "ema" in variant:
            torch.ops.tfd.ema_flat(e0, p, EMA_DECAY, False, step, 1)
        assert _same_bits(ema, e0), (variant, n)
        for k, (buf, _) in bufs.items():
            assert _bands_intact(buf, n), (variant, n, k)
        if variant != "plain":
            q, qm, qv, qbf = p0.clone(), m0, v0, torch.zeros_like(pbf)
            _adam(q, qm, qv, g, qbf, step=step, grad_scale=0.5, sched=sched)
            assert all(_same_bits(a, b) for a, b in ((q, p), (qm, m), (qv, v), (qbf, pbf))), (variant, n)
    print(f"flat adam {variant} {'sched' if sched else 'const'} {str(gdt).split('.')[-1]}: worst err / bound {worst:.4f}")
    assert 0 < worst <= 1


@GDTS
@SCHEDS
@pytest.mark.parametrize("variant", VARIANTS)
def test_sgd_every_size_stays_inside_its_buffers(cuda, variant, sched, gdt):
    """The same for sgd_kernel (one element per lane: the last two sizes take a second and a third grid-stride
    pass): Momentum, Nesterov and plain gradient descent, each with a weight decay."""
    assert SGD_SIZES[-2:] == [2048 * 256 + 259, 2 * 2048 * 256 + 3]
    gen = torch.Generator(device=cuda).manual_seed(4)
    step = torch.full((1,), 2, dtype=torch.int64, device=cuda)
    lr = _rate(sched, 0.01, 3)
    worst = 0.0
    for nesterov, slot in ((False, True), (True, True), (False, False)):
        for n in SGD_SIZES:
            bufs = _adam_state(n, gen, cuda, gdt)
            p, mom, g, pbf, ema = (bufs[k][1] for k in ("p", "m", "g", "pbf", "ema"))
            if not slot:
                mom = None
            p0, mom0, e0 = p.clone(), None if mom is None else mom.clone(), ema.clone()
            mods = _mods(variant, cuda, ema)
            mods.pop("ema_decay", None)
            _sgd(p, mom, g, pbf, nesterov=nesterov, step=step, grad_scale=0.5, sched=sched, **mods)
            ref, tol = FO.sgd_ref(p0, mom0, g, lr, MOM, WD, nesterov, 0.5)
            ok, w = FO.check({"p": p, "mom": mom}, ref, tol)
            assert ok, (variant, nesterov, slot, n, w)
            worst = max(worst, w)
            assert _same_bits(pbf, p.to(torch.bfloat16)), (variant, n)
            if "ema" in variant:
                torch.ops.tfd.ema_flat(e0, p, EMA_DECAY, False, step, 1)
            assert _same_bits(ema, e0), (variant, n)
            for k, (buf, _) in bufs.items():
                assert _bands_intact(buf, n), (variant, n, k)
            if variant != "plain":
                q, qbf = p0.clone(), torch.zeros_like(pbf)
                _sgd(q, mom0, g, qbf, nesterov=nesterov, step=step, grad_scale=0.5, sched=sched)
                assert _same_bits(q, p) and _same_bits(qbf, pbf) and (mom is None or _same_bits(mom0, mom)), (variant, n)
    print(f"flat sgd {variant} {'sched' if sched else 'const'} {str(gdt).split('.')[-1]}: worst err / bound {worst:.4f}")
    assert 0 < worst <= 1


# ---------------------------------------------------------------- c. the lr_t probe and steps
@pytest.mark.parametrize("beta2", [0.999, 0.99])
@pytest.mark.parametrize("sched", [None, PROBE_SCHED], ids=["const", "sched"])
def test_device_lr_t_within_e_lr(cuda, sched, beta2):
    """p = 0, m = v = g = 1, eps = 0 leave m' = v' = 1 and p' = -lr_t: the device's bias-corrected rate, bit for
    bit, against the fp64 one within E_lr -- the measurement behind K_POW (profiles/flat_optim_rel.txt)."""
    for t in FO.LR_T_PROBE_T:
        got, err, bound = FO.probe_lr_t(cuda, t, LR, B1, beta2, sched)
        print(f"lr_t probe {'sched' if sched else 'const'} beta2={beta2} t={t}: device {got!r}, rel err {err:.3e}, "
              f"E_lr {bound:.3e}, ratio {err / bound:.4f}")
        assert err <= bound, (t, got, err, bound)


def _six_updates(cuda, sched, gdt, t0, variant="clip"):
    """Six updates from m = v = 0 at t = t0 .. t0 + 5, multiplier 0.5 * 0.75; -> (worst by quantity, the last
    update's device results, inputs and bounds)."""
    n = 20003
    gen = torch.Generator(device=cuda).manual_seed(11)
    p = torch.randn(n, device=cuda, generator=gen) * 0.05
    m, v = torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    pbf = torch.zeros(n, device=cuda, dtype=torch.bfloat16)
    step = torch.full((1,), t0 - 1, dtype=torch.int64, device=cuda)
    keys, last = {}, None
    for t in range(t0, t0 + 6):
        g = _grad(n, gen, cuda, gdt)
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        _adam(p, m, v, g, pbf, step=step, grad_scale=0.5, sched=sched, gscale=torch.full((1,), 0.75, device=cuda))
        step += 1
        ref, tol = FO.adam_ref(p0, m0, v0, g, t, _rate(sched, LR, t), B1, B2, EPS, 0.5, 0.75)
        dev = {"p": p, "m": m, "v": v}
        ok, w = FO.check(dev, ref, tol, by_key=keys)
        assert ok, (t, w, keys)
        assert _same_bits(pbf, p.to(torch.bfloat16))
        last = (dev, (p0, m0, v0, g), tol, t)
    return keys, last


@GDTS
@SCHEDS
@pytest.mark.parametrize("t0", [1, 1000])
def test_six_updates_follow_fp64_and_mutations_do_not(cuda, t0, sched, gdt):
    keys, (dev, (p0, m0, v0, g), tol, t) = _six_updates(cuda, sched, gdt, t0)
    print(f"flat adam six updates from t={t0} {'sched' if sched else 'const'} {str(gdt).split('.')[-1]}: worst err / bound "
          + ", ".join(f"{k} {w:.4f}" for k, w in keys.items()))
    assert all(0 < w <= 1 for w in keys.values()) and set(keys) == {"p", "m", "v"}
    # mutations, against the last update: the same check must refuse a reference that is 2 % off (t: off by one)
    lr = _rate(sched, LR, t)
    good = dict(t=t, lr=lr, beta1=B1, beta2=B2)
    muts = [dict(lr=lr * 1.02), dict(beta1=B1 * 0.98), dict(beta2=B2 * 0.98)] + ([dict(t=t + 1), dict(t=t - 1)] if t0 == 1 else [])
    for mut in muts:
        a = {**good, **mut}
        bad, _ = FO.adam_ref(p0, m0, v0, g, a["t"], a["lr"], a["beta1"], a["beta2"], EPS, 0.5, 0.75)
        assert not FO.check(dev, bad, tol)[0], mut
        assert not FO.check({"p": dev["p"]}, {"p": bad["p"]}, tol)[0], mut  # p' alone tells as well


@GDTS
@pytest.mark.parametrize("nesterov", [False, True])
def test_six_momentum_updates_follow_fp64_and_mutations_do_not(cuda, nesterov, gdt):
    n = 20003
    gen = torch.Generator(device=cuda).manual_seed(12)
    p = torch.randn(n, device=cuda, generator=gen) * 0.05
    mom = torch.zeros(n, device=cuda)
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    keys = {}
    for t in range(1, 7):
        g = _grad(n, gen, cuda, gdt)
        p0, mom0 = p.clone(), mom.clone()
        _sgd(p, mom, g, None, nesterov=nesterov, step=step, grad_scale=0.5, sched=SCHED, gscale=torch.full((1,), 0.75, device=cuda))
        step += 1
        ref, tol = FO.sgd_ref(p0, mom0, g, _rate(SCHED, 0.0, t), MOM, WD, nesterov, 0.5, 0.75)
        dev = {"p": p, "mom": mom}
        ok, w = FO.check(dev, ref, tol, by_key=keys)
        assert ok, (t, w, keys)
    print(f"flat momentum six updates nesterov={nesterov} {str(gdt).split('.')[-1]}: worst err / bound "
          + ", ".join(f"{k} {w:.4f}" for k, w in keys.items()))
    assert all(0 < w <= 1 for w in keys.values())
    lr = _rate(SCHED, 0.0, 6)
    for kw in (dict(lr=lr * 1.02), dict(momentum=MOM * 0.98), dict(weight_decay=WD * 2), dict(nesterov=not nesterov)):
        a = {**dict(lr=lr, momentum=MOM, weight_decay=WD, nesterov=nesterov), **kw}
        bad, _ = FO.sgd_ref(p0, mom0, g, a["lr"], a["momentum"], a["weight_decay"], a["nesterov"], 0.5, 0.75)
        assert not FO.check(dev, bad, tol)[0], kw


# ---------------------------------------------------------------- d. the ranges form
RANGE_VARIANTS = [("plain", None), ("plain", SCHED), ("clip", None), ("ema", None)]


@GDTS
@pytest.mark.parametrize("name", list(FO.range_tables()))
def test_ranges_form_follows_its_table(cuda, name, gdt):
    """adam_ranges_kernel over one table, in its plain, scheduled, clip and EMA instantiations: elements inside the
    ranges within the oracle's bounds and bit-equal to adam_flat over the same elements; elements in the gaps
    and the guard bands keep their bits in p, m, v, pbf and the shadow."""
    table = FO.range_tables()[name]
    n = FO.table_extent(table) + 24  # a gap behind the last range as well
    mask = FO.range_mask(table, n, cuda)
    assert int(mask.sum().item()) == sum(k for _, k in table)
    gen = torch.Generator(device=cuda).manual_seed(5)
    step = torch.full((1,), 2, dtype=torch.int64, device=cuda)  # t = 3
    for variant, sched in RANGE_VARIANTS:
        bufs = _adam_state(n, gen, cuda, gdt)
        p, m, v, g, pbf, ema = (bufs[k][1] for k in ("p", "m", "v", "g", "pbf", "ema"))
        before = {k: bufs[k][1].clone() for k in ("p", "m", "v", "pbf", "ema")}
        mods = lambda e: _mods(variant, cuda, e, gscale=0.75)  # noqa: E731
        _adam(p, m, v, g, pbf, step=step, grad_scale=0.5, sched=sched, ranges=table, **mods(ema))
        gscale = 0.75 if variant == "clip" else 1.0
        ref, tol = FO.adam_ref(before["p"], before["m"], before["v"], g, 3, _rate(sched, LR, 3), B1, B2, EPS, 0.5, gscale)
        after = {"p": p, "m": m, "v": v, "pbf": pbf, "ema": ema}
        ok, w = FO.check(after, ref, tol, where=mask)
        assert ok and 0 < w <= 1, (name, variant, w)
        for k in after:  # the gaps
            assert _same_bits(after[k][~mask], before[k][~mask]), (name, variant, k)
        if variant != "ema":
            assert _same_bits(ema, before["ema"])
        for k, (buf, _) in bufs.items():
            assert _bands_intact(buf, n), (name, variant, k)
        flat = {k: x.clone() for k, x in before.items()}
        for beg, cnt in table:  # adam_flat over the same elements (beg % 4 == 0: the slices are aligned)
            if cnt:
                sl = slice(beg, beg + cnt)
                _adam(flat["p"][sl], flat["m"][sl], flat["v"][sl], g[sl], flat["pbf"][sl], step=step, grad_scale=0.5,
                      sched=sched, **mods(flat["ema"][sl]))
        for k in after:
            assert _same_bits(after[k], flat[k]), (name, variant, k)


def test_ranges_form_refuses_before_launching(cuda):
    n = 64
    z = lambda dt=torch.float32: torch.zeros(n, device=cuda, dtype=dt)  # noqa: E731
    p = torch.full((n,), 7.0, device=cuda)
    run = lambda table, **kw: _adam(p, z(), z(), torch.ones(n, device=cuda), None, ranges=table, **kw)  # noqa: E731
    bad = [dict(table=[(0, 8)], guard=torch.ones(1, device=cuda)),  # no guarded ranges kernel
           dict(table=[(2, 8)]), dict(table=[(0, 8), (18, 4)]),   # beg % 4
           dict(table=[(0, 6), (8, 4)]), dict(table=[(0, 4), (8, 3), (16, 4)]),  # a non-last n % 4
           dict(table=[]), dict(table=[(0, 4), (8, 4), (16, 4), (24, 4)]),  # 1..3 ranges
           dict(table=[(0, 8), (4, 8)]), dict(table=[(8, 8), (0, 4)]),  # overlapping, out of order
           dict(table=[(60, 8)]), dict(table=[(0, 68)]), dict(table=[(-4, 8)]), dict(table=[(0, -4), (8, 4)])]  # outside
    for kw in bad:
        with pytest.raises(RuntimeError):
            run(**kw)
    with pytest.raises(RuntimeError):  # one n per beg
        torch.ops.tfd.adam_ranges_flat(p, z(), z(), z(), None, [0, 8], [4], LR, B1, B2, EPS, None)
    torch.cuda.synchronize()
    assert (p == 7.0).all()
    run([(0, 8), (16, 5)])  # and a good table is taken
    assert (p[:8] != 7.0).all() and (p[8:16] == 7.0).all() and (p[16:21] != 7.0).all() and (p[21:] == 7.0).all()


# ---------------------------------------------------------------- e. the bf16 rounding
def _bf16_specials(cuda):
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even downwards, upwards, and negative
            0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,  # one ulp either side of a tie
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # the largest finite fp32 rounds to inf; the last that does not
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000,  # subnormals, the smallest normal
            0x7FC00000, 0x7F800001, 0xFFC00001, 0x7FFFFFFF]  # NaNs, one whose payload sits in the dropped bits only
    x = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32, device=cuda)
    return x.view(torch.float32)


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 5])
def test_to_bf16_rounds_as_torch_does(cuda, n):
    """tfd::to_bf16 (f2bf_bits, the rounding of every pbf) against torch's round-to-nearest-even, bit for bit; a NaN
    stays a NaN (compared by isnan, not by payload)."""
    sp = _bf16_specials(cuda)
    gen = torch.Generator(device=cuda).manual_seed(n)
    if n == 1:
        xs = [sp[i:i + 1].clone() for i in range(sp.numel())]
    else:  # every bit pattern is fair: random words, the specials at both ends (the last block's ragged end)
        x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device=cuda, generator=gen).to(torch.int32).view(torch.float32)
        k = min(sp.numel(), n // 2)
        x[:k] = sp[:k]
        x[n - k:] = sp[sp.numel() - k:]
        xs = [x]
    for x in xs:
        got, want = torch.ops.tfd.to_bf16(x), x.to(torch.bfloat16)
        assert got.dtype == torch.bfloat16 and got.shape == x.shape
        nan = torch.isnan(x)
        assert torch.equal(torch.isnan(got), nan) and torch.equal(torch.isnan(want), nan)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (n, _bits(x)[~nan][(_bits(got) != _bits(want))[~nan]][:8].tolist())


# ---------------------------------------------------------------- 4. argument checks
def test_bad_arguments_raise_before_launching(cuda):
    n = 64
    z = lambda dt=torch.float32, dev=cuda, m=n: torch.zeros(m, dtype=dt, device=dev)  # noqa: E731
    ops = torch.ops.tfd
    sentinel = lambda: torch.full((n,), 7.0, device=cuda)  # noqa: E731
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    piecewise = dict(lr_kind="piecewise", lr_params=[LR], lr_boundaries=[2], lr_values=[LR, LR / 2])

    def adam(p=None, m=None, v=None, g=None, pbf=None, step=step, **kw):
        p = sentinel() if p is None else p
        ops.adam_flat(p, z() if m is None else m, z() if v is None else v, torch.ones(n, device=cuda) if g is None else g,
                      pbf, LR, B1, B2, EPS, step, **kw)
        return p

    def momentum(p=None, mom="slot", g=None, pbf=None, ema=None, step=None, **kw):
        p = sentinel() if p is None else p
        mom = z() if isinstance(mom, str) else mom
        g = torch.ones(n, device=cuda) if g is None else g
        if ema is None:
            ops.momentum_flat(p, mom, g, pbf, LR, MOM, 0.0, False, 1.0, step, **kw)
        else:
            ops.momentum_ema_flat(p, mom, g, pbf, LR, MOM, 0.0, False, 1.0, step, ema=ema, **{"ema_decay": 0.5, **kw})
        return p

    # the baseline calls are fine
    assert (adam() != 7.0).all() and (momentum() != 7.0).all() and (momentum(ema=z()) != 7.0).all()
    assert (momentum(mom=None) != 7.0).all() and (adam(step=None) != 7.0).all()
    off1 = lambda dt=torch.float32: z(dt, m=n + 1)[1:]  # noqa: E731  a view offset by one element
    slot_bad = [z(torch.float64), z(dev="cpu"), z(torch.float16), z(m=2 * n)[::2], z(m=n + 4), z(m=n - 4)]
    g_bad = [z(torch.float64), z(torch.float16), z(dev="cpu"), z(m=2 * n)[::2], z(torch.bfloat16, m=2 * n)[::2], z(m=n + 4),
             z(m=n - 4), z(torch.bfloat16, m=n + 4)]
    pbf_bad = [z(torch.float32), z(torch.float16), z(torch.bfloat16, dev="cpu"), z(torch.bfloat16, m=2 * n)[::2],
               z(torch.bfloat16, m=n + 4), z(torch.bfloat16, m=n - 4)]
    common = [dict(step=torch.zeros(1, dtype=torch.int32, device=cuda)), dict(step=torch.zeros(1, dtype=torch.int64)),
              dict(step=torch.zeros(2, dtype=torch.int64, device=cuda)), dict(step=None, **piecewise),  # a schedule needs step
              dict(gscale=torch.ones(2, device=cuda)), dict(gscale=torch.ones(1)), dict(guard=torch.ones(2, device=cuda)),
              dict(guard=torch.ones(1))]
    bad_adam = ([dict(m=x) for x in slot_bad] + [dict(v=x) for x in slot_bad] + [dict(g=x) for x in g_bad]
                + [dict(pbf=x) for x in pbf_bad] + common
                + [dict(p=z(torch.float64)), dict(p=z(m=2 * n)[::2]), dict(p=z(m=0), m=z(m=0), v=z(m=0), g=z(m=0)),
                   dict(ema=z(m=n + 4), ema_decay=0.5), dict(ema=z(), ema_decay=1.5), dict(ema=z(torch.float64), ema_decay=0.5),
                   dict(ema=z(), ema_decay=0.5, ema_num_updates=True, step=None),
                   # 4-byte aligned only: the float4 / uint2 paths would fault or tear
                   dict(p=off1()), dict(m=off1()), dict(v=off1()), dict(g=off1()), dict(g=off1(torch.bfloat16)),
                   dict(pbf=off1(torch.bfloat16)), dict(ema=off1(), ema_decay=0.5),
                   dict(g=z(torch.bfloat16, m=n + 2)[2:])])  # 4-byte aligned bf16
    kept = []  # the sentinel-filled p of every refused call

    def refused(op, kw, **more):
        if "p" not in kw:
            kept.append(sentinel())
            kw = {"p": kept[-1], **kw}
        with pytest.raises((RuntimeError, NotImplementedError)):
            op(**kw, **more)

    for kw in bad_adam:
        refused(adam, kw)
    # an aligned view is taken: 4 elements in is 16 bytes in
    assert (adam(p=torch.full((n + 4,), 7.0, device=cuda)[4:], m=z(m=n + 4)[4:],
                 g=torch.ones(n + 4, device=cuda, dtype=torch.bfloat16)[4:]) != 7.0).all()
    bad_mom = ([dict(mom=x) for x in slot_bad] + [dict(g=x) for x in g_bad] + [dict(pbf=x) for x in pbf_bad] + common
               + [dict(p=z(torch.float64)), dict(p=z(m=2 * n)[::2]), dict(p=z(m=0), mom=None, g=z(m=0))])
    for ema in (None, z()):
        for kw in bad_mom:
            refused(momentum, kw, ema=ema)
    for kw in (dict(ema=z(m=n + 4)), dict(ema=z(), ema_decay=0.0), dict(ema=z(torch.float64)), dict(ema=z(), ema_num_updates=True)):
        refused(momentum, kw)
    # sgd_kernel reads single elements: a view offset by one element is fine for it
    assert (momentum(p=torch.full((n + 1,), 7.0, device=cuda)[1:], mom=off1(), g=torch.ones(n + 1, device=cuda)[1:],
                     pbf=off1(torch.bfloat16)) != 7.0).all()
    # nothing was launched by a refused call: every sentinel-filled p keeps its bits
    torch.cuda.synchronize()
    assert len(kept) > 100 and all(bool((x == 7.0).all().item()) for x in kept)
