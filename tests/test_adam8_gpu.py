"""8-bit Adam on the device (csrc/optim_q8.h, csrc/kernels/optim_q8.hip; tfd::adam8_flat / q8_encode / q8_decode,
MnistEngine.set_adam8): the codec against torch's float8 dtypes, the update on exact operands, random operands at every
size at which the kernel takes another path against flat_optim_oracle's fp64 Adam, the variants, the engine's step.

The bounds of the random cases. d is flat_optim_oracle's bound of m' (or v') from the kernel's own roundings.
  absmax:  max is monotone, so |absmax - A| <= max over the block of d =: dA.
  decode:  the device normalises x_dev = x +- d by inv = T / absmax (the division rounds once, the product once:
           2 U), converts -- at most half a code spacing off at that magnitude -- and decodes with one product
           (U); the scale absmax 2^-k is exact. So |decode - x| <= half spacing * (A + dA) / T + d + 4 U |x|, the
           spacing taken at y_hi = |x| T / A (1 + dA / A) + (d + 4 U |x|) T / A, the largest normalised magnitude
           the device can have seen (the wider binade next to an edge). A v' > 0 below the smallest code takes code
           1: there the allowance is one whole smallest code.
"""
import numpy as np
import pytest
import torch

import flat_optim_oracle as FO
from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O

pytestmark = pytest.mark.gpu

U = FO.U
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8
GUARD = 16  # guard-band elements on either side: the inner view keeps every alignment the launcher asks for
# kind -> (torch dtype, T, mantissa bits, exponent of the smallest normal)
FMT = {"m": (torch.float8_e4m3fn, 256.0, 3, -6), "v": (torch.float8_e5m2, 32768.0, 2, -14)}
ops = torch.ops.tfd


def _apply(p, st, g, pbf=None, lr=LR, b1=B1, b2=B2, eps=EPS, **kw):
    ops.adam8_flat(p, st["m8"], st["v8"], st["am"], st["av"], g, pbf, lr, b1, b2, eps, **kw)


def _encoded(m, v):
    (m8, am), (v8, av) = ops.q8_encode(m, "m"), ops.q8_encode(v, "v")
    return {"m8": m8, "v8": v8, "am": am, "av": av}


def _decoded(st):
    return ops.q8_decode(st["m8"], st["am"], "m"), ops.q8_decode(st["v8"], st["av"], "v")


@pytest.mark.parametrize("kind", ["m", "v"])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1023])
def test_codec_matches_torch_float8(cuda, kind, n):
    dt, T, _, _ = FMT[kind]
    val = torch.arange(256, dtype=torch.uint8).view(dt).float()
    ok = torch.isfinite(val) & (val.abs() <= T) & ((val >= 0) | (kind == "m"))
    ok[128] = False  # -0 is not a value of a moment
    codes = torch.arange(256)[ok]
    # exactly representable values, midpoints of neighbouring codes (to the even one), a quarter of the smallest code
    pos = codes[(codes < 127) & ok[(codes + 1) % 256]]
    x = torch.cat([val[codes], (val[pos] + val[pos + 1]) / 2, val[1:2] / 4])
    want = torch.cat([codes, pos + (pos & 1), torch.zeros(1, dtype=torch.long)])
    if kind == "v":  # a positive value never takes code 0
        want[(x > 0) & (want == 0)] = 1
    A = 0.5  # the block's maximum: a power of two, so inv = T / A and x inv are exact
    pick = (torch.arange(n) * 7) % x.numel()
    x, want = x[pick] * (A / T), want[pick].to(torch.uint8)
    x[::256], want[::256] = A, int(torch.tensor(T).to(dt).view(torch.uint8))
    got, absmax = ops.q8_encode(x.to(cuda), kind)
    assert torch.equal(got.cpu(), want) and bool((absmax == A).all()) and absmax.numel() == O.q8_blocks(n)
    ref = O.q8_encode(x.numpy(), kind)
    assert np.array_equal(got.cpu().numpy(), ref[0]) and np.array_equal(absmax.cpu().numpy(), ref[1])
    assert bool((ops.q8_decode(got, absmax, kind)[::256] == A).all())  # the maximum decodes to itself
    z, za = ops.q8_encode(torch.zeros(n, device=cuda), kind)
    assert not z.any() and not za.any()
    # tiny blocks that also hold zeros (T / max overflows from 2^-120 down): finite, the definition's, zero below 2^-90
    for top in (2.0 ** -90, 2.0 ** -91, 1e-36, 2.0 ** -120):
        t = torch.zeros(n)
        t[::3], t[::256] = top / 4, top
        (tc, ta), ref = ops.q8_encode(t.to(cuda), kind), O.q8_encode(t.numpy(), kind)
        assert np.array_equal(tc.cpu().numpy(), ref[0]) and np.array_equal(ta.cpu().numpy(), ref[1])
        assert bool(torch.isfinite(ops.q8_decode(tc, ta, kind)).all()) and bool((ta == (top if top >= 2.0 ** -90 else 0)).all())
        assert top >= 2.0 ** -90 or not tc.any()
    # codes 0 .. n - 1, all 256 from n = 256 up (e4m3's NaN codes left out), times a scale, bit for bit
    every = (torch.arange(n) % 256).to(torch.uint8)
    if kind == "m":
        every[(every & 127) == 127] = 0
    scale = torch.linspace(0.3, 1.7, O.q8_blocks(n))
    dec = ops.q8_decode(every.to(cuda), scale.to(cuda), kind).cpu()
    ref = torch.from_numpy(O.q8_decode(every.numpy(), scale.numpy(), kind))
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(dec), nan) and torch.equal(dec[~nan].view(torch.int32), ref[~nan].view(torch.int32))


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_update_on_exact_operands_equals_the_definition(cuda, gdt):
    n, t, lr, eps = 300 + 256 * 3, 3, 0.125, 2.0 ** -10
    i = torch.arange(n)
    top = i % 7 == 0  # m = v = g = 1 there: every block's maxima stay 1
    m0 = torch.where(top, 1.0, (i % 5 - 2) * 0.25)
    v0 = torch.where(top, 1.0, (i % 3) * 0.25)
    g = torch.where(top, 1.0, (i % 2) * 0.5)
    p0 = torch.linspace(-1, 1, n)
    # the reference arithmetic is exact: fp64 m', v' are fp32 numbers whose normalised values are codes
    p_ref, (m8, am), (v8, av) = O.adam8_update(p0, m0, v0, g, t, lr, 0.5, 0.75, eps)
    _, m_ref, v_ref = O.adam_update(p0, m0, v0, g, t, lr, 0.5, 0.75, eps)
    assert np.array_equal(O.q8_decode(m8, am, "m"), m_ref.numpy()) and np.array_equal(O.q8_decode(v8, av, "v"), v_ref.numpy())
    st = _encoded(m0.to(cuda), v0.to(cuda))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(_decoded(st), (m0, v0)))
    p = p0.to(cuda)
    _apply(p, st, g.to(cuda, gdt), None, lr, 0.5, 0.75, eps, t_offset=t)
    for k, want in (("m8", m8), ("am", am), ("v8", v8), ("av", av)):
        assert np.array_equal(st[k].cpu().numpy(), want), k
    ref, tol = FO.adam_ref(p0, m0, v0, g, t, lr, 0.5, 0.75, eps)
    assert FO.check({"p": p.cpu()}, {"p": ref["p"]}, {"p": tol["p"]})[0] and torch.equal(ref["p"], p_ref)


def _banded(x, band=77):
    buf = torch.full((x.numel() + 2 * GUARD,), band, device=x.device, dtype=x.dtype)
    buf[GUARD:GUARD + x.numel()] = x
    return buf, buf[GUARD:GUARD + x.numel()]


def _state_bound(kind, x, d):
    """(A, dA, bound of |decode - x|) per the module docstring; x: fp64 m' or v', d: its fp32 slack."""
    _, T, mbits, emin = FMT[kind]
    n, nb = x.numel(), O.q8_blocks(x.numel())
    blocks = lambda y: torch.nn.functional.pad(y, (0, nb * 256 - n)).view(nb, 256)  # noqa: E731
    A, dA = blocks(x.abs()).max(1).values, blocks(d).max(1).values
    Ae, dAe = (y.repeat_interleave(256)[:n] for y in (A, dA))
    s = d + 4 * U * x.abs()
    y_hi = x.abs() * T / Ae * (1 + dAe / Ae) + s * T / Ae
    half = 0.5 * torch.exp2(torch.log2(y_hi.clamp_min(2.0 ** -40)).floor().clamp_min(emin) - mbits)
    if kind == "v":
        half = torch.where(y_hi < 2.0 ** (emin - mbits), 2 * half, half)
    return A, dA, half * (Ae + dAe) / T + s


def _check_update(before, after, g, t, lr, worst, **kw):  # against fp64 Adam from the decoded state `before`
    ref, tol = FO.adam_ref(before["p"], before["m"], before["v"], g, t, lr, B1, B2, EPS, **kw)
    dev = {"p": after["p"]}
    for kind, k in (("m", "m"), ("v", "v")):
        A, dA, bound = _state_bound(kind, ref[k], tol[k])
        ref["a" + k], tol["a" + k], dev["a" + k] = A, dA + FO.TINY, after["a" + k]
        tol[k], dev[k] = bound, after[k]
    ok, w = FO.check(dev, ref, tol, by_key=worst)
    assert ok, (t, worst)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_random_updates_at_every_size_stay_inside_bounds_and_buffers(cuda, gdt):
    """One update per size (the last above one grid pass; six chained at 1025, each from the device's own previous
    state), multiplier grad_scale * *gscale = 0.5 * 0.75. Every guard band keeps its bits."""
    gen = torch.Generator(device=cuda).manual_seed(5)
    rnd = lambda n, sc: torch.randn(n, device=cuda, generator=gen) * sc  # noqa: E731
    worst = {}
    for n in [1, 2, 255, 256, 257, 1023, 1025, int(ops.q8_grid_elems()) + 257]:
        st = _encoded(rnd(n, 1e-3), torch.rand(n, device=cuda, generator=gen) * 1e-5 + 1e-7)
        g = (rnd(n, 0.01).abs().clamp_min(1e-6) * torch.sign(rnd(n, 1.0))).to(gdt)
        bufs = {"p": _banded(rnd(n, 0.05)), "g": _banded(g), "pbf": _banded(torch.zeros(n, device=cuda, dtype=torch.bfloat16)),
                "ema": _banded(rnd(n, 0.05)), **{k: _banded(v) for k, v in st.items()}}
        st = {k: bufs[k][1] for k in st}
        p, pbf, ema = bufs["p"][1], bufs["pbf"][1], bufs["ema"][1]
        step = torch.zeros(1, dtype=torch.int64, device=cuda)
        for t in range(1, 7 if n == 1025 else 2):
            m0, v0 = _decoded(st)
            before, e0 = {"p": p.clone(), "m": m0, "v": v0}, ema.clone()
            _apply(p, st, bufs["g"][1], pbf, step=step, t_offset=1, grad_scale=0.5, gscale=torch.tensor([0.75], device=cuda),
                   ema=ema, ema_decay=0.75)
            step += 1
            m1, v1 = _decoded(st)
            _check_update(before, {"p": p, "m": m1, "v": v1, "am": st["am"], "av": st["av"]}, bufs["g"][1], t, LR, worst,
                          grad_scale=0.5, gscale=0.75)
            assert torch.equal(pbf, p.to(torch.bfloat16)), n
            ops.ema_flat(e0, p, 0.75)
            assert torch.equal(ema, e0), n
            assert bool((v1 > 0).all()), n  # the code-1 floor: no parameter divides by 0 + eps
        for k, (buf, inner) in bufs.items():
            assert bool((buf[:GUARD] == 77).all() and (buf[GUARD + n:] == 77).all()), (n, k)
    print(f"adam8 flat {str(gdt).split('.')[-1]}: worst err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert 0 < max(worst.values()) <= 1


def test_clip_guard_ema_and_schedule_variants(cuda):
    n = 600  # two whole blocks and a ragged one

    def run(**kw):
        gen = torch.Generator(device=cuda).manual_seed(9)
        p, g = (torch.randn(n, device=cuda, generator=gen) * s for s in (0.05, 0.01))
        st = _encoded(torch.randn(n, device=cuda, generator=gen) * 1e-3, torch.rand(n, device=cuda, generator=gen) * 1e-5)
        out = {"p": p, "pbf": torch.full((n,), 3.0, device=cuda, dtype=torch.bfloat16), **st}
        start = {k: v.clone() for k, v in out.items()}
        _apply(p, st, g, out["pbf"], **kw)
        return out, start

    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)  # noqa: E731
    plain, start = run()
    assert not same(plain, start)
    assert same(run(gscale=torch.ones(1, device=cuda))[0], plain)  # a clip factor of exactly 1
    ema = torch.full((n,), 7.0, device=cuda)
    skipped, _ = run(guard=torch.tensor([float("inf"), 0.0, 0.0], device=cuda), ema=ema, ema_decay=0.5)
    assert same(skipped, start) and bool((ema == 7.0).all())  # ok = 0 stores nothing
    ema, want = start["p"] + 0.01, start["p"] + 0.01
    got, _ = run(ema=ema, ema_decay=0.9)
    ops.ema_flat(want, got["p"], 0.9)
    assert same(got, plain) and torch.equal(ema, want)
    # a schedule read at s = t - 1 = 1 from a device step of 5 and t_offset = -3: the constant launch at that rate and t
    sched = dict(step=torch.full((1,), 5, dtype=torch.int64, device=cuda), t_offset=-3, lr_kind="piecewise", lr_params=[LR],
                 lr_boundaries=[0], lr_values=[LR, LR / 4])
    assert same(run(**sched)[0], run(lr=LR / 4, t_offset=2)[0]) and not same(run(t_offset=2)[0], run(lr=LR / 4, t_offset=2)[0])
    # a block that decays under a zero gradient becomes the zero block
    m = torch.zeros(300, device=cuda)
    m[5], m[7], m[290] = 2.0 ** -90, 2.0 ** -93, 1.0  # block 0: its maxima fall below 2^-90 in this update
    st, p = _encoded(m, m.clone()), torch.full((300,), 0.05, device=cuda)
    _apply(p, st, torch.zeros(300, device=cuda))
    assert not st["m8"][:256].any() and not st["v8"][:256].any() and st["am"][0] == 0 and st["av"][0] == 0
    assert bool((p[:256] == 0.05).all()) and all(bool(torch.isfinite(x).all()) for x in (p, *_decoded(st)))
    assert 0.89 < float(st["am"][1]) < 0.91 and float(st["av"][1]) > 0.99  # the ordinary block beside it


def _engine(cuda, dtype, batch=5):
    e = torch.classes.tfd.MnistEngine(batch, 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    e.set_adam8(LR, B1, B2, EPS)
    e.params().copy_(M.flat_from_dict(M.init_params(13)).to(cuda) * 0.05)
    e.sync_shadow()
    g = torch.Generator().manual_seed(3)
    e.feed_x().copy_(torch.rand(batch, 784, generator=g).to(cuda))
    e.feed_y().copy_(torch.randint(0, 10, (batch,), generator=g, dtype=torch.int32).to(cuda))
    return e


@pytest.mark.parametrize("dtype,mode", [("bf16", "eager"), ("bf16", "graph1"), ("bf16", "graph3"), ("fp32", "graph3")])
def test_engine_steps_equal_the_flat_op_on_its_own_gradients(cuda, dtype, mode):
    names = ("m8", "v8", "am", "av")
    with torch.cuda.stream(torch.cuda.Stream()):
        e, twin = _engine(cuda, dtype), _engine(cuda, dtype)
        p = twin.params().clone()
        st = {k: v.clone() for k, v in zip(names, twin.adam8_state())}
        for _ in range(3):  # the op, in sequence, on the gradients of an engine stepped eagerly beside it
            twin.train_step()
            _apply(p, st, twin.grads(), None, step=twin.step_tensor(), t_offset=0)
        if mode == "eager":
            for _ in range(3):
                e.train_step()
        else:
            k = int(mode[-1])
            e.capture_train_steps("g", k)
            e.replay("g", 3 // k)
        got = dict(zip(names, e.adam8_state()))
        torch.cuda.synchronize()
        assert torch.equal(e.params(), p) and int(e.step_tensor().item()) == 3
        assert all(torch.equal(got[k], st[k]) for k in names) and bool(got["m8"].any()) and bool(got["av"].any())
        assert torch.equal(e.params_bf16(), p.to(torch.bfloat16))
        assert all(torch.equal(a, b) for a, b in zip((e.adam_m(), e.adam_v()), _decoded(st)))
        e.load_adam8(e.adam_m(), e.adam_v())  # decode then encode keeps codes and scales
        assert all(torch.equal(got[k], st[k]) for k in names)


@pytest.mark.parametrize("which", ["sfb", "zero"])
def test_engine_refuses_the_sharded_schedules(cuda, which):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, "bf16", batch=8)
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, bf16=True, sfb=which == "sfb", zero=which == "zero")
        if which == "zero":
            e.set_zero(True)
        with pytest.raises(RuntimeError, match="set_adam8 conflicts with " + ("ZeRO-1" if which == "zero" else "sufficient-factor")):
            e.train_step()
        e.set_zero(False)
        e.set_fc_sfb(False)
        for _ in range(2):  # the all-reduce schedule takes it: one launch over the whole reduced gradient
            e.train_step()
        torch.cuda.synchronize()
        assert int(e.step_tensor().item()) == 2 and bool(torch.isfinite(e.params()).all()) and bool(e.adam8_state()[0].any())
    tr.check()
    tr.close()


def test_runner_broadcast_lands_in_the_state_itself(cuda):
    from tensorflow_distributed_amd.models.mnist_runner import NativeMnistRunner

    class Chief:  # a communicator whose broadcast delivers the root's value, 3, into the tensor it is given
        def broadcast(self, t, root):
            t.fill_(3)

    r = NativeMnistRunner(5, O.Adam8bitOptimizer(LR), device=cuda)
    r.comm = Chief()
    r.broadcast_from(0)
    assert all(bool((t == 3).all()) for t in r.eng.adam8_state() + r.state_tensors()) and r.global_step() == 3
