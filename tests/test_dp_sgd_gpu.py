"""DP-SGD on the device (csrc/mnist_dp.h, kernels/mnist_dp.hip): tfd::mnist_per_example_norms against
training/dp_sgd.py per_example_sqnorms_from_factors (numpy fp64), tfd::dp_noise_flat against dp_noise_ref, and
MnistEngine.set_dp_sgd against per-example fp64 autograd (dp_sgd_gradient_ref).

The bound of the random case, from the formats (U = 2^-23 per fp32 accumulation step, as tests/test_input_grad_gpu.py
takes it; bf16 has 8 significant bits). For one element w = sum_k a_k b_k of a per-example weight gradient:
    e_w  = L U sum |a| |b|  +  sum |a| e_b        L = 224 (conv2), 896 (conv1 weight), 784 (a bias: a = 1); e_b = 0 but
                                                  for conv1, whose b is dz1: e_b = (1 + 2^-9) 1600 U sum |dz2| |W2| +
                                                  2^-8 |dp1| (the kernel's and the reference's dz1 round different numbers)
    |sq - ref| / B^2 <= sum (2 |w| + e_w) e_w  +  D U sum (|w| + e_w)^2          D = 256 bounds the depth of every sum
                                                  of squares (at most 200 in a lane, 6 shuffle steps, 3 wave adds, B^2)
and the fc columns are one or two sums of squares of exact products: relative (D + 2) U, or (2 D + 4) U for a product.
The noise bound: logf, sqrtf and sincospif are documented at 1 ulp each, so r = sqrt(-2 log u) is within (1 + 1/2) U
relative (the square root halves the logarithm's error), the sine or cosine within U, their product another U / 2:
|z - ref| <= 3 U |ref|, to first order. profiles/dp_sgd_rel.txt holds the measured figures.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import adversarial as A
from tensorflow_distributed_amd.training import dp_sgd as D

pytestmark = pytest.mark.gpu

U, DEPTH = 2.0 ** -23, 256
SEED, RANK = 77, 3
# relative L2 of dp_norms() and, per tensor, of the clipped flat gradient against fp64 autograd (which rounds nothing to
# bf16), measured on an MI355X at these B = 5 rows (profiles/dp_sgd_rel.txt: the plain bf16 step's own gradient sits at the
# same distance from that reference); the assertions take 3x
REL_NORM_MEASURED = 2.359e-3
REL_GRAD_MEASURED = dict(wc1=7.356e-2, bc1=5.503e-2, wc2=5.109e-2, bc2=4.550e-2, wd1=2.015e-2, bd1=1.975e-2, out=2.916e-3, out_b=1.092e-3)
TOL_LINEAR = 3 ** 0.5 * 2.0 ** -8  # the clipped gradient against the engine's own per-row gradients: derived where it is used
NAMES = ("x", "p1", "idx1", "dz2", "p2", "hd", "dh", "dlogits", "W2")


def _sparse(g, shape, per_row, lo=-2, hi=3):
    """integers in [lo, hi) at about per_row places of every row, zero elsewhere"""
    return g.integers(lo, hi, shape) * (g.random(shape) < per_row / np.prod(shape[1:]))


def _integer_case(g, B):
    """sparse integer factors; the densities fall with B so that sq (which carries B^2) stays below 2^24"""
    k = int(min(64, (2.0 ** 24 / B ** 2) ** 0.5 / 4))
    return dict(x=_sparse(g, (B, 784), 2 * k, 0, 2), p1=_sparse(g, (B, 14, 14, 32), 6 * k, 0, 3), idx1=g.integers(0, 4, (B, 14, 14, 32)),
                dz2=_sparse(g, (B, 14, 14, 64), k), p2=_sparse(g, (B, 3136), k), hd=_sparse(g, (B, 1024), k, 0, 3),
                dh=_sparse(g, (B, 1024), k), dlogits=g.integers(-2, 3, (B, 10)), W2=g.integers(-1, 2, (5, 5, 32, 64)))


def _run(dev, f, clip=1e30, scale=False):
    """the op on fp64 / integer numpy factors that bf16 holds exactly -> (sq, norm, c, dz2, dh, dlogits) as numpy"""
    B = f["dz2"].shape[0]
    pbf = torch.zeros(M.TOTAL)
    pbf[832:832 + 51200] = torch.from_numpy(np.asarray(f["W2"], dtype=np.float32)).reshape(-1)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    bf = torch.bfloat16
    dz2, dh, dl = t(f["dz2"], bf), t(f["dh"], bf), t(f["dlogits"], torch.float32)
    sq, norm, c = torch.ops.tfd.mnist_per_example_norms(t(f["x"], torch.float32), t(f["p1"], bf), t(f["idx1"], torch.uint8), dz2,
                                                        t(f["p2"], bf), t(f["hd"], bf), dh, dl, pbf.to(bf).to(dev), clip, scale)
    torch.cuda.synchronize()
    return [v.float().cpu().numpy() for v in (sq, norm, c, dz2, dh, dl)]


def _want_exact(f, B):
    """the reference, after asserting that it has one right bit pattern: |dp1| <= 256 (bf16 holds it) and, on absolute
    values (an upper bound of every partial sum), every sq below 2^24 (fp32 holds it)"""
    ab = {k: np.abs(v) if k != "idx1" else v for k, v in f.items()}
    assert A.conv2_dgrad_ref(ab["dz2"], ab["W2"]).max() <= 256
    assert D.per_example_sqnorms_from_factors(*[ab[k] for k in NAMES], B).max() < 2 ** 24
    return D.per_example_sqnorms_from_factors(*[f[k] for k in NAMES], B)


@pytest.mark.parametrize("B", [1, 3, 67])
def test_op_is_exact_on_integer_factors(cuda, B):
    f = _integer_case(np.random.default_rng(B), B)
    want = _want_exact(f, B)
    sq = _run(cuda, f)[0]
    assert (want.max(0) > 0).all() and np.array_equal(sq.astype(np.float64), want), np.argwhere(sq != want)[:8]


@pytest.mark.parametrize("case", ["idx0", "idx1", "idx2", "idx3", "dead"])
def test_op_borders_and_masks(cuda, case):
    g = np.random.default_rng(11)
    B = 2
    f = _integer_case(g, B)
    f["dz2"], f["p1"], x = np.zeros((B, 14, 14, 64)), np.zeros((B, 14, 14, 32)), np.zeros((B, 28, 28))
    for r, c in ((0, 0), (0, 13), (13, 0), (13, 13), (7, 6)):  # one impulse at each corner and at the centre
        f["dz2"][:, r, c, g.integers(0, 64)] = 1 + g.integers(0, 2)
        f["p1"][:, r, c, :] = 0 if case == "dead" else 1 + g.integers(0, 2)
    for r, c in ((0, 0), (0, 27), (27, 0), (27, 27), (14, 13), (1, 1), (26, 26), (1, 26), (26, 1)):
        x[:, r, c] = 1
    f["x"], f["idx1"] = x.reshape(B, 784), np.full((B, 14, 14, 32), 0 if case == "dead" else int(case[3]))
    want = _want_exact(f, B)
    sq = _run(cuda, f)[0]
    assert ((want[:, :3] > 0).all() == (case != "dead")) and (want[:, 3] > 0).all()
    assert np.array_equal(sq.astype(np.float64), want), (sq, want)


def test_op_random_bf16_factors_within_the_derived_bound(cuda):
    g = torch.Generator().manual_seed(5)
    B = 5
    rb = lambda shape, s: (torch.randn(shape, generator=g) * s).to(torch.bfloat16).double().numpy()
    f = dict(x=rb((B, 784), 0.5).clip(0, 1), p1=np.maximum(rb((B, 14, 14, 32), 1.0), 0), idx1=torch.randint(0, 4, (B, 14, 14, 32), generator=g).numpy(),
             dz2=rb((B, 14, 14, 64), 0.01), p2=np.maximum(rb((B, 3136), 1.0), 0), hd=np.maximum(rb((B, 1024), 1.0), 0), dh=rb((B, 1024), 0.01),
             dlogits=(torch.randn((B, 10), generator=g) * 0.1).float().double().numpy(), W2=rb((5, 5, 32, 64), 0.05))
    want = D.per_example_sqnorms_from_factors(*[f[k] for k in NAMES], B)
    live = f["p1"] != 0
    dp1 = A.conv2_dgrad_ref(f["dz2"], f["W2"])
    ez = D.unpool1(((1 + 2.0 ** -9) * 1600 * U * A.conv2_dgrad_ref(np.abs(f["dz2"]), np.abs(f["W2"])) + 2.0 ** -8 * np.abs(dp1)) * live, f["idx1"])
    dz1 = D.unpool1(A.round_bf16(dp1) * live, f["idx1"])
    xb = A.round_bf16(f["x"]).reshape(B, 28, 28, 1)

    def sq_err(w, e):
        return ((2 * np.abs(w) + e) * e).reshape(B, -1).sum(1) + DEPTH * U * ((np.abs(w) + e) ** 2).reshape(B, -1).sum(1)

    bound = np.zeros((B, 8))
    for col, inp, dz, e_dz, L in ((0, xb, dz1, ez, 896), (2, f["p1"], f["dz2"], 0 * f["dz2"], 224)):
        w, b = D.wgrad_ref(inp, dz)
        aw, ab = D.wgrad_ref(np.abs(inp), np.abs(dz) + e_dz)
        ew, eb = D.wgrad_ref(np.abs(inp), e_dz)
        bound[:, col], bound[:, col + 1] = sq_err(w, L * U * aw + ew), sq_err(b, 784 * U * ab + eb)
    bound[:, :4] *= B ** 2
    bound[:, 4:] = want[:, 4:] * U * np.array([2 * DEPTH + 4, DEPTH + 2, 2 * DEPTH + 4, DEPTH + 2])
    clip = float(np.median(np.sqrt(want.sum(1))))
    sq, norm, c, dz2, dh, dl = _run(cuda, f, clip, True)
    err = np.abs(sq.astype(np.float64) - want)
    print(f"per-example norms random bf16 B={B}: worst |sq - ref| / bound per column {np.max(err / bound, 0)}, worst relative "
          f"{np.max(err / want):.3e}")
    assert bound.min() > 0 and (err <= bound).all(), np.max(err / bound, 0)
    # norm and c: a few fp32 roundings from the kernel's OWN sq (7 adds, a square root, a division)
    n64 = np.sqrt(sq.astype(np.float64).sum(1))
    assert np.all(np.abs(norm - n64) <= 8 * U * n64) and np.all(np.abs(c - D.clip_factors(norm, np.float32(clip))) <= 2 * U)
    assert 0 < (c < 1).sum() < B  # both kinds of rows
    # scaled rows: the product with the kernel's OWN c, rounded once; an unclipped row keeps its bits
    cc = c.astype(np.float32)
    for got, src, shape in ((dz2, f["dz2"], (B, -1)), (dh, f["dh"], (B, -1))):
        prod = torch.from_numpy(cc[:, None] * src.reshape(shape).astype(np.float32)).to(torch.bfloat16).float().numpy()
        assert np.array_equal(got.reshape(shape), np.where(cc[:, None] == 1, src.reshape(shape).astype(np.float32), prod))
    assert np.array_equal(dl, cc[:, None] * f["dlogits"].astype(np.float32))


def _noise(dev, step, seed, amp=1.0, regions=None):
    buf = torch.zeros(M.TOTAL, device=dev)
    reg = torch.tensor(regions or [[off, off + M._numel(M.SHAPES[k])] for k, off in M.OFFSETS.items()], dtype=torch.int64)
    torch.ops.tfd.dp_noise_flat(buf, reg, amp, torch.tensor([step], dtype=torch.int64, device=dev), seed)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def test_noise_op(cuda):
    step = (1 << 32) + 7  # both counter words of the step
    z = _noise(cuda, step, SEED)
    want = D.dp_noise_ref(M.TOTAL, step, SEED)
    assert not z[M.NUM_PARAMS:].any() and np.count_nonzero(z[:M.NUM_PARAMS]) > M.NUM_PARAMS - 8
    err = np.abs(z[:M.NUM_PARAMS].astype(np.float64) - want[:M.NUM_PARAMS])
    bound = 3 * U * (1 + 2.0 ** -20) * np.abs(want[:M.NUM_PARAMS]) + 1e-37
    print(f"dp_noise: worst |z - ref| / bound {np.max(err / bound):.3e}, worst |z - ref| {err.max():.3e}, max |z| {np.abs(want).max():.3f}")
    assert (err <= bound).all(), float(np.max(err / bound))
    assert np.array_equal(z.view(np.int32), _noise(cuda, step, SEED).view(np.int32))
    for other in (_noise(cuda, step + 1, SEED), _noise(cuda, step, SEED + 1)):
        assert np.mean(other[:M.NUM_PARAMS] == z[:M.NUM_PARAMS]) < 1e-3
    # a region table with a hole: elements outside every region keep their value; the draws follow the flat index
    part = _noise(cuda, step, SEED, 1.0, [[3, 10], [64, 65]])
    keep = np.zeros(M.TOTAL, bool)
    keep[3:10], keep[64] = True, True
    assert np.array_equal(part.view(np.int32), np.where(keep, z, 0).astype(np.float32).view(np.int32))
    n, zz = M.NUM_PARAMS, z[:M.NUM_PARAMS].astype(np.float64)
    assert abs(zz.mean()) <= 5 / np.sqrt(n) and abs(zz.var() - 1) <= 5 * np.sqrt(2.0 / n)


# ---- the engine ----
TB, STEPS = 5, 3


def _engine(dev, fused, keep_prob=0.75):
    e = torch.classes.tfd.MnistEngine(TB, dev.index or 0, keep_prob, SEED, RANK)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    e.set_fused_tail(int(fused))
    flat = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(13).items()})
    e.params().copy_(flat.to(torch.bfloat16).float().to(dev))  # every parameter a bf16 number: the shadow is exact
    e.sync_shadow()
    return e


def _state(e):
    torch.cuda.synchronize()
    return [t.clone().view(torch.int32) for t in (e.params(), e.adam_m(), e.adam_v())] + [e.step_tensor().clone()]


def _rows(dev, n, seed=9):
    g = np.random.default_rng(seed)
    x, y = g.random((n, 784), dtype=np.float32), g.integers(0, 10, n).astype(np.int32)
    return x, y, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def _train(e, mode):
    if mode == "graph3":
        e.capture_train_steps("g", STEPS)
        e.replay("g", 1)
    elif mode == "graph1":
        e.capture_train_step("g")
        e.replay("g", STEPS)
    else:
        for _ in range(STEPS):
            e.train_step()


@pytest.mark.parametrize("fused", [True, False])
def test_engine_huge_bound_without_noise_is_the_plain_unfused_step(cuda, fused):
    x, y, xd, yd = _rows(cuda, 23)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(23).astype(np.int32)).to(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        for mode in ("eager", "graph1", "graph3"):
            plain, dp = _engine(cuda, False), _engine(cuda, fused)
            dp.set_dp_sgd(1e30, 0.0)
            assert list(dp.dp_sgd()) == [1e30, 0.0]
            for e in (plain, dp):
                e.set_dataset(xd, yd, perm)
                e.set_input_mode(1)
            for _ in range(STEPS):
                plain.train_step()
            _train(dp, mode)
            for name, got, want in zip(("params", "m", "v", "step"), _state(dp), _state(plain)):
                assert torch.equal(got, want), (mode, name, int((got != want).sum()))
            assert torch.equal(dp.dp_clip_factors(), torch.ones(TB, device=cuda)) and (dp.dp_norms() > 0).all()


def _one_step(dev, fused, xd, yd, clip, sigma):
    e = _engine(dev, fused, keep_prob=1.0)
    e.set_dp_sgd(clip, sigma)
    e.feed_x().copy_(xd)
    e.feed_y().copy_(yd)
    e.train_step()
    torch.cuda.synchronize()
    return e


@pytest.mark.parametrize("fused", [True, False])
def test_engine_clipped_gradient_and_noise(cuda, fused):
    x, y, xd, yd = _rows(cuda, TB)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    with torch.cuda.stream(torch.cuda.Stream()):
        params = _engine(cuda, fused).params().cpu()
        clip = float(_one_step(cuda, fused, xd, yd, 1e30, 0.0).dp_norms().median().item())
        e0 = _one_step(cuda, fused, xd, yd, clip, 0.0)
        g0, norms, c = e0.grads().cpu().numpy(), e0.dp_norms().cpu().numpy(), e0.dp_clip_factors().cpu().numpy()
        want, want_norms, want_c = D.dp_sgd_gradient_ref(params, x, y, clip)
        assert 0 < (c < 1).sum() < TB and np.array_equal(c < 1, norms > np.float32(clip))
        rn = rel(norms.astype(np.float64), want_norms)
        got_d, want_d = M.dict_from_flat(torch.from_numpy(g0).double()), M.dict_from_flat(torch.from_numpy(want))
        rels = {k: rel(got_d[k].numpy(), want_d[k].numpy()) for k in got_d}
        print(f"engine DP-SGD B={TB} fused={fused}: dp_norms relative L2 {rn:.3e}; clipped gradient per tensor " +
              " ".join(f"{k} {v:.3e}" for k, v in rels.items()))
        assert rn <= 3 * REL_NORM_MEASURED and all(rels[k] <= 3 * REL_GRAD_MEASURED[k] for k in rels), (rn, rels)
        for k in ("out", "out_b"):  # where bf16 leaves room for it, the tolerance refuses a 2 % error of one tensor
            assert rel(got_d[k].numpy(), 1.02 * want_d[k].numpy()) > 3 * REL_GRAD_MEASURED[k], k
        assert not g0[M.NUM_PARAMS:].any()
        # The 2 % refusal on EVERY tensor: against sum_i c_i G_i / B, G_i the engine's own gradient of a batch of TB copies of
        # row i at a huge bound and c the engine's own factors. Row i's forward, its 1 / B and all its bf16 rounding points are
        # those of the clipped run, so the bf16 distance to fp64 cancels. Left over: bf16(c_i dh), bf16(c_i dz2) and, for conv1,
        # the dp1 rounded behind it are rounded once more, 2^-8 relative each at worst; three independent roundings add in
        # quadrature in L2 (taking a sum's terms as uncorrelated in sign, as its rounding errors are): sqrt(3) 2^-8 = 6.8e-3.
        G = [_one_step(cuda, fused, xd[i:i + 1].expand(TB, -1), yd[i:i + 1].expand(TB), 1e30, 0.0).grads().double().cpu() for i in range(TB)]
        lin = M.dict_from_flat(sum(float(ci) * gi for ci, gi in zip(c, G)) / TB)
        rl = {k: rel(got_d[k].numpy(), lin[k].numpy()) for k in got_d}
        print(f"engine DP-SGD B={TB} fused={fused}: against sum c_i G_i / B per tensor " + " ".join(f"{k} {v:.3e}" for k, v in rl.items()))
        for k in got_d:
            assert rl[k] <= TOL_LINEAR < rel(got_d[k].numpy(), 1.02 * lin[k].numpy()), (k, rl)
        # sigma > 0: the same gradient plus amp * z, z the noise op's draws at the step the update made
        sigma = 1.1
        e1 = _one_step(cuda, fused, xd, yd, clip, sigma)
        z = _noise(cuda, int(e1.step_tensor().item()), SEED)
        g1 = e1.grads().cpu().numpy()
        amp = np.longdouble(np.float32(sigma * clip / TB))  # one fma: the exact sum rounded once (64-bit significands hold it)
        assert np.array_equal(g1.view(np.int32), (g0.astype(np.longdouble) + amp * z.astype(np.longdouble)).astype(np.float32).view(np.int32))
        assert np.array_equal(e1.dp_norms().cpu().numpy(), norms)


def test_refusals(cuda):
    e = _engine(cuda, True)
    e.set_dtype("fp32")
    with pytest.raises(RuntimeError, match="fp32 engine"):
        e.set_dp_sgd(1.0, 0.0)
    e = _engine(cuda, True)
    e.set_grad_accum(2)
    with pytest.raises(RuntimeError, match="accumulation"):
        e.set_dp_sgd(1.0, 0.0)
    e.set_grad_accum(1)
    e.set_adversarial(0.1, -1)
    with pytest.raises(RuntimeError, match="set_adversarial"):
        e.set_dp_sgd(1.0, 0.0)
    e.set_adversarial(0.0, -1)
    e.set_dp_sgd(1.0, 1.1)
    for call, msg in ((lambda: e.set_grad_accum(2), "set_dp_sgd"), (lambda: e.set_adversarial(0.1, -1), "set_dp_sgd"),
                      (lambda: e.set_dtype("fp32"), "set_dp_sgd"), (lambda: e.set_dp_sgd(0.0, 1.0), "clip bound"),
                      (lambda: e.backward_a(), "set_dp_sgd"), (lambda: e.set_dp_sgd(0.0, 0.0) or e.dp_norms(), "is off")):
        with pytest.raises(RuntimeError, match=msg):
            call()
