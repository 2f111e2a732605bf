"""The input gradient / FGSM kernel (csrc/mnist_input_grad.h, kernels/mnist_input_grad.hip): tfd::mnist_input_grad
against training/adversarial.py input_grad_from_factors (numpy fp64), and MnistEngine.input_gradient / fgsm /
set_adversarial against the op and against a feed-mode engine fed fgsm's output, bit for bit.

The element bound of the random case, from the formats (U = 2^-23 per fp32 accumulation step, as tests/conv_oracle.py
err_e takes it: the matrix core's internal adds need not round to nearest; bf16 has 8 significant bits):
    e1[q][c]  = 1600 U sum_{tap,co} |dz2| |W2|                       fp32 accumulation of dp1 over L = 1600 exact products
    ez[q][c]  = (1 + 2^-9) e1 + 2^-8 |dp1|                                    |bf16(a) - bf16(b)| <= |a - b| + 2^-9 (|a| + |b|): the
                                                                     kernel's and the reference's dz1 round different numbers
    |dx - ref| <= sum_{tap,c} ez |W1|  +  (32 + 25) U sum (|dz1| + ez) |W1|   ez carried through sum |W1|; T's 32-term and the
                                                                     gather's 25-term fp32 accumulations
both sums taken by conv1_dgrad_ref on absolute values. profiles/input_grad_rel.txt holds the measured figures.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import adversarial as A

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
EPS, ADV = 0.1, 2
# MnistEngine.input_gradient against fp64 autograd, relative L2, measured on an MI355X (profiles/input_grad_rel.txt)
REL_L2_MEASURED = 3.393e-2


def _pixels(g, B):
    """rows in [0, 1] with pixels at exactly 0 and exactly 1, so both clamps are hit"""
    x = g.random((B, 784), dtype=np.float32)
    x[:, ::7], x[:, 3::7] = 0.0, 1.0
    return x, g.integers(0, 10, B).astype(np.int32)


def _run(dev, dz2, p1, idx1, W2, W1, x, y, eps=EPS, adv_rows=ADV):
    """the op on fp64 / integer numpy operands that bf16 holds exactly; also checks the epilogue of the launch:
    xadv from the kernel's OWN dx in fp32, clean rows and labels bit for bit"""
    pbf = torch.zeros(M.TOTAL)
    pbf[:800] = torch.from_numpy(np.asarray(W1, dtype=np.float32)).reshape(-1)
    pbf[832:832 + 51200] = torch.from_numpy(np.asarray(W2, dtype=np.float32)).reshape(-1)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    dx, xadv, yadv = torch.ops.tfd.mnist_input_grad(t(dz2, torch.bfloat16), t(p1, torch.bfloat16), t(idx1, torch.uint8),
                                                    pbf.to(torch.bfloat16).to(dev), t(x, torch.float32), t(y, torch.int32),
                                                    eps, adv_rows)
    torch.cuda.synchronize()
    dx, xadv = dx.cpu().numpy(), xadv.cpu().numpy()
    assert np.array_equal(yadv.cpu().numpy(), y)
    assert np.array_equal(xadv.view(np.int32), A.fgsm_rows(x, dx, eps, adv_rows).view(np.int32))
    assert np.array_equal(xadv[adv_rows:].view(np.int32), x[adv_rows:].view(np.int32))
    return dx


def _integer_case(g, B):
    dz2 = g.integers(-2, 3, (B, 14, 14, 64)) * (g.random((B, 14, 14, 64)) < 0.1)
    return dz2, g.integers(0, 2, (B, 14, 14, 32)), g.integers(0, 4, (B, 14, 14, 32)), g.integers(-1, 2, (5, 5, 32, 64)), \
        g.integers(-2, 3, (5, 5, 1, 32))


def _assert_exact(dz2, p1, idx1, W2, W1):
    """|dp1| <= 256 (bf16 holds it: the rounding of dz1 is exact) and every partial sum below 2^24 (fp32 holds it):
    dx then has one right bit pattern"""
    absdp1 = A.conv2_dgrad_ref(np.abs(dz2), np.abs(W2))
    assert absdp1.max() <= 256 and A.conv1_dgrad_ref(absdp1, idx1, np.abs(W1)).max() < 2 ** 24


@pytest.mark.parametrize("B", [1, 3, 67])
def test_op_is_exact_on_integer_operands(cuda, B):
    g = np.random.default_rng(B)
    ops = _integer_case(g, B)
    _assert_exact(*ops)
    want = A.input_grad_from_factors(*ops)
    got = _run(cuda, *ops, *_pixels(g, B), adv_rows=min(ADV, B))
    assert np.abs(want).max() > 0 and np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("case", ["idx0", "idx1", "idx2", "idx3", "dead"])
def test_op_borders_and_masks(cuda, case):
    g = np.random.default_rng(11)
    B = 2
    dz2 = np.zeros((B, 14, 14, 64))
    for r, c in ((0, 0), (0, 13), (13, 0), (13, 13), (7, 6)):  # one impulse at each corner and at the centre
        dz2[:, r, c, g.integers(0, 64)] = 1 + g.integers(0, 2)
    _, _, _, W2, W1 = _integer_case(g, B)
    p1 = np.zeros((B, 14, 14, 32)) if case == "dead" else np.ones((B, 14, 14, 32))
    idx1 = np.full((B, 14, 14, 32), 0 if case == "dead" else int(case[3]))
    _assert_exact(dz2, p1, idx1, W2, W1)
    want = A.input_grad_from_factors(dz2, p1, idx1, W2, W1)
    got = _run(cuda, dz2, p1, idx1, W2, W1, *_pixels(g, B))
    assert (np.abs(want).max() > 0) == (case != "dead")
    assert np.array_equal(got.astype(np.float64), want)  # dead: zero everywhere


def test_op_random_bf16_operands_within_the_derived_bound(cuda):
    g = torch.Generator().manual_seed(5)
    B = 5
    rb = lambda shape, s: (torch.randn(shape, generator=g) * s).to(torch.bfloat16).double().numpy()
    dz2, W2, W1 = rb((B, 14, 14, 64), 0.01), rb((5, 5, 32, 64), 0.05), rb((5, 5, 1, 32), 0.2)
    p1 = np.maximum(rb((B, 14, 14, 32), 1.0), 0)  # about half the relus dead
    idx1 = torch.randint(0, 4, (B, 14, 14, 32), generator=g).numpy()
    live = p1 != 0
    dp1 = A.conv2_dgrad_ref(dz2, W2)
    ez = ((1 + 2.0 ** -9) * 1600 * U * A.conv2_dgrad_ref(np.abs(dz2), np.abs(W2)) + 2.0 ** -8 * np.abs(dp1)) * live
    bound = A.conv1_dgrad_ref(ez, idx1, np.abs(W1)) + 57 * U * A.conv1_dgrad_ref(np.abs(A.round_bf16(dp1)) * live + ez, idx1, np.abs(W1))
    want = A.input_grad_from_factors(dz2, p1, idx1, W2, W1)
    got = _run(cuda, dz2, p1, idx1, W2, W1, *_pixels(np.random.default_rng(5), B))
    err = np.abs(got.astype(np.float64) - want)
    print(f"input_grad random bf16 B={B}: worst |got - ref| / bound {np.max(err / bound):.3e}, worst |got - ref| {err.max():.3e}, "
          f"max |ref| {np.abs(want).max():.3e}")
    assert bound.min() > 0 and (err <= bound).all(), (err.max(), float(np.max(err / bound)))


# ---- the engine ----
SEED, RANK = 77, 3


def _engine(dev, B, dtype="bf16", fused=True):
    e = torch.classes.tfd.MnistEngine(B, dev.index or 0, 0.75, SEED, RANK)
    e.set_dtype(dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    e.set_fused_tail(int(fused))
    flat = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(13).items()})
    e.params().copy_(flat.to(torch.bfloat16).float().to(dev))  # every parameter a bf16 number: the shadow is exact
    e.sync_shadow()
    return e


def _state(e):
    torch.cuda.synchronize()
    return [t.clone().view(torch.int32) for t in (e.params(), e.adam_m(), e.adam_v())] + [e.step_tensor().clone()]


def _rows(n, seed=9):
    g = np.random.default_rng(seed)
    x, y = _pixels(g, n)
    return x, y, g.permutation(n).astype(np.int32)


@pytest.mark.parametrize("B,n", [(1, 3), (37, 50)])
def test_engine_input_gradient(cuda, B, n):
    x, y, _ = _rows(n)
    xd, yd = torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, B)
        e.feed_x().copy_(xd[:B])
        e.feed_y().copy_(yd[:B])
        e.train_step()  # slots, the counter and the loss rows hold something to keep
        e.params().copy_(e.params().to(torch.bfloat16).float())  # bf16 numbers again: what the reference is taken on
        e.sync_shadow()
        before = _state(e) + [e.loss_rows().clone(), e.correct_rows().clone()]
        dx = e.input_gradient(xd, yd)
        after = _state(e) + [e.loss_rows().clone(), e.correct_rows().clone()]
        for a, b in zip(before, after):
            assert torch.equal(a, b)
        # the last chunk's factors are still in the engine's buffers: the op on them is the same launch
        nb = n - (n - 1) // B * B
        op_dx, _, _ = torch.ops.tfd.mnist_input_grad(e.conv2_preact_grad()[:nb].contiguous(), e.pool1()[:nb].contiguous(),
                                                     e.pool1_argmax()[:nb].contiguous(), e.params_bf16(), xd[n - nb:].clone(),
                                                     yd[n - nb:].clone(), 0.0, 0)  # clones: 16-byte aligned
        torch.cuda.synchronize()
        assert torch.equal(dx[n - nb:].view(torch.int32), op_dx.view(torch.int32))
        assert e.input_gradient(xd[:0], yd[:0]).shape == (0, 784)
        params = e.params().cpu()
    got = dx.cpu().double().numpy()
    want = np.concatenate([A.input_gradient_ref(params, x[o:o + B], y[o:o + B]) for o in range(0, n, B)])
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"engine input_gradient B={B} n={n}: relative L2 error against fp64 autograd {rel:.3e}")
    assert rel <= 3 * REL_L2_MEASURED


TB, TN, STEPS = 5, 23, 3


def _train(e, mode, steps):
    if mode == "graph3":
        e.capture_train_steps("g", steps)
        e.replay("g", 1)
    elif mode == "graph1":
        e.capture_train_step("g")
        e.replay("g", steps)
    else:
        for _ in range(steps):
            e.train_step()


@pytest.mark.parametrize("mode", ["eager_unfused", "graph1", "graph3"])
def test_adversarial_steps_equal_feed_mode_on_fgsm_rows(cuda, mode):
    x, y, perm = _rows(TN)
    xd, yd, pd = (torch.from_numpy(v).to(cuda) for v in (x, y, perm))
    fused = mode != "eager_unfused"
    with torch.cuda.stream(torch.cuda.Stream()):
        fed = _engine(cuda, TB, fused=fused)
        for t in range(STEPS):
            rows = pd[(t * TB + torch.arange(TB, device=cuda)) % TN].long()
            fed.feed_x().copy_(fed.fgsm(xd[rows].contiguous(), yd[rows].contiguous(), 0.1, 3))
            fed.feed_y().copy_(yd[rows])
            fed.train_step()
        adv = _engine(cuda, TB, fused=fused)
        adv.set_dataset(xd, yd, pd)
        adv.set_input_mode(1)
        adv.set_adversarial(0.1, 3)
        assert list(adv.adversarial()) == [0.1, 3.0]
        _train(adv, mode, STEPS)
        for name, g, w in zip(("params", "m", "v", "step"), _state(adv), _state(fed)):
            assert torch.equal(g, w), (mode, name, int((g != w).sum()))
        # off again: the steps of an engine that never had it on, from the same state
        adv.set_adversarial(0.0, -1)
        plain = _engine(cuda, TB, fused=fused)
        plain.set_dataset(xd, yd, pd)
        plain.set_input_mode(1)
        for dst, src in zip((plain.params(), plain.adam_m(), plain.adam_v(), plain.step_tensor()),
                            (adv.params(), adv.adam_m(), adv.adam_v(), adv.step_tensor())):
            dst.copy_(src)
        plain.sync_shadow()
        _train(adv, mode, 2)
        _train(plain, mode, 2)
        for name, g, w in zip(("params", "m", "v", "step"), _state(adv), _state(plain)):
            assert torch.equal(g, w), (mode, "off", name)


def test_refusals(cuda):
    e = _engine(cuda, TB, dtype="fp32")
    x, y, _ = _rows(TB)
    xd, yd = torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda)
    with pytest.raises(RuntimeError, match="fp32 engine"):
        e.set_adversarial(0.1, -1)
    with pytest.raises(RuntimeError, match="fp32 engine"):
        e.input_gradient(xd, yd)
    e = _engine(cuda, TB)
    e.set_grad_accum(2)
    with pytest.raises(RuntimeError, match="accumulation"):
        e.set_adversarial(0.1, -1)
    e.set_grad_accum(1)
    e.set_adversarial(0.1, -1)
    with pytest.raises(RuntimeError, match="set_grad_accum"):
        e.set_grad_accum(2)
    g = np.random.default_rng(0)
    dz2, p1, idx1, _, _ = _integer_case(g, 2)
    good = [torch.from_numpy(dz2).to(torch.bfloat16), torch.from_numpy(p1).to(torch.bfloat16), torch.from_numpy(idx1).to(torch.uint8),
            torch.zeros(M.TOTAL, dtype=torch.bfloat16), torch.zeros(2, 784), torch.zeros(2, dtype=torch.int32)]
    good = [t.to(cuda) for t in good]
    shifted = torch.zeros(2 * 784 + 1, device=cuda)[1:].view(2, 784)  # contiguous, 4 bytes off a 16-byte boundary
    for i, bad, msg in ((4, shifted, "16-byte aligned"), (0, good[0].float(), "must be BFloat16"), (2, good[2].int(), "must be Byte")):
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.tfd.mnist_input_grad(*(good[:i] + [bad] + good[i + 1:]), 0.1, -1)
