"""Device data augmentation (csrc/mnist_augment.h, kernels/mnist_augment.hip): tfd::augment_batch against
the fp64 reference of training/augment.py, element by element, and MnistEngine.set_augment against a
feed-mode engine fed the op's output, bit for bit, in every way a step can run.

The element bound, from the formats (eps = 2^-24, pixels in [0, 1]; profiles/augment_rel.txt):
    |out - ref| <= (e_x + e_y) * max|pixel| + 4 eps        (bilinear with a zero border is 1-Lipschitz per
                                                            axis; four roundings in the interpolation)
    e_axis = (57 alpha + 352) eps + 32 * SINCOS
  57 alpha eps   the two 28-term fp32 sums of S = alpha G N G^T over |N| <= 1 and rows of G that sum to <= 1
                 (28 eps each, the first carried through the second), and the product with alpha
  352 eps        the affine arithmetic: ten roundings at magnitudes <= 32, and theta's own rounding
                 (|dy| + |dx| <= 27, 1 / s <= 1.18: a factor 32)
  32 * SINCOS    the device sincosf: SINCOS is 3 x the error measured through the op against fp64
                 (tools/augment_rel.py), the one constant no format gives
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import augment as A

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SINCOS = 3 * 1.584e-07  # 3 x profiles/augment_rel.txt "sincos"
CONFIGS = {"identity": (0, 0, 0, 0, 0), "shift": (2, 0, 0, 0, 0), "rot_scale": (0, 15, 0.15, 0, 0),
           "elastic_8_1": (0, 0, 0, 8, 1), "elastic_34_4": (0, 0, 0, 34, 4), "elastic_34_12": (0, 0, 0, 34, 12),
           "all": (2, 15, 0.15, 34, 4)}
SEED, RANK = 77, 3


def bound(cfg):
    return 2 * ((57 * cfg[3] + 352) * EPS + 32 * SINCOS) + 4 * EPS


def dataset(n, seed=5):
    """random rows in [0, 1]; then one image of impulses at the corners and the centre, one of ones"""
    g = np.random.default_rng(seed)
    x = g.random((n, 784), dtype=np.float32)
    imp = np.zeros((28, 28), np.float32)
    for r, c in ((0, 0), (0, 27), (27, 0), (27, 27), (13, 14)):
        imp[r, c] = 1.0
    x[n - 2], x[n - 1] = imp.reshape(-1), 1.0
    return x, g.integers(0, 10, n).astype(np.int32), g.permutation(n).astype(np.int32)


def _op(dev, x, y, perm, step, B, cfg):
    out = torch.ops.tfd.augment_batch(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(perm).to(dev),
                                      step, B, SEED, RANK, *[float(v) for v in cfg])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,n,step", [(1, 7, 0), (3, 7, 5), (65, 97, 2 ** 33 + 3)])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_op_matches_the_fp64_reference(cuda, name, B, n, step):
    cfg = CONFIGS[name]
    x, y, perm = dataset(n)
    got_x, got_y = _op(cuda, x, y, perm, step, B, cfg)
    ref_x, ref_y = A.augment_batch_ref(x, y, perm, step, B, SEED, RANK, A.augment_config(*cfg))
    assert np.array_equal(got_y.cpu().numpy(), ref_y)
    got = got_x.cpu().numpy()
    if name == "identity":
        rows = perm[(step * B + np.arange(B)) % n]
        assert np.array_equal(got.view(np.int32), x[rows].view(np.int32))
        return
    err = np.abs(got.astype(np.float64) - ref_x)
    print(f"{name} B={B}: worst {err.max():.3e} bound {bound(cfg):.3e}")
    assert err.max() <= bound(cfg), (np.unravel_index(err.argmax(), err.shape), err.max(), bound(cfg))


# ---- the engine: augmentation on == feed mode fed the op's output ----
EB, EN, STEPS, AUG = 5, 23, 4, CONFIGS["all"]


def _engine(dev, dtype, accum=1):
    e = torch.classes.tfd.MnistEngine(EB, dev.index or 0, 0.75, SEED, RANK)
    e.set_dtype(dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    if accum > 1:
        e.set_grad_accum(accum)
    e.params().copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(13).items()}).to(dev))
    e.sync_shadow()
    return e


def _state(e):
    torch.cuda.synchronize()
    return [t.clone().view(torch.int32) for t in (e.params(), e.adam_m(), e.adam_v())]


def _augmented(dev, dtype, mode, accum=1):
    x, y, perm = (torch.from_numpy(v).to(dev) for v in dataset(EN))
    e = _engine(dev, dtype, accum)
    e.set_dataset(x, y, perm)
    e.set_input_mode(1)
    e.set_augment(*[float(v) for v in AUG])
    assert list(e.augment()) == [float(v) for v in AUG]
    if mode == "eager":
        for _ in range(STEPS):
            e.train_step()
    elif mode == "graph1":
        e.capture_train_step("g")
        e.replay("g", STEPS)
    else:
        e.capture_train_steps("g", STEPS)
        e.replay("g", 1)
    return e


def _fed(dev, dtype, accum=1):
    x, y, perm = dataset(EN)
    e = _engine(dev, dtype, accum)
    for t in range(STEPS):
        ax, ay = _op(dev, x, y, perm, t, accum * EB, AUG)
        e.feed_x().copy_(ax)
        e.feed_y().copy_(ay)
        e.train_step()
    return e


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_steps_equal_feed_mode_on_the_ops_output(cuda, dtype):
    with torch.cuda.stream(torch.cuda.Stream()):
        want = _state(_fed(cuda, dtype))
        for mode in ("eager", "graph1", "graph4"):
            e = _augmented(cuda, dtype, mode)
            got = _state(e)
            assert int(e.step_tensor().item()) == STEPS
            for name, g, w in zip(("params", "m", "v"), got, want):
                assert torch.equal(g, w), (mode, name, int((g != w).sum()))
        # two micro-batches of B: the rows of one batch of 2 B at the same cursor
        want = _state(_fed(cuda, dtype, accum=2))
        for g, w in zip(_state(_augmented(cuda, dtype, "eager", accum=2)), want):
            assert torch.equal(g, w)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_evaluate_never_augments(cuda, dtype):
    x, y, _ = dataset(EN)
    xe, ye = torch.from_numpy(x[:7]).to(cuda), torch.from_numpy(y[:7]).to(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _augmented(cuda, dtype, "eager")
        on = e.evaluate(xe, ye, False).clone()
        e.set_augment(0.0, 0.0, 0.0, 0.0, 0.0)
        off = e.evaluate(xe, ye, False).clone()
    torch.cuda.synchronize()
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
