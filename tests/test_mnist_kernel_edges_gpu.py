"""The MNIST step kernels at the batches and inputs where tile-structured kernels go wrong, checked
slice by slice against the fp64 oracle (tests/mnist_oracle.py; bounds from
profiles/mnist_oracle_slices_r7.txt): edge batches, an integer-valued step whose forward must be exact
(max-pool and argmax ties included), impulse images at the SAME-padding corners, blank and saturated
neighbours, a saturated head, evaluate() tails, captured-equals-eager at a prime batch, and the
largest batch the engine accepts.
"""
import pytest
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp32"]


def _checked(cuda, dtype, params, x, y, keep=1.0, follow=True, only=None):
    """Run the engine, then the oracle (taking the kernel's side of near ties), print every class's
    error and return (got, ref, classes above their bound)."""
    got = O.run_engine(cuda, dtype, params, x, y, keep)
    mask = M.native_dropout_mask(x.shape[0], 0, 0, 1234, keep) if keep < 1.0 else None
    ref = O.oracle_step(params, x, y, dtype, keep, mask, follow=got if follow else None)
    for k, (e, i) in sorted(O.measure(got, ref).items()):
        print(f"{dtype} {k[0]} {k[1]}: {e:.3e} @ {i} (bound {O.bound_for(k, ref, dtype):.3e})")
    return got, ref, O.check(got, ref, dtype, only=only)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,keep", [(B, 1.0) for B in O.EDGE_BATCHES] + [(37, 0.75)])
def test_edge_batches(cuda, dtype, B, keep):
    """Odd, prime and off-tile batches (O.EDGE_BATCHES says which edge each one sits on): activations,
    loss rows, predictions and every gradient, per slice."""
    _, _, bad = _checked(cuda, dtype, *O.random_case(B), keep=keep)
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [5, 37])
def test_integer_step_forward_is_exact(cuda, dtype, B):
    """Integer-valued inputs (O.integer_case): every forward value is a small integer under any
    summation order, so pool1, pool2, hidden, the predictions and both pools' argmax positions must
    EQUAL the oracle -- thousands of max-pool windows tie at positive values and a row's top two logits
    tie, which pins the first-maximum rule. Loss rows and gradients go through the checker."""
    params, x, y = O.integer_case(B)
    got, ref, bad = _checked(cuda, dtype, params, x, y, follow=False)
    for k in ("pool1", "pool2", "hidden", "logits"):
        assert bool((ref[k] == ref[k].round()).all()) and ref[k].abs().max() <= 256, k
    top = ref["logits"].topk(2, 1).values
    mx2 = ref["win2"].max(-1).values
    assert int((top[:, 0] == top[:, 1]).sum()) >= 1
    assert int((((ref["win2"] == mx2[..., None]).sum(-1) > 1) & (mx2 > 0)).sum()) >= 1
    for k in ("pool1", "pool2", "hidden", "correct_rows"):
        assert torch.equal(got[k].reshape(ref[k].shape), ref[k]), k
    for k in ("idx1", "idx2"):
        assert torch.equal(got[k].long().reshape(ref[k].shape), ref[k]), k
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [9, 37])
def test_impulse_images(cuda, dtype, B):
    """A single 1.0 pixel at each corner, edge midpoint and the centre, dense random weights: every one
    of the 25 taps meets the zero border. As a batch of their own and as the first and the last images
    of a batch of 37; pool1 and pool2 elementwise (and per image and channel)."""
    got, ref, bad = _checked(cuda, dtype, *O.impulse_case(B), only=("pool1", "pool2", "idx1", "idx2"))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("B", [6, 3])
def test_neighbours_do_not_leak(cuda, dtype, B, reverse):
    """blank, all-ones, random, blank, random, all-ones in one batch (B = 3: the first three, for the
    fp32 conv2 weight gradient's groups of 2), and reversed: per-image activations and all gradients."""
    _, _, bad = _checked(cuda, dtype, *O.neighbours_case(B, reverse))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("labels", ["zeros", "nines", "argmin"])
def test_saturated_head(cuda, dtype, labels):
    """Output layer scaled to max |logit| = 60 (inside fp32 exp's range): finite loss rows within the
    bound of the fp64 log-sum-exp, and the out / out_b gradients."""
    params, x, y = O.saturated_case(37, labels)
    got, ref, bad = _checked(cuda, dtype, params, x, y, only=("loss_rows", "out", "out_b", "correct_rows"))
    assert 55.0 <= ref["logits"].abs().max().item() <= 65.0
    assert bool(torch.isfinite(got["loss_rows"]).all())
    assert not bad, bad


def _dataset_engine(cuda, dtype, B, n, keep, seed=5):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(n, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (n,), device=cuda, generator=g, dtype=torch.int32)
    perm = torch.randperm(n, device=cuda, generator=g).to(torch.int32)
    e = torch.classes.tfd.MnistEngine(B, cuda.index or 0, keep, 1234, 0)
    e.set_dtype(dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    e.params().copy_(M.flat_from_dict(M.init_params(2)).to(cuda) * 0.05)
    e.sync_shadow()
    e.set_dataset(data, labels, perm)
    e.set_input_mode(1)
    return e, data, labels


@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluate_tails(cuda, dtype):
    """evaluate() runs the forward kernels at the tail size n % B of an engine with B = 64: n on both
    sides of the batch. Integer-valued inputs: the number correct equals the oracle exactly, the loss
    sum is within the loss rows' bound."""
    params, x, y = O.integer_case(150)
    ref = O.oracle_step(params, x, y, dtype, backward=False)
    e = torch.classes.tfd.MnistEngine(64, cuda.index or 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    out = {}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.params().copy_(M.flat_from_dict(params).to(cuda))
        e.sync_shadow()
        xd, yd = x.to(cuda), y.to(cuda)
        for n in (1, 63, 64, 65, 150):
            out[n] = e.evaluate(xd[:n].clone(), yd[:n].clone()).cpu()
    torch.cuda.synchronize()
    for n, r in out.items():
        rows = ref["loss_rows"][:n]
        tol = O.bound_for(("loss_rows", "elem"), ref, dtype) * rows.pow(2).mean().sqrt().item() * n
        print(f"{dtype} n={n}: loss sum {r[0].item():.6f} (oracle {rows.sum().item():.6f}, tol {tol:.2e}) correct {int(r[1])}")
        assert int(r[1]) == int(ref["correct_rows"][:n].sum()), n
        assert abs(r[0].item() - rows.sum().item()) <= tol + 2.0 ** -23 * rows.sum().item(), n  # + the fp32 sum's rounding


@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluate_leaves_training_state_alone(cuda, dtype):
    """Dataset mode, Adam, dropout: 3 steps, an evaluate() with a tail, 3 steps == 6 straight steps, bit
    for bit (parameters, both Adam slots, the step counter, the bf16 shadow)."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a, data, labels = _dataset_engine(cuda, dtype, 64, 200, 0.75)
        b, _, _ = _dataset_engine(cuda, dtype, 64, 200, 0.75)
        for _ in range(3):
            a.train_step()
        a.evaluate(data[:150].clone(), labels[:150].clone())
        for _ in range(3):
            a.train_step()
        for _ in range(6):
            b.train_step()
    torch.cuda.synchronize()
    assert int(a.step_tensor().item()) == int(b.step_tensor().item()) == 6
    for get in ("params", "adam_m", "adam_v", "params_bf16"):
        assert torch.equal(getattr(a, get)(), getattr(b, get)()), get


@pytest.mark.parametrize("dtype", DTYPES)
def test_captured_graph_equals_eager_at_a_prime_batch(cuda, dtype):
    """B = 37 over a dataset of 100 rows (the cursor wraps inside the run), dropout, Adam: a 4-step
    graph replayed twice == 8 eager steps, bit for bit."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a, _, _ = _dataset_engine(cuda, dtype, 37, 100, 0.75)
        b, _, _ = _dataset_engine(cuda, dtype, 37, 100, 0.75)
        a.capture_train_steps("g", 4)
        a.replay("g", 2)
        for _ in range(8):
            b.train_step()
    torch.cuda.synchronize()
    assert int(a.step_tensor().item()) == int(b.step_tensor().item()) == 8
    for get in ("params", "adam_m", "adam_v", "params_bf16"):
        assert torch.equal(getattr(a, get)(), getattr(b, get)()), get
    assert torch.equal(a.loss_rows(), b.loss_rows())


def test_constructor_refuses_more_than_max_batch(cuda):
    """The output-layer gradient blocks keep dlogits [B][10] in LDS: (10 B + 2560) floats <= 160 KiB
    gives 3840. One more is refused by the constructor (nothing is launched), with the limit named."""
    mx = int(torch.ops.tfd.mnist_max_batch())
    assert mx == 3840 == int(torch.classes.tfd.MnistEngine.max_batch())
    with pytest.raises(RuntimeError, match=str(mx)):
        torch.classes.tfd.MnistEngine(mx + 1, cuda.index or 0, 1.0, 1234, 0)
    with pytest.raises(RuntimeError, match=str(mx)):
        torch.classes.tfd.MnistEngine(0, cuda.index or 0, 1.0, 1234, 0)


@pytest.mark.slow
def test_largest_batch_runs(cuda):
    """bf16 at exactly mnist_max_batch(): the output-layer blocks use the whole 160 KiB of LDS. Loss rows
    and the out / out_b / bd1 gradients against the oracle."""
    B = int(torch.ops.tfd.mnist_max_batch())
    params, x, y = O.random_case(B)
    got = O.run_engine(cuda, "bf16", params, x, y)
    ref = O.oracle_step(params, x, y, "bf16", follow=got, conv_backward=False)
    bad = O.check(got, ref, "bf16", only=("loss_rows", "out", "out_b", "bd1"))
    assert not bad, bad
