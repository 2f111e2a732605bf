"""The bf16 MNIST step at the batches that reach each edge of the range-checked write-through stores
(csrc/wt_store.h) in the epilogues of conv12_fwd_lds, fc1_bwd and conv2_bwd_lds:

  B = 1   six wgrad and two dgrad blocks; ragged M tiles in fc1 (dX tiles with 31 dropped rows)
  B = 3   a partial image group
  B = 5   a ragged second image group
  B = 36  nine image groups (54 wgrad blocks, not a multiple of 8), a dX row tile with 4 live rows

Every batch also has the dropped rows of the last fc1 dW tile row (3137 = 49 * 64 + 1) and of the last
output-layer gradient block (1025 = 16 * 64 + 1).

One step from seeded parameters: loss rows, activations and every gradient against the fp64 oracle with
the per-slice checker of tests/mnist_oracle.py at its bounds; and the same training step (dropout,
Adam) captured and replayed once equals the eager one bit for bit.
"""
import functools

import pytest
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

BATCHES = [1, 3, 5, 36]


@functools.lru_cache(maxsize=None)
def _case(B):
    return O.random_case(B)


@pytest.mark.parametrize("B", BATCHES)
def test_step_matches_oracle_per_slice(cuda, B):
    params, x, y = _case(B)
    got = O.run_engine(cuda, "bf16", params, x, y)
    ref = O.oracle_step(params, x, y, "bf16", follow=got)
    for k, (e, i) in sorted(O.measure(got, ref).items()):
        print(f"B={B} {k[0]} {k[1]}: {e:.3e} @ {i} (bound {O.bound_for(k, ref, 'bf16'):.3e})")
    bad = O.check(got, ref, "bf16")
    assert not bad, bad


def _engine(cuda, B, params, x, y):
    e = torch.classes.tfd.MnistEngine(B, cuda.index or 0, 0.75, 1234, 0)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    e.params().copy_(M.flat_from_dict(params).to(cuda))
    e.sync_shadow()
    e.feed_x().copy_(x.to(cuda))
    e.feed_y().copy_(y.to(torch.int32).to(cuda))
    return e


@pytest.mark.parametrize("B", BATCHES)
def test_captured_step_equals_eager(cuda, B):
    params, x, y = _case(B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = _engine(cuda, B, params, x, y)
        b = _engine(cuda, B, params, x, y)
        a.train_step()  # eager (also sets every kernel's launch attributes outside capture)
        b.capture_train_step("g")
        b.replay("g", 1)
    torch.cuda.synchronize()
    assert int(a.step_tensor().item()) == int(b.step_tensor().item()) == 1
    for get in ("params", "adam_m", "adam_v", "params_bf16", "loss_rows", "grads_bf16"):
        assert torch.equal(getattr(a, get)(), getattr(b, get)()), get
    assert bool(torch.isfinite(a.params()).all()) and bool(torch.isfinite(a.loss_rows()).all())
    assert not torch.equal(a.params().cpu(), M.flat_from_dict(params)), "the step moved the parameters"
