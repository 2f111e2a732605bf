"""The step kernels take their hot pointers as leading, preloaded kernel parameters (docs/DESIGN.md
section 8c): every launch site and every captured graph node changed with the signatures, and each
kernel's prologue has a branch per input mode. Eager steps and a captured one-step graph replayed the
same number of times, from the same state, must leave every tensor a step reads and updates across
steps bit-equal -- at the smallest batches that reach the single-block (1), ragged-tile (3) and
multi-tile (33) paths, and in each input mode that takes a different prologue branch:

  feed      a fed batch: perm is null, the rows are feed_x / feed_y themselves;
  hit       dataset mode, the rows prefetched by the previous step's last kernel (tag == step);
  miss      dataset mode after invalidate_prefetch() before EVERY step: the step -> perm -> row chain.

bf16, three steps, dropout on; the fused tail on and off, the EMA tail once and the scheduled tail once.
The fused tail has one fc-region loop per gradient format: fp32 in the cases above, and bf16
(set_local_bf16_grads(1), what the default step runs: p / gbf / m / v and t requested side by side through
the preloaded pointers) in cases of its own, at each batch and in each instantiation.
"""
import pytest
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

STEPS = 3


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _state_tensors(eng, ema):
    """Everything a training step reads and updates across steps (bench.py's list), and the shadow."""
    return [eng.params(), eng.params_bf16(), eng.adam_m(), eng.adam_v(), eng.step_tensor()] + (
        [eng.ema_params()] if ema else [])


def _engine(cuda, B, mode, fused, variant, p0, data, labels, perm, gbf=False):
    e = torch.classes.tfd.MnistEngine(B, cuda.index or 0, 0.75, 1234, 0)
    e.set_dtype("bf16")
    e.set_adam(O.FUSED_LR if "sched" in variant else 0.01, 0.9, 0.999, 1e-8)
    e.set_fused_tail(1 if fused else 0)
    e.set_local_bf16_grads(1 if gbf else 0)
    if "sched" in variant:
        e.set_lr_schedule(*O.FUSED_SCHEDULE)
    e.params().copy_(p0)
    e.sync_shadow()
    if "ema" in variant:
        e.set_ema(*O.FUSED_EMA)
    if mode == "feed":
        e.feed_x().copy_(data[:B])
        e.feed_y().copy_(labels[:B])
    else:
        e.set_dataset(data, labels, perm)
        e.set_input_mode(1)
    return e


def _run(cuda, B, mode, fused, variant="", gbf=False):
    n = 2 * B + 3  # the cursor wraps inside the run
    g = torch.Generator().manual_seed(7)
    data, labels = torch.rand(n, 784, generator=g).to(cuda), torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).to(cuda)
    perm = torch.randperm(n, generator=g).to(torch.int32).to(cuda)
    p0 = (M.flat_from_dict(M.init_params(3)) * 0.05).to(cuda)
    ema = "ema" in variant
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a, b = (_engine(cuda, B, mode, fused, variant, p0, data, labels, perm, gbf) for _ in range(2))
        for e in (a, b):  # one eager step each: launch attributes set outside capture, the next rows prefetched
            e.train_step()
        a.capture_train_step("g")
        start = [t.clone() for t in _state_tensors(a, ema)]
        for _ in range(STEPS):
            if mode == "miss":
                a.invalidate_prefetch()
                b.invalidate_prefetch()
            a.replay("g", 1)
            b.train_step()
    torch.cuda.synchronize()
    sa, sb = _state_tensors(a, ema), _state_tensors(b, ema)
    assert int(a.step_tensor().item()) == int(b.step_tensor().item()) == 1 + STEPS
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert torch.equal(_bits(x), _bits(y)), f"state tensor {i} differs between graph replays and eager steps"
    assert not torch.equal(_bits(sa[0]), _bits(start[0])), "the steps moved nothing"
    assert bool(torch.isfinite(sa[0]).all())
    a.drop_graph("g")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("mode", ["feed", "hit", "miss"])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_graph_replays_equal_eager_steps(cuda, B, mode, fused):
    _run(cuda, B, mode, fused)


@pytest.mark.parametrize("variant", ["ema", "sched"])
def test_tail_instantiations(cuda, variant):
    """The EMA and the scheduled instantiations of the fused tail (code objects of their own), once each:
    dataset mode with a prefetch hit, the multi-tile batch."""
    _run(cuda, 33, "hit", True, variant)


@pytest.mark.parametrize("B", [1, 3, 33])
def test_bf16_gradient_loop_of_the_fused_tail(cuda, B):
    """The default step's tail: fc-region gradients in bf16, dataset mode with a prefetch hit."""
    _run(cuda, B, "hit", True, gbf=True)


@pytest.mark.parametrize("variant", ["ema", "sched"])
def test_bf16_gradient_loop_of_the_tail_instantiations(cuda, variant):
    _run(cuda, 33, "miss", True, variant, gbf=True)
