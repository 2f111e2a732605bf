"""Numerics of the native fused MNIST step (HIP kernels) against the PyTorch fp32 oracle.

The oracle is ``models.mnist_cnn.conv_net`` in fp32 (optionally rounding to bf16 exactly where
the native kernels store/consume bf16). Gradients come from torch autograd on the same params.
"""
import pytest
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu


def _engine(B, dev, keep=1.0):
    from tensorflow_distributed_amd import _native
    _native.require()
    return torch.classes.tfd.MnistEngine(B, dev.index or 0, keep, 1234, 0)


def _ref_grads(params, x, y, emulate):
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    logits = M.conv_net(x, p, 1.0, emulate_bf16=emulate)
    loss_rows = torch.nn.functional.cross_entropy(logits, y.long(), reduction="none")
    loss_rows.mean().backward()
    return logits.detach(), loss_rows.detach(), {k: v.grad for k, v in p.items()}


def _relerr(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


# Per-tensor relative-L2 bounds of the fused bf16 step against the bf16-emulating fp32 oracle: ~3x the
# worst error measured over these three configurations x 3 seeds (profiles/mnist_oracle_rel_r6.txt,
# tools/mnist_oracle_rel.py), like the ResNet bounds (profiles/resnet_oracle_rel_r5.txt). Scaling any
# one gradient by 1.02 must break them (the mutation check below).
REL_BOUND = {"loss": 3e-5, "wc1": 1.2e-2, "wc2": 9e-3, "wd1": 7.5e-3, "out": 6e-3, "bc1": 1.1e-2, "bc2": 8e-3,
             "bd1": 5.5e-3, "out_b": 2e-5}


def _oracle_errors(loss, loss_ref, g, g_ref):
    errs = {"loss": _relerr(loss, loss_ref)}
    errs.update({k: _relerr(g[k].float(), g_ref[k]) for k in g_ref})
    return {k: v for k, v in errs.items() if v > REL_BOUND[k]}


@pytest.mark.parametrize("scale,B", [(0.05, 128), (1.0, 128), (0.05, 40)])
def test_step_grads_match_oracle(cuda, scale, B):
    torch.manual_seed(0)
    params = {k: v * scale for k, v in M.init_params(7).items()}
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,), dtype=torch.int32)
    eng = _engine(B, cuda)
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
    _, loss_ref, g_ref = _ref_grads({k: v.float() for k, v in params.items()}, x, y, emulate=True)
    loss = eng.loss_rows().cpu()
    g = M.dict_from_flat(eng.grads().cpu())
    bad = _oracle_errors(loss, loss_ref, g, g_ref)
    assert not bad, bad  # bf16 rounding points emulated by the oracle
    # mutation check: a 2 % scale error in any single gradient tensor (or the loss) must fail
    for k in list(g_ref) + ["loss"]:
        gm = dict(g)
        lm = loss * 1.02 if k == "loss" else loss
        if k != "loss":
            gm[k] = g[k] * 1.02
        assert k in _oracle_errors(lm, loss_ref, gm, g_ref), f"a 1.02x {k} passes the bounds"
    # the localised check: every slice of every tensor against the fp64 oracle (tests/mnist_oracle.py)
    got = O.collect(eng)
    bad = O.check(got, O.oracle_step(params, x, y, "bf16", follow=got), "bf16")
    assert not bad, bad


def test_adam_step_and_counter(cuda):
    B = 64
    params = {k: v * 0.05 for k, v in M.init_params(3).items()}
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,), dtype=torch.int32)
    eng = _engine(B, cuda)
    eng.set_adam(0.01, 0.9, 0.999, 1e-8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(M.flat_from_dict(params).to(cuda))
        eng.sync_shadow()
        eng.feed_x().copy_(x.to(cuda))
        eng.feed_y().copy_(y.to(cuda))
        p0 = eng.params().clone()
        eng.forward(True); eng.backward_a(); eng.backward_b()
        g = eng.grads().clone()
        eng.apply_optimizer(1.0)
    torch.cuda.synchronize()
    assert int(eng.step_tensor().item()) == 1
    # TF ApplyAdam first step: p -= lr * sqrt(1-b2)/(1-b1) * m/(sqrt(v)+eps), m=(1-b1)g, v=(1-b2)g^2
    lr_t = 0.01 * (1 - 0.999) ** 0.5 / (1 - 0.9)
    m = 0.1 * g
    v = 0.001 * g * g
    ref = p0 - lr_t * m / (v.sqrt() + 1e-8)
    assert torch.allclose(eng.params(), ref, rtol=1e-5, atol=1e-6)
    assert torch.equal(eng.params_bf16(), eng.params().to(torch.bfloat16))


def test_graph_replay_matches_eager(cuda):
    B = 128
    params = M.flat_from_dict(M.init_params(11)).to(cuda)
    n = 1024
    data = torch.rand(n, 784, device=cuda)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, device=cuda)
    perm = torch.randperm(n, device=cuda).to(torch.int32)
    engs = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            e = _engine(B, cuda, keep=0.75)
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.params().copy_(params)
            e.sync_shadow()
            e.set_dataset(data, labels, perm)
            e.set_input_mode(1)
            engs.append(e)
        for _ in range(3):
            engs[0].train_step()
        engs[1].capture_train_step("g")
        engs[1].replay("g", 3)
    torch.cuda.synchronize()
    assert int(engs[0].step_tensor().item()) == 3 and int(engs[1].step_tensor().item()) == 3
    assert torch.equal(engs[0].params(), engs[1].params())


def test_training_reduces_loss(cuda):
    B = 128
    n = 4096
    torch.manual_seed(1)
    # learnable synthetic task: class templates + noise
    tmpl = torch.rand(10, 784)
    yl = torch.randint(0, 10, (n,))
    data = (0.7 * tmpl[yl] + 0.3 * torch.rand(n, 784)).to(cuda)
    labels = yl.to(torch.int32).to(cuda)
    perm = torch.randperm(n).to(torch.int32).to(cuda)
    eng = _engine(B, cuda, keep=0.75)
    eng.set_adam(0.01, 0.9, 0.999, 1e-8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(M.flat_from_dict(M.init_params(5)).to(cuda))
        eng.sync_shadow()
        eng.set_dataset(data, labels, perm)
        eng.set_input_mode(1)
        r0 = eng.evaluate(data[:1000], labels[:1000]).cpu()
        for _ in range(60):
            eng.train_step()
        r1 = eng.evaluate(data[:1000], labels[:1000]).cpu()
    torch.cuda.synchronize()
    assert r1[1] > r0[1] and r1[1] >= 800, (r0, r1)


def test_fused_adam_tail_matches_unfused(cuda):
    """One-GPU step whose Adam kernel also reduces the conv grad slabs (set_fused_tail) == the
    reduce kernel + plain Adam path, up to the slab summation order."""
    B = 128
    params = M.flat_from_dict(M.init_params(13)).to(cuda) * 0.05
    n = 1024
    data = torch.rand(n, 784, device=cuda)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, device=cuda)
    perm = torch.randperm(n, device=cuda).to(torch.int32)
    engs = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for fused in (1, 0):
            e = _engine(B, cuda, keep=0.75)
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.set_fused_tail(fused)
            e.params().copy_(params)
            e.sync_shadow()
            e.set_dataset(data, labels, perm)
            e.set_input_mode(1)
            engs.append(e)
        for e in engs:
            for _ in range(3):
                e.train_step()
    torch.cuda.synchronize()
    assert [int(e.step_tensor().item()) for e in engs] == [3, 3]
    d0 = engs[0].params() - params
    d1 = engs[1].params() - params
    assert _relerr(d0, d1) < 1e-2, _relerr(d0, d1)
    assert torch.equal(engs[0].params_bf16(), engs[0].params().to(torch.bfloat16))


def test_local_bf16_fc_grads_match_fp32(cuda):
    """One GPU, fused tail, fc-region gradients kept in bf16 (set_local_bf16_grads: fc backward
    writes bf16, Adam reads bf16) == the fp32-gradient path, up to bf16 rounding of the grads."""
    B = 128
    params = M.flat_from_dict(M.init_params(17)).to(cuda) * 0.05
    n = 1024
    data = torch.rand(n, 784, device=cuda)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, device=cuda)
    perm = torch.randperm(n, device=cuda).to(torch.int32)
    engs = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for bf in (1, 0):
            e = _engine(B, cuda, keep=0.75)
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.set_local_bf16_grads(bf)
            e.params().copy_(params)
            e.sync_shadow()
            e.set_dataset(data, labels, perm)
            e.set_input_mode(1)
            engs.append(e)
        for e in engs:
            for _ in range(3):
                e.train_step()
    torch.cuda.synchronize()
    assert [int(e.step_tensor().item()) for e in engs] == [3, 3]
    d0 = engs[0].params() - params
    d1 = engs[1].params() - params
    assert _relerr(d0, d1) < 2e-2, _relerr(d0, d1)
    fc = slice(M.BUCKET_SPLIT, None)
    assert _relerr(d0[fc], d1[fc]) < 2e-2
    assert torch.equal(engs[0].params_bf16(), engs[0].params().to(torch.bfloat16))


def _assert_same_regions(p0, p1, what):
    bad = {}
    for name, sl in (("conv1", slice(0, 832)), ("conv2", slice(832, M.BUCKET_SPLIT)),
                     ("fc1", slice(M.BUCKET_SPLIT, M.OFFSETS["out"])), ("out", slice(M.OFFSETS["out"], None))):
        d = (p0[sl] - p1[sl]).abs()
        if d.max().item() > 0:
            bad[name] = (int((d > 0).sum().item()), d.max().item())
    assert not bad, f"{what}: differing elements per region {bad}"


def test_captured_graph_steps_are_bitwise_the_eager_steps(cuda):
    """One GPU: a multi-step hipGraph replays exactly the eager step sequence (device step counter,
    dataset cursor, prefetched next batch, dropout key): parameters, slots and the step counter are
    bitwise equal after 1 + 4 + 3x4 steps either way (a missing dependency inside the captured step
    shows up as a mismatch)."""
    B = 128
    params = M.flat_from_dict(M.init_params(23)).to(cuda) * 0.05
    n = 1024
    data = torch.rand(n, 784, device=cuda)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, device=cuda)
    perm = torch.randperm(n, device=cuda).to(torch.int32)
    engs = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            e = _engine(B, cuda, keep=0.75)
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.params().copy_(params)
            e.sync_shadow()
            e.set_dataset(data, labels, perm)
            e.set_input_mode(1)
            engs.append(e)
        for e in engs:
            e.train_step()
        engs[0].capture_train_steps("g", 4)
        engs[0].replay("g", 4)
        for _ in range(16):
            engs[1].train_step()
    torch.cuda.synchronize()
    assert [int(e.step_tensor().item()) for e in engs] == [17, 17]
    _assert_same_regions(engs[0].params(), engs[1].params(), "captured vs eager")
    assert torch.equal(engs[0].adam_v(), engs[1].adam_v())
    assert torch.equal(engs[0].params_bf16(), engs[1].params_bf16())


def test_phase_timing_events_inside_graph(cuda):
    """HIP timing events at the phase boundaries, recorded eagerly and as graph event nodes."""
    B = 128
    n = 1024
    data = torch.rand(n, 784, device=cuda)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, device=cuda)
    perm = torch.randperm(n, device=cuda).to(torch.int32)
    e = _engine(B, cuda, keep=0.75)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.params().copy_(M.flat_from_dict(M.init_params(1)).to(cuda))
        e.sync_shadow()
        e.set_dataset(data, labels, perm)
        e.set_input_mode(1)
        e.set_phase_timing(True)
        e.train_step()
        eager = e.phase_times().tolist()
        e.capture_train_step("g")
        e.replay("g", 3)
        graph = e.phase_times().tolist()
    torch.cuda.synchronize()
    for ph in (eager, graph):
        fwd, bfc, bconv, opt, ar, wait, step = ph
        assert min(fwd, bfc, bconv, opt) > 0 and ar == 0 and step > 0, ph
        assert abs(fwd + bfc + bconv + opt - step) < 1e-3 * max(step, 1), ph
        assert step < 5.0, ph  # ms


def test_fused_conv12_forward_matches_oracle(cuda):
    """conv1 fused into the conv2 kernel (bf16 MFMA, p1 computed into LDS) matches the fp32 oracle
    that rounds its conv1 operands (x, W1) to bf16 the same way; so do the gradients."""
    B = 128
    params = {k: v * 0.05 for k, v in M.init_params(21).items()}
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,), dtype=torch.int32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e = _engine(B, cuda, keep=1.0)
        e.params().copy_(M.flat_from_dict(params).to(cuda))
        e.sync_shadow()
        e.feed_x().copy_(x.to(cuda))
        e.feed_y().copy_(y.to(cuda))
        e.forward(True)
        e.backward_a()
        e.backward_b()
    torch.cuda.synchronize()
    r = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    x4 = x.reshape(-1, 28, 28, 1)
    p1 = r(M.maxpool_same_nhwc(torch.relu(M.conv2d_same_nhwc(r(x4), r(params["wc1"]), params["bc1"])), 2))
    got = e.pool1().float().cpu()
    assert _relerr(got, p1) < 4e-3, _relerr(got, p1)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    logits = M.conv_net(x, p, 1.0, emulate_bf16=True, bf16_conv1=True)
    torch.nn.functional.cross_entropy(logits, y.long()).backward()
    g = M.dict_from_flat(e.grads().cpu())
    for k in p:
        assert _relerr(g[k], p[k].grad) < 3e-2, (k, _relerr(g[k], p[k].grad))


def test_device_dataset_rows_equal_host_gathered_batches(cuda):
    """Dataset mode (batch rows perm[(step*B + b) % n], prefetched for the next step by the kernel
    that bumps the step) == feeding the same host-gathered batches, bit for bit, across an epoch
    boundary and an invalidated prefetch (new permutation)."""
    B, n, steps = 64, 200, 7  # 200 / 64: wraps around the dataset
    g = torch.Generator(device=cuda).manual_seed(5)
    data = torch.rand(n, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (n,), device=cuda, generator=g, dtype=torch.int32)
    perm = torch.randperm(n, device=cuda, generator=g).to(torch.int32)
    params = M.flat_from_dict(M.init_params(2)).to(cuda) * 0.05
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a, b = _engine(B, cuda, keep=0.75), _engine(B, cuda, keep=0.75)
        for e in (a, b):
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.params().copy_(params)
            e.sync_shadow()
        a.set_dataset(data, labels, perm)
        a.set_input_mode(1)
        for i in range(steps):
            if i == 4:  # reshuffle mid-run: the prefetched rows must be dropped
                perm.copy_(torch.randperm(n, device=cuda, generator=g).to(torch.int32))
                a.invalidate_prefetch()
            a.train_step()
            idx = perm[(torch.arange(B, device=cuda) + i * B) % n].long()
            b.feed_x().copy_(data[idx])
            b.feed_y().copy_(labels[idx])
            b.train_step()
    torch.cuda.synchronize()
    assert torch.equal(a.params(), b.params())
    assert torch.equal(a.loss_rows(), b.loss_rows())

