"""Gradient accumulation against one big batch, per parameter tensor, against the fp64 oracle.

A helper module (like tests/mnist_oracle.py), shared by tests/test_grad_accum_gpu.py and
tools/grad_accum_rel.py: K = 4 micro-batches of 32 fed rows through an accumulating MnistEngine, and the
same 128 rows through a plain engine at batch 128 (the unfused path: forward, backward_a, backward_b),
keep_prob 1.0. Both gradients -- grads() / K for the accumulating engine -- are measured in relative L2
against tests/mnist_oracle.py's fp64 step at batch 128.
"""
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

K, B = 4, 32
_ORACLE = {}


def case():
    return O.random_case(K * B, seed=2)


def oracle_grads(dtype):
    """fp64 gradients of the 128-row batch (computed once per dtype and shared)."""
    if dtype not in _ORACLE:
        params, x, y = case()
        _ORACLE[dtype] = O.oracle_step(params, x, y, dtype, keep=1.0)["grads"]
    return _ORACLE[dtype]


def _engine(dev, dtype, batch, params):
    e = torch.classes.tfd.MnistEngine(batch, dev.index or 0, 1.0, 1234, 0)
    e.set_dtype(dtype)
    e.set_momentum(0.0, 0.0, False)  # a zero rate: the step leaves the parameters alone
    e.params().copy_(M.flat_from_dict(params).to(dev))
    e.sync_shadow()
    return e


def rel_l2(flat, ref):
    got = M.dict_from_flat(flat.detach().double().cpu())
    return {k: float((got[k] - ref[k]).norm() / ref[k].norm()) for k in ref}


def micro_grads(dev, dtype):
    """The four micro-batch gradients (batch 32 each, fp32, unscaled) from a plain engine."""
    params, x, y = case()
    out = []
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(dev, dtype, B, params)
        for j in range(K):
            e.feed_x().copy_(x[j * B:(j + 1) * B].to(dev))
            e.feed_y().copy_(y[j * B:(j + 1) * B].to(dev))
            e.forward(True)
            e.backward_a()
            e.backward_b()
            out.append(e.grads().clone())
    torch.cuda.synchronize()
    return out


def accum_vs_one(dev, dtype):
    """({tensor: e_acc}, {tensor: e_one}, summed gradient of the accumulating engine)."""
    params, x, y = case()
    ref = oracle_grads(dtype)
    with torch.cuda.stream(torch.cuda.Stream()):
        one = _engine(dev, dtype, K * B, params)
        one.feed_x().copy_(x.to(dev))
        one.feed_y().copy_(y.to(dev))
        one.forward(True)
        one.backward_a()
        one.backward_b()
        acc = _engine(dev, dtype, B, params)
        acc.set_grad_accum(K)
        assert tuple(acc.feed_x().shape) == (K * B, 784)
        acc.feed_x().copy_(x.to(dev))
        acc.feed_y().copy_(y.to(dev))
        acc.train_step()
    torch.cuda.synchronize()
    assert int(acc.step_tensor().item()) == 1 and int(acc.micro_step_tensor().item()) == K
    summed = acc.grads().clone()
    return rel_l2(summed / K, ref), rel_l2(one.grads(), ref), summed
