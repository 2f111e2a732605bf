"""The fused one-GPU Adam step (train_step() with set_fused_tail(1): the path bench.py measures), checked
per slice against the fp64 oracle.

The step ends in one launch (mnist_adam_kernel, csrc/mnist_tail.h) that sums the conv weight-gradient
slabs itself, reads the fc-region gradient (bf16 with set_local_bf16_grads) and applies Adam; the
gradient it consumes is never stored. Starting the step from m = v = 0 leaves m' = g * (1 - beta1), one
fp32 rounding of the consumed gradient, so g is read back out of adam_m() (O.grads_from_adam_m) and goes
through the checker of tests/mnist_oracle.py with the unfused step's bounds plus the derived allowances
of O.fused_allowance. The update itself is then checked against fp64 ApplyAdam from that same gradient.
Measured values beside their bounds: profiles/mnist_fused_step_slices.txt (tools/mnist_oracle_rel.py
--fused).
"""
import numpy as np
import pytest
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.models import mnist_cnn as M

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp32"]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _checked(cuda, dtype, B, keep=1.0, local_bf16=False, step0=0, **kw):
    """One fused step at global step ``step0`` on O.random_case(B), then the oracle on what the step
    read; prints every gradient class's error and bound and returns (res, ref, classes above their
    bound). local_bf16 only exists on the bf16 step: the fp32 step takes no allowance for it."""
    res = O.run_fused_step(cuda, dtype, *O.random_case(B), keep=keep, local_bf16=local_bf16, step0=step0, **kw)
    ref = O.fused_oracle(res, dtype, keep, step0)
    bf = local_bf16 and dtype == "bf16"
    for k, (e, b, i) in sorted(O.measure_fused(res, ref, dtype, bf, only=O.GRADS).items()):
        print(f"{dtype} B={B} {k[0]} {k[1]}: {e:.3e} @ {i} (bound {b:.3e})")
    return res, ref, O.check_fused(res, ref, dtype, bf, only=O.GRADS)


def _assert_update(res, dtype):
    """v and p' against fp64 ApplyAdam from the consumed gradient (O.update_ratios), the step counter,
    the bf16 shadow, and untouched parameters where the gradient is zero."""
    r = O.update_ratios(res)
    print(f"{dtype} t={res['t']}: worst v ratio {r['v'][0]:.3f} @ {r['v'][1]}, worst p ratio {r['p'][0]:.3f} @ {r['p'][1]}")
    assert r["v"][0] <= 1.0, r
    assert r["p"][0] <= 1.0, r
    assert res["step"] == res["t"]
    if dtype == "bf16":
        assert torch.equal(_bits(res["params_bf16"]), _bits(res["p_after"].to(torch.bfloat16)))
    else:
        assert torch.equal(_bits(res["params_bf16"]), _bits(res["params_bf16_before"]))
    dead = res["m_after"] == 0
    assert int(dead.sum()) >= M.TOTAL - M.NUM_PARAMS
    assert torch.equal(_bits(res["p_after"][dead]), _bits(res["p_before"][dead]))


@pytest.mark.parametrize("dtype,B", [(d, B) for d in DTYPES for B in O.FUSED_BATCHES[d]])
def test_consumed_gradient_matches_oracle(cuda, dtype, B):
    """Feed mode, no dropout, fp32 fc gradients, at the batches on the edges of the tail's slab loops
    (O.FUSED_BATCHES says which): every gradient tensor the tail consumed, per slice."""
    _, _, bad = _checked(cuda, dtype, B)
    assert not bad, f"B={B} ({2 * B} conv1 slabs): {bad}"


@pytest.mark.parametrize("B", [5, 37, 130])
def test_consumed_gradient_with_the_benchmark_settings(cuda, B):
    """bf16, bf16 fc-region gradients, dataset mode (the next batch's gather blocks lead the tail's
    grid), dropout 0.75. The fc-region gradient the tail consumed is a bf16 number."""
    res, _, bad = _checked(cuda, "bf16", B, keep=0.75, local_bf16=True, dataset=True)
    assert not bad, bad
    g = O.grads_from_adam_m(res["m_after"], res["b1"])[M.BUCKET_SPLIT:]
    assert int((g != 0).sum()) > 1000
    assert bool(((g - g.float().to(torch.bfloat16).double()).abs() <= 2.0 ** -23 * g.abs()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_later_steps(cuda, dtype):
    """The step at global step 2 (t = 3), B = 37, dataset mode with the cursor wrapped, dropout: the
    oracle gets the parameters, the rows and the mask of step 2."""
    res, _, bad = _checked(cuda, dtype, 37, keep=0.75, dataset=True, step0=2)
    assert res["t"] == 3 and res["step"] == 3
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("variant", ["sched", "ema", "sched+ema"])
def test_tail_instantiations(cuda, variant, dtype, B):
    """The scheduled and the EMA instantiations of the tail (code objects of their own), at global step
    1 so that the exponential schedule's rate (O.FUSED_LR / 2) is not the base rate: the consumed gradient per
    slice, the update with lr_at_step's rate, and the shadow e' = e - (1 - d_t)(e - p') from the engine's
    own p' within three fp32 roundings, doubled."""
    sched = O.FUSED_SCHEDULE if "sched" in variant else None
    ema = O.FUSED_EMA if "ema" in variant else None
    res, _, bad = _checked(cuda, dtype, B, step0=1, lr=O.FUSED_LR, schedule=sched, ema=ema)
    assert not bad, bad
    assert abs(res["lr"] - (O.FUSED_LR / 2 if sched else O.FUSED_LR)) <= 2.0 ** -22 * O.FUSED_LR  # the host's fp32 evaluation
    _assert_update(res, dtype)
    if ema:
        e, p = res["ema_before"].double(), res["p_after"].double()
        omd = float(np.float32(1.0) - np.float32(res["ema_decay"]))
        assert 0.0 < omd < 1.0 and res["ema_decay"] == float(np.float32(3.0) / np.float32(12.0))
        want = e - omd * (e - p)
        tol = 2.0 ** -22 * torch.maximum(e.abs(), p.abs())
        err = (res["ema_after"].double() - want).abs()
        print(f"ema worst err / tol: {(err / tol.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= tol).all())
        assert not torch.equal(res["ema_after"], res["ema_before"])


@pytest.mark.parametrize("local_bf16", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("step0", [0, 2])
def test_update_from_consumed_gradient(cuda, dtype, local_bf16, step0):
    """B = 37, dataset mode, dropout: v and p' against fp64 ApplyAdam from the gradient the tail
    consumed, at t = 1 and t = 3.

    Bounds (derived): v within 2^-22 relative (g * g * c2: three roundings); p' within 2^-24 |p_ref| +
    2^-18 |dp_ref| -- about a dozen fp32 roundings in the two powf, lr_t, sqrtf, + eps, the divide and
    the multiply, under 2^-20 of the step, with a factor 4 over that count. Of that budget one operation
    takes most at t > 1: 1.f - powf(beta2, t) cancels three digits, so the fp32 rounding of beta2^t
    (<= 2^-25 absolute) is 2^-25 / (1 - beta2^t) of lr_t^2 -- at t = 3 a correctly rounded powf puts lr_t
    3.0e-6 (0.78 x 2^-18) from the fp64 value, for every element alike. The worst measured ratios are in
    profiles/mnist_fused_step_slices.txt."""
    res, _, bad = _checked(cuda, dtype, 37, keep=0.75, local_bf16=local_bf16, dataset=True, step0=step0)
    assert not bad, bad
    _assert_update(res, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_feed_and_dataset_steps_agree(cuda, dtype):
    """B = 37: a dataset-mode step and a feed-mode step on the same rows leave bit-identical p, m, v --
    the gather blocks in front of the tail's grid shift nothing."""
    params, x, y = O.random_case(37)
    a = O.run_fused_step(cuda, dtype, params, x, y, keep=0.75, dataset=True)
    b = O.run_fused_step(cuda, dtype, params, x, y, keep=0.75, dataset=False)
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["y"], b["y"])
    for k in ("p_after", "m_after", "v_after", "params_bf16"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert a["step"] == b["step"] == 1


def test_captured_fused_steps_with_bf16_fc_gradients(cuda):
    """B = 37 over a dataset of 100 rows, dropout, set_local_bf16_grads(1): a 2-step graph replayed
    twice == 4 eager steps, bit for bit (parameters, both Adam slots, the bf16 shadow, the step)."""
    g = torch.Generator().manual_seed(5)
    data, labels = torch.rand(100, 784, generator=g), torch.randint(0, 10, (100,), generator=g, dtype=torch.int32)
    perm = torch.randperm(100, generator=g).to(torch.int32)
    p0 = M.flat_from_dict(M.init_params(2)) * 0.05
    engs = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            e = torch.classes.tfd.MnistEngine(37, cuda.index or 0, 0.75, 1234, 0)
            e.set_adam(0.01, 0.9, 0.999, 1e-8)
            e.set_fused_tail(1)
            e.set_local_bf16_grads(1)
            e.params().copy_(p0.to(cuda))
            e.sync_shadow()
            e.set_dataset(data.to(cuda), labels.to(cuda), perm.to(cuda))
            e.set_input_mode(1)
            engs.append(e)
        a, b = engs
        a.capture_train_steps("g", 2)
        a.replay("g", 2)
        for _ in range(4):
            b.train_step()
    torch.cuda.synchronize()
    assert int(a.step_tensor().item()) == int(b.step_tensor().item()) == 4
    for get in ("params", "adam_m", "adam_v", "params_bf16"):
        assert torch.equal(_bits(getattr(a, get)()), _bits(getattr(b, get)())), get
    assert not torch.equal(a.params().cpu(), p0)
