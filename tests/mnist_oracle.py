"""fp64 oracle of one MNIST step and a localised (per-slice) checker for the native kernels.

A helper module (like tests/dist_util.py), shared by tests/test_mnist_oracle_checker_cpu.py, the GPU
tests and tools/mnist_oracle_rel.py --slices.

The oracle (``oracle_step``) computes forward and backward by hand in fp64. In ``"bf16"`` mode it
rounds to bf16 exactly where the bf16 kernels store or consume bf16 (csrc/kernels/mnist.hip):

  forward   x and wc1 (conv1's MFMA operands), pool1, wc2, pool2, wd1; the hidden activations only
            where they are stored for the backward (the logits use the unrounded ones), biases and
            the output layer stay unrounded;
  backward  the stored hidden activations (out-layer dW operand), dh (gradient at the fc1
            pre-activation), the pooled gradient of each conv layer before it is unpooled.

Nothing passes through fp32. ``"fp32"`` mode is plain fp64. Max-pool takes the FIRST maximum of the
2x2 window in row-major order of the pre-activation values (the kernels' ``if (z > mx)`` scan) and the
prediction is the first maximal logit (numpy.argmax).

The checker (``slice_errors`` / ``check``) measures ``|got - ref|_2 / max(|ref|_2, floor)`` per slice
of each tensor, for every slicing along which a tile-structured kernel can go wrong (a tap, a
channel, a 64-row tile, one image, ...), and an elementwise ``max|got - ref| / RMS(ref)``.
``floor = RMS(ref) * sqrt(slice size) * FLOOR_FRAC`` makes the check on a dead slice (all-zero
reference) an absolute one. Bounds: one number per (dtype, tensor, slicing), 3x the worst value
measured on the kernels (profiles/mnist_oracle_slices_r7.txt).

The last section runs the fused one-GPU Adam step, whose gradient is never stored, reads the gradient it
consumed back out of Adam's m and puts it through the same checker (tests/test_mnist_fused_step_gpu.py,
tests/test_mnist_fused_step_checker_cpu.py, tools/mnist_oracle_rel.py --fused).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from tensorflow_distributed_amd.models import mnist_cnn as M

FLOOR_FRAC = 0.1
GRADS = ("wc1", "wc2", "wd1", "out", "bc1", "bc2", "bd1", "out_b")
ACTS = ("pool1", "pool2", "hidden", "loss_rows", "dlogits", "dh")


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float64)


def _conv_same(x_nhwc, w_hwio, b):
    """5x5 SAME convolution, NHWC in and out, fp64."""
    y = F.conv2d(x_nhwc.permute(0, 3, 1, 2), w_hwio.permute(3, 2, 0, 1), b, padding=2)
    return y.permute(0, 2, 3, 1)


def _windows(z):
    """[B,H,W,C] -> [B,H/2,W/2,C,4]: the 2x2 pool windows, last axis in row-major window order."""
    B, H, W, C = z.shape
    return z.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _unwindows(w):
    B, h, wd, C, _ = w.shape
    return w.reshape(B, h, wd, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * wd, C)


def _pool_first_max(z):
    """relu + 2x2 max pool of the pre-activations z; argmax = first maximum in window order."""
    win = _windows(z)
    idx = torch.from_numpy(win.numpy().argmax(-1))
    mx = win.gather(-1, idx[..., None])[..., 0]
    return torch.relu(mx), idx, win


def _unpool(g, idx):
    w = torch.zeros(*g.shape, 4, dtype=g.dtype)
    w.scatter_(-1, idx[..., None], g[..., None])
    return _unwindows(w)


def _conv_grads(x_nhwc, w_hwio, dz, need_dx):
    x = x_nhwc.detach().clone().requires_grad_(need_dx)
    w = w_hwio.detach().clone().requires_grad_(True)
    y = _conv_same(x, w, None)
    gs = torch.autograd.grad(y, [w, x] if need_dx else [w], dz)
    return gs[0], (gs[1] if need_dx else None)


# The backward is discontinuous in three kinds of forward decision: which window element a pool routes
# its gradient to, and whether a relu (conv or fc1) passes it. Where the oracle's own margin for such a
# decision is below the forward error of the format -- a pool window whose top two values, or a relu
# input whose distance from zero, are within KINK_TOL x RMS of that activation -- either choice is a
# correct result, and a kernel that chose the other one differs from the oracle by a whole gradient
# entry (measured: fp32, B = 128, seed 1 has one fc1 unit at |pre| = 5.9e-7 RMS; its flipped mask is a
# 0.26 RMS error in one wd1 element, against 8e-6 for every other configuration). With ``follow`` (a
# kernel result) the oracle takes the kernel's decision in exactly those places and its own everywhere
# else. The tolerances sit above the measured forward errors (fp32: elementwise <= 5.4e-6 RMS;
# bf16: per-unit relative L2 <= 7e-3) and far below the spacing of ordinary decisions.
KINK_TOL = {"bf16": 2.0 ** -7, "fp32": 2.0 ** -17}


def _rms(t):
    return max(t.pow(2).mean().sqrt().item(), 1e-300)


def _follow_idx(idx, win, got_idx, tol):
    gi = torch.as_tensor(got_idx).long().reshape(idx.shape).clamp(0, 3)
    regret = win.max(-1).values - win.gather(-1, gi[..., None])[..., 0]
    return torch.where(regret <= tol, gi, idx)


def oracle_step(params, x, y, dtype="bf16", keep=1.0, mask=None, backward=True, follow=None, conv_backward=True):
    """One step in fp64. params: dict of tensors (reference shapes), x [B,784], y [B] ints.
    dtype "bf16" rounds where the bf16 kernels do (module docstring), "fp32" is plain fp64.
    mask: the 0/1 dropout mask [B,1024] (M.native_dropout_mask) when keep < 1.
    follow: a kernel result (run_engine) whose pool-argmax / relu decisions the backward takes where
    the oracle's own are within KINK_TOL of a tie (see above); the forward values are never affected.
    conv_backward=False stops after the fc-layer gradients (out, out_b, wd1, bd1).
    Returns a dict: pool1 [B,14,14,32], pool2 [B,3136] (pixel-major, channel minor), hidden (after
    relu and dropout, as stored), logits, loss_rows, correct_rows, idx1 / idx2 (argmax positions 0..3),
    win1 / win2 (the pre-activation pool windows, for argmax_regret), dlogits, dh, grads{...}."""
    assert dtype in ("bf16", "fp32")
    r = _bf if dtype == "bf16" else (lambda t: t)
    p = {k: v.detach().to(torch.float64) for k, v in params.items()}
    B = x.shape[0]
    x4 = r(x.detach().to(torch.float64).reshape(B, 28, 28, 1))
    w1, w2, wd1 = r(p["wc1"]), r(p["wc2"]), r(p["wd1"])
    p1, idx1, win1 = _pool_first_max(_conv_same(x4, w1, p["bc1"]))
    p1 = r(p1)
    p2, idx2, win2 = _pool_first_max(_conv_same(p1, w2, p["bc2"]))
    p2 = r(p2)
    p2f = p2.reshape(B, M.FEAT)
    pre = p2f @ wd1 + p["bd1"]
    scale = torch.ones_like(pre) if (keep >= 1.0 or mask is None) else mask.to(torch.float64) / keep
    h = torch.relu(pre) * scale
    logits = h @ p["out"] + p["out_b"]
    lab = torch.as_tensor(y).long()
    lse = torch.logsumexp(logits, 1)
    loss_rows = lse - logits.gather(1, lab[:, None])[:, 0]
    pred = torch.from_numpy(logits.numpy().argmax(1))
    res = {
        "pool1": p1, "pool2": p2f, "hidden": r(h), "logits": logits, "loss_rows": loss_rows,
        "correct_rows": (pred == lab).to(torch.float64), "idx1": idx1, "idx2": idx2.reshape(B, M.FEAT),
        "win1": win1, "win2": win2.reshape(B, M.FEAT, 4),
    }
    if not backward:
        return res
    # the backward's decisions: the oracle's own, or the kernel's where they are within a tie
    on_h, on2, on1, r1, r2 = pre > 0, p2f != 0, p1 != 0, idx1, idx2
    if follow is not None:
        tol = KINK_TOL[dtype]
        t1, t2, th = tol * _rms(p1), tol * _rms(p2), tol * _rms(pre)
        r1 = _follow_idx(idx1, win1, follow["idx1"], t1)
        r2 = _follow_idx(idx2, win2, torch.as_tensor(follow["idx2"]).reshape(idx2.shape), t2)
        k1 = torch.as_tensor(follow["pool1"]).reshape(p1.shape) != 0
        k2 = torch.as_tensor(follow["pool2"]).reshape(p2f.shape) != 0
        on1 = torch.where(win1.max(-1).values.abs() <= t1, k1, on1)
        on2 = torch.where(win2.max(-1).values.abs().reshape(p2f.shape) <= t2, k2, on2)
        kh = torch.as_tensor(follow["hidden"]).reshape(pre.shape) != 0
        on_h = torch.where((pre.abs() <= th) & (scale > 0), kh, on_h)
    dl = (torch.softmax(logits, 1) - F.one_hot(lab, M.NCLS).to(torch.float64)) / B
    g = {"out": r(h).t() @ dl, "out_b": dl.sum(0)}
    dh = r((dl @ p["out"].t()) * on_h * scale)
    g["wd1"] = p2f.t() @ dh
    g["bd1"] = dh.sum(0)
    res.update(dlogits=dl, dh=dh, grads=g)
    if not conv_backward:
        return res
    g2 = torch.where(on2, r(dh @ wd1.t()), torch.zeros_like(p2f)).reshape(B, 7, 7, 64)
    dz2 = _unpool(g2, r2)
    g["wc2"], dp1 = _conv_grads(p1, w2, dz2, True)
    g["bc2"] = dz2.sum((0, 1, 2))
    g1 = torch.where(on1, r(dp1), torch.zeros_like(p1))
    dz1 = _unpool(g1, r1)
    g["wc1"], _ = _conv_grads(x4, w1, dz1, False)
    g["bc1"] = dz1.sum((0, 1, 2))
    return res


# ------------------------------------------------------------------ slicings
def _views(tensor, t):
    """{slicing: (view, dims reduced per slice)} of tensor ``tensor`` holding ``t``."""
    if tensor == "wc1":
        v = t.reshape(25, 32)
        return {"tap": (v, (1,)), "cout": (v, (0,))}
    if tensor == "wc2":
        v = t.reshape(25, 32, 64)
        return {"tap": (v, (1, 2)), "cin": (v, (0, 2)), "cout": (v, (0, 1))}
    if tensor == "wd1":
        v = t.reshape(49, 64, 1024)
        return {"pixel": (v, (1, 2)), "channel": (v, (0, 2)), "column": (v, (0, 1)),
                "tile": (t.reshape(49, 64, 16, 64), (1, 3))}
    if tensor == "out":
        return {"class": (t, (0,)), "block": (t.reshape(16, 64, 10), (1, 2))}
    if tensor == "pool1":
        return {"image": (t, (1, 2, 3)), "channel": (t, (0, 1, 2))}
    if tensor == "pool2":
        v = t.reshape(t.shape[0], 49, 64)
        return {"image": (v, (1, 2)), "channel": (v, (0, 1))}
    if tensor in ("hidden", "dh"):
        return {"image": (t, (1,)), "unit": (t, (0,))}
    if tensor == "dlogits":
        return {"image": (t, (1,)), "class": (t, (0,))}
    return {}  # biases, loss rows: elementwise only


def slice_errors(got, ref, tensor):
    """{slicing: (worst error, index of the worst slice)} of ``got`` against ``ref`` (see the module
    docstring); every tensor also gets "elem": max|got - ref| / RMS(ref)."""
    got = torch.as_tensor(got).detach().to(torch.float64).reshape(ref.shape)
    ref = ref.to(torch.float64)
    rms = ref.pow(2).mean().sqrt().item()
    d = got - ref
    if not math.isfinite(d.abs().sum().item()):
        return {"elem": (float("inf"), -1)}
    out = {}
    for name, (rv, dims) in _views(tensor, ref).items():
        dv = d.reshape(rv.shape)
        n = 1
        for a in dims:
            n *= rv.shape[a]
        den = rv.pow(2).sum(dims).sqrt().clamp_min(max(rms * math.sqrt(n) * FLOOR_FRAC, 1e-300))
        e = (dv.pow(2).sum(dims).sqrt() / den).reshape(-1)
        i = int(e.argmax())
        out[name] = (e[i].item(), i)
    e = d.abs().reshape(-1)
    i = int(e.argmax())
    out["elem"] = (e[i].item() / max(rms, 1e-300), i)
    return out


def argmax_regret(got_idx, win, pooled):
    """How far from the window's maximum the value at the kernel's argmax is, in units of the pooled
    tensor's RMS: 0 when the kernel picked a maximum. (Exact equality of the positions is only
    defined where the window has no near tie; the integer-valued tests assert it.)"""
    gi = torch.as_tensor(got_idx).long().reshape(win.shape[:-1])
    if int(gi.min()) < 0 or int(gi.max()) > 3:
        return (float("inf"), -1)
    reg = (win.max(-1).values - win.gather(-1, gi[..., None])[..., 0]).reshape(-1)
    i = int(reg.argmax())
    return (reg[i].item() / max(pooled.pow(2).mean().sqrt().item(), 1e-300), i)


# ------------------------------------------------------------------ bounds
# 3x the worst value of each class over profiles/mnist_oracle_slices_r7.txt (section "bounds"; the
# tool prints this table). A class whose measured worst is exactly 0 has nothing to scale: it gets the
# format's own resolution against the tensor's RMS (2^-8 for bf16 values, 2^-23 for fp32).
#
# What the measurements say about the two precisions: the fp32 step sits at 1e-7 .. 2e-5 everywhere. The
# bf16 step's gradients are exact to ~1e-7 whenever its stored bf16 activations equal the oracle's bit
# for bit (seeds 1 and 2 at B = 3 and 5); its whole error is bf16 values that the kernel's fp32 sum and
# the oracle's fp64 sum round to neighbouring bf16 numbers, one gradient entry's worth each, so the
# smallest batches (fewest images to average over) set most of the bf16 bounds.
BOUNDS = {
    "bf16": {
        ("bc1", "elem"): 3 * 2.875e-03, ("bc2", "elem"): 3 * 1.767e-03, ("bd1", "elem"): 3 * 4.963e-03,
        ("correct_rows", "gap"): 3 * 0.000e+00, ("hidden", "elem"): 3 * 2.458e-02,
        ("hidden", "image"): 3 * 1.328e-03, ("hidden", "unit"): 3 * 6.949e-03,
        ("idx1", "regret"): 3 * 0.000e+00, ("idx2", "regret"): 3 * 8.947e-05,
        ("loss_rows", "elem"): 3 * 2.544e-04, ("out", "block"): 3 * 1.341e-03, ("out", "class"): 3 * 1.157e-03,
        ("out", "elem"): 3 * 2.055e-02, ("out_b", "elem"): 3 * 2.620e-05, ("pool1", "channel"): 3 * 5.436e-05,
        ("pool1", "elem"): 3 * 1.266e-02, ("pool1", "image"): 3 * 1.585e-04,
        ("pool2", "channel"): 3 * 5.805e-04, ("pool2", "elem"): 3 * 1.718e-02,
        ("pool2", "image"): 3 * 4.454e-04, ("wc1", "cout"): 3 * 3.841e-03, ("wc1", "elem"): 3 * 4.532e-03,
        ("wc1", "tap"): 3 * 1.688e-03, ("wc2", "cin"): 3 * 6.027e-04, ("wc2", "cout"): 3 * 3.672e-03,
        ("wc2", "elem"): 3 * 5.031e-03, ("wc2", "tap"): 3 * 6.418e-04, ("wd1", "channel"): 3 * 5.805e-04,
        ("wd1", "column"): 3 * 1.313e-02, ("wd1", "elem"): 3 * 1.782e-02, ("wd1", "pixel"): 3 * 4.851e-04,
        ("wd1", "tile"): 3 * 7.625e-04, ("dh", "elem"): 3 * 1.868e-02, ("dh", "image"): 3 * 7.031e-04,
        ("dh", "unit"): 3 * 3.151e-03, ("dlogits", "class"): 3 * 4.102e-05, ("dlogits", "elem"): 3 * 1.103e-04,
        ("dlogits", "image"): 3 * 6.143e-05,
    },
    "fp32": {
        ("bc1", "elem"): 3 * 1.867e-06, ("bc2", "elem"): 3 * 2.259e-06, ("bd1", "elem"): 3 * 2.715e-06,
        ("correct_rows", "gap"): 3 * 0.000e+00, ("hidden", "elem"): 3 * 3.551e-06,
        ("hidden", "image"): 3 * 5.756e-07, ("hidden", "unit"): 3 * 2.453e-05,
        ("idx1", "regret"): 3 * 0.000e+00, ("idx2", "regret"): 3 * 1.308e-06,
        ("loss_rows", "elem"): 3 * 1.321e-06, ("out", "block"): 3 * 8.337e-07, ("out", "class"): 3 * 3.256e-06,
        ("out", "elem"): 3 * 7.351e-06, ("out_b", "elem"): 3 * 7.701e-07, ("pool1", "channel"): 3 * 4.854e-07,
        ("pool1", "elem"): 3 * 1.021e-06, ("pool1", "image"): 3 * 8.922e-08,
        ("pool2", "channel"): 3 * 1.393e-06, ("pool2", "elem"): 3 * 5.392e-06,
        ("pool2", "image"): 3 * 4.610e-07, ("wc1", "cout"): 3 * 3.347e-06, ("wc1", "elem"): 3 * 2.964e-06,
        ("wc1", "tap"): 3 * 8.929e-07, ("wc2", "cin"): 3 * 6.660e-07, ("wc2", "cout"): 3 * 3.275e-06,
        ("wc2", "elem"): 3 * 7.134e-06, ("wc2", "tap"): 3 * 7.154e-07, ("wd1", "channel"): 3 * 1.425e-06,
        ("wd1", "column"): 3 * 5.786e-06, ("wd1", "elem"): 3 * 1.707e-05, ("wd1", "pixel"): 3 * 6.623e-07,
        ("wd1", "tile"): 3 * 8.725e-07, ("dh", "elem"): 3 * 1.548e-05, ("dh", "image"): 3 * 3.679e-06,
        ("dh", "unit"): 3 * 5.787e-06, ("dlogits", "class"): 3 * 8.481e-07, ("dlogits", "elem"): 3 * 1.208e-05,
        ("dlogits", "image"): 3 * 3.647e-06,
    },
}
ZERO_FLOOR = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -23}


def softmax_ulp(ref):
    """The head kernels form every softmax probability as exp(logit - lse) with lse = max + log(sum)
    held in fp32 (both precisions): the exponent carries the rounding of a number of the logits' size,
    2^-23 x max|logit| absolute, which is the RELATIVE error of each probability and so of every
    gradient entry, and the absolute error of a loss row. The calibration set's unsaturated logits are
    of order 1 (the allowance is below a tenth of any bound there); integer-valued and saturated-head
    inputs reach 50 - 60. Rows whose softmax is saturated outright (top probability 1 to 2^-20: the
    scale-1.0 configuration) have exact 0 / 1 probabilities and do not count."""
    lg = ref["logits"]
    live = torch.softmax(lg, 1).max(1).values < 1.0 - 2.0 ** -20
    return 2.0 ** -23 * lg[live].abs().max().item() if bool(live.any()) else 0.0


def bound_for(key, ref, dtype):
    """BOUNDS[dtype][key], its floor where the measurement is exactly 0, plus the softmax allowance for
    everything downstream of the softmax (relative for slices, scaled to the largest entry for "elem")."""
    b = BOUNDS[dtype][key]
    if b == 0.0:
        b = ZERO_FLOOR[dtype]
    t, s = key
    if t in GRADS or t in ("dlogits", "dh"):
        g = ref["grads"][t] if t in GRADS else ref[t]
        b += softmax_ulp(ref) * (g.abs().max().item() / _rms(g) if s == "elem" else 1.0)
    elif t == "loss_rows":
        b += softmax_ulp(ref) / _rms(ref["loss_rows"])
    return b


def measure(got, ref):
    """Every class's error of a kernel result ``got`` against an oracle result ``ref``:
    {(tensor, slicing): (error, worst index)}. ``got`` may hold any subset of pool1, pool2, hidden,
    loss_rows, correct_rows, idx1, idx2, dlogits (gradient at the logits), dh (at the fc1
    pre-activation) and grads{...}."""
    out = {}
    for k in ACTS:
        if k in got and k in ref:
            for s, v in slice_errors(got[k], ref[k], k).items():
                out[(k, s)] = v
    for k in GRADS:
        if k in got.get("grads", {}) and k in ref.get("grads", {}):
            for s, v in slice_errors(got["grads"][k], ref["grads"][k], k).items():
                out[(k, s)] = v
    if "correct_rows" in got:
        bad = (torch.as_tensor(got["correct_rows"]).double().reshape(-1) != ref["correct_rows"]).nonzero().reshape(-1)
        # a flipped prediction is legitimate only where the top two logits (nearly) tie
        top = ref["logits"].topk(2, 1).values
        gap = (top[:, 0] - top[:, 1]) / max(ref["logits"].pow(2).mean().sqrt().item(), 1e-300)
        out[("correct_rows", "gap")] = (gap[bad].max().item(), int(bad[gap[bad].argmax()])) if len(bad) else (0.0, -1)
    for k, w, pl in (("idx1", "win1", "pool1"), ("idx2", "win2", "pool2")):
        if k in got:
            out[(k, "regret")] = argmax_regret(got[k], ref[w], ref[pl])
    return out


def check(got, ref, dtype, only=None):
    """The classes of ``measure(got, ref)`` above their bound: {(tensor, slicing): (error, bound, index)}.
    Empty when the result passes. ``only``: restrict to these tensors."""
    bad = {}
    for key, (e, i) in measure(got, ref).items():
        if only is not None and key[0] not in only:
            continue
        b = bound_for(key, ref, dtype)
        if not e <= b:
            bad[key] = (e, b, i)
    return bad


# ------------------------------------------------------------------ inputs shared by the tests and the tool
STANDARD = [(0.05, 128), (1.0, 128), (0.05, 40)]  # (scale, B) of test_step_grads_match_oracle
EDGE_BATCHES = (1, 2, 3, 5, 37, 63, 65, 130)
# B = 1: nothing to tile; 2, 3, 5: fewer rows than a 16-B loader chunk, empty batch quarters in the
# output-layer gradient (B < 4), half-filled image groups (4 in bf16, 2 in fp32); 37: prime; 63 / 65:
# either side of the 64-row GEMM tiles; 130: three row tiles, the last with two rows.


def random_case(B, scale=0.05, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = {k: v * scale for k, v in M.init_params(7 + seed).items()}
    x = torch.rand(B, 784, generator=g)
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return params, x, y


INTEGER_SEED = 4  # gives top-logit ties at B = 5 and at B = 37, and thousands of positive pool ties


def integer_case(B, seed=INTEGER_SEED):
    """Images in {0,1} (density 0.3); every weight tensor zero except a few +-1 per output unit (6
    conv1, 8 conv2, 6 fc1, 12 output layer); integer biases in [-2, 2]. Every forward value is then a
    small integer, exact in bf16 and fp32 under any summation order."""
    g = torch.Generator().manual_seed(seed)

    def sparse(fan_in, n_out, k):
        w = torch.zeros(fan_in, n_out)
        for j in range(n_out):
            rows = torch.randperm(fan_in, generator=g)[:k]
            w[rows, j] = (torch.randint(0, 2, (k,), generator=g) * 2 - 1).float()
        return w

    params = {
        "wc1": sparse(25, 32, 6).reshape(5, 5, 1, 32), "wc2": sparse(800, 64, 8).reshape(5, 5, 32, 64),
        "wd1": sparse(M.FEAT, M.HID, 6), "out": sparse(M.HID, M.NCLS, 12),
        "bc1": torch.randint(-2, 3, (32,), generator=g).float(), "bc2": torch.randint(-2, 3, (64,), generator=g).float(),
        "bd1": torch.randint(-2, 3, (M.HID,), generator=g).float(),
        "out_b": torch.randint(-2, 3, (M.NCLS,), generator=g).float(),
    }
    x = (torch.rand(B, 784, generator=g) < 0.3).float()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    # a row whose top logits tie is labelled with the LAST of the tied classes: the first-maximum
    # prediction is then wrong, a last-maximum one would be counted correct
    lg = oracle_step(params, x, y, "fp32", backward=False)["logits"]
    tied = lg == lg.max(1, keepdim=True).values
    for b in (tied.sum(1) > 1).nonzero().reshape(-1).tolist():
        y[b] = int(tied[b].nonzero().max())
    return params, x, y


IMPULSES = [(0, 0), (0, 27), (27, 0), (27, 27), (0, 14), (14, 0), (27, 14), (14, 27), (14, 14)]


def impulse_images():
    x = torch.zeros(len(IMPULSES), 28, 28)
    for i, (r, c) in enumerate(IMPULSES):
        x[i, r, c] = 1.0
    return x.reshape(-1, 784)


def impulse_case(B):
    """Dense random weights; one image per impulse position (single 1.0 pixel at the four corners, the
    four edge midpoints and the centre): B = 9 holds just those, a larger batch has them as its first
    and its last nine images with random images between."""
    params, x, y = random_case(B)
    imp = impulse_images()
    x = x.clone()
    x[:9] = imp
    x[B - 9:] = imp
    return params, x, y


def neighbours_case(B, reverse=False):
    """blank, all-ones, random, blank, random, all-ones (the first B of them), dense random weights."""
    params, x, y = random_case(B)
    x = x.clone()
    for i, kind in enumerate(["blank", "ones", "random", "blank", "random", "ones"][:B]):
        if kind == "blank":
            x[i] = 0.0
        elif kind == "ones":
            x[i] = 1.0
    if reverse:
        x, y = x.flip(0), y.flip(0)
    return params, x, y


def saturated_case(B, labels):
    """random_case with the output layer scaled so that the largest |logit| of the fp64 forward is 60:
    e^-120 is still a normal fp32 number's neighbourhood (no overflow anywhere), every softmax is
    saturated. labels: "zeros", "nines" or "argmin" (each row's least likely class)."""
    params, x, y = random_case(B)
    lg = oracle_step(params, x, y, "fp32", backward=False)["logits"]
    f = 60.0 / lg.abs().max().item()
    params = dict(params)
    params["out"] = params["out"] * f
    params["out_b"] = params["out_b"] * f
    if labels == "zeros":
        y = torch.zeros(B, dtype=torch.int32)
    elif labels == "nines":
        y = torch.full((B,), 9, dtype=torch.int32)
    else:
        y = (lg * f).argmin(1).to(torch.int32)
    return params, x, y


def run_engine(dev, dtype, params, x, y, keep=1.0, seed=1234, backward=True, train=True):
    """One forward (+ backward) of the native engine at global step 0 on ``dev``; returns the result in
    ``measure``'s format plus dlogits / dh."""
    from tensorflow_distributed_amd import _native

    _native.require()
    B = x.shape[0]
    eng = torch.classes.tfd.MnistEngine(B, dev.index or 0, keep, seed, 0)
    eng.set_dtype(dtype)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(M.flat_from_dict(params).to(dev))
        eng.sync_shadow()
        eng.feed_x().copy_(x.to(dev))
        eng.feed_y().copy_(torch.as_tensor(y).to(torch.int32).to(dev))
        eng.forward(train)
        if backward:
            eng.backward_a()
            eng.backward_b()
    torch.cuda.synchronize()
    return collect(eng, backward, train)


def collect(eng, backward=True, train=True):
    """The engine's last step in ``measure``'s format (plus dlogits / dh)."""
    got = {
        "pool1": eng.pool1().double().cpu(), "pool2": eng.pool2().double().cpu(),
        "loss_rows": eng.loss_rows().double().cpu(), "correct_rows": eng.correct_rows().double().cpu(),
        "idx1": eng.pool1_argmax().cpu(), "idx2": eng.pool2_argmax().cpu(),
    }
    if train:
        got["hidden"] = eng.hidden().double().cpu()
    if backward:
        got["grads"] = {k: v.double().clone() for k, v in M.dict_from_flat(eng.grads().cpu()).items()}
        got["dlogits"] = eng.dlogits().double().cpu()
        got["dh"] = eng.dhidden().double().cpu()
    return got


# ------------------------------------------------------------------ the fused one-GPU step
# train_step() with set_fused_tail(1) ends in ONE launch (mnist_adam_kernel, csrc/mnist_tail.h) that sums
# the conv weight-gradient slabs, reads the fc-region gradient (bf16 with set_local_bf16_grads) and
# applies Adam: the gradient it consumes is never stored. It is read back out of Adam's m instead
# (grads_from_adam_m) and goes through the same per-slice checker as the unfused step's grads().
#
# The batches of tests/test_mnist_fused_step_gpu.py, on the edges of the tail's slab loops. conv1:
# 2 B slabs, a pass of slab_sum<16> takes 16 x 16 = 256, thread group q sums slabs q, q + 16, ...;
# conv2: ceil(B / 4) slabs (bf16) or ceil(B / 2) (fp32), a pass of slab_sum<4> takes 4 x 16 = 64.
#   1, 2, 3, 5: 2, 4, 6, 10 conv1 slabs for 16 q groups, 1 .. 3 conv2 slabs for 4; B = 1, 2, 3, 5 (bf16)
#       and 1, 3, 5 (fp32) leave the last conv2 image group half filled;
#   37: prime -- 74 conv1 slabs (q groups with 5 and with 4 slabs), 10 / 19 conv2 slabs;
#   65: 130 conv1 slabs; fp32: 33 conv2 slabs, the last holding one image;
#   130: 260 conv1 slabs = one full pass and a second of 4; fp32: 65 conv2 slabs = a second pass of one;
#   258 (bf16 only): 516 conv1 slabs = two full passes and 4; 65 conv2 slabs = a second pass of one, half
#       filled.
FUSED_BATCHES = {"bf16": (1, 2, 3, 5, 37, 65, 130, 258), "fp32": (1, 2, 3, 5, 37, 65, 130)}
FC_GRADS = ("wd1", "bd1", "out", "out_b")
# The scheduled and the EMA instantiations' settings: set_lr_schedule's (kind, [lr, decay_steps, rate, end,
# power, alpha, warmup_steps, staircase], boundaries, values) -- lr = 1e-4 * 0.5^s -- and set_ema's (decay,
# num_updates). They run at global step 1, where the schedule's rate is not its base rate, so one Adam
# step precedes the checked one, and the rate is small for that step's sake: at 0.01 it moves every
# parameter of the B = 3 case by 0.01 the same way for all three images, the logits reach +-45, and there
# the fp32 step -- fused and unfused alike, they agree to 2.5e-8 -- is up to 1.8e-4 from the oracle, 11x a
# bound calibrated on logits of order 1 (profiles/mnist_fused_step_slices.txt, last section).
FUSED_LR = 1e-4
FUSED_SCHEDULE = ("exponential", [FUSED_LR, 1.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0], [], [])
FUSED_EMA = (0.99, True)
# Classes of the fused step whose bound is not BOUNDS + allowance: 3x the value measured on the fused
# path against the oracle, each cited to profiles/mnist_fused_step_slices.txt. (None was needed.)
FUSED_BOUNDS = {"bf16": {}, "fp32": {}}


def _f32(v):
    """The fp32 value the kernel holds for a host double, as a Python float."""
    return float(np.float32(v))


def run_fused_step(dev, dtype, params, x, y, keep=1.0, *, local_bf16=False, dataset=False, schedule=None, ema=None,
                   step0=0, b1=0.9, b2=0.999, lr=0.01, eps=1e-8):
    """One fused one-GPU Adam step (set_fused_tail(1)) of the native engine from m = v = 0, at global
    step ``step0``, on the rows ``x, y``; everything needed to check it afterwards.

    params: dict of tensors. schedule: the (kind, params, boundaries, values) of set_lr_schedule or None.
    ema: (decay, num_updates) or None. dataset=True: the rows come from a device dataset of
    n = 2 B + 3 rows through a fixed non-identity permutation (so the cursor wraps at step 1); the
    dataset is laid out so that step ``step0`` draws exactly ``x, y`` -- row perm[(step0 B + b) % n]
    holds x[b] -- and the other rows are random. step0 > 0: that many ordinary fused steps run first (feed
    mode: on the same x, y), then m and v are zeroed in place on the same stream; the step counter, the
    dropout key, Adam's t and the data cursor stay advanced.

    Returns a dict: p_before, p_after, m_after, v_after (fp32, CPU), params_bf16_before / params_bf16,
    ema_before / ema_after (None without EMA), step (step_tensor() after), t = step0 + 1, lr (the fp32
    rate of this update, lr_at_step(step0)), ema_decay (ema_decay_at_step(t)), b1 / b2 / eps, x / y (the
    rows the step used: read back through perm in dataset mode), acts (collect(eng, backward=False))."""
    from tensorflow_distributed_amd import _native

    _native.require()
    B = x.shape[0]
    eng = torch.classes.tfd.MnistEngine(B, dev.index or 0, keep, 1234, 0)
    eng.set_dtype(dtype)
    eng.set_adam(lr, b1, b2, eps)
    eng.set_fused_tail(1)
    eng.set_local_bf16_grads(1 if local_bf16 else 0)
    if schedule is not None:
        eng.set_lr_schedule(*schedule)
    yi = torch.as_tensor(y).to(torch.int32)
    if dataset:
        n = 2 * B + 3
        g = torch.Generator().manual_seed(11)
        data = torch.rand(n, 784, generator=g)
        labels = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
        perm = torch.randperm(n, generator=g)
        assert not torch.equal(perm, torch.arange(n))
        used = perm[(step0 * B + torch.arange(B)) % n]
        data[used] = x.to(torch.float32)
        labels[used] = yi
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(M.flat_from_dict(params).to(dev))
        eng.sync_shadow()
        if ema is not None:
            eng.set_ema(float(ema[0]), bool(ema[1]))  # copies the parameters into the shadow
        if dataset:
            eng.set_dataset(data.to(dev), labels.to(dev), perm.to(torch.int32).to(dev))
            eng.set_input_mode(1)
        else:
            eng.feed_x().copy_(x.to(torch.float32).to(dev))
            eng.feed_y().copy_(yi.to(dev))
        for _ in range(step0):
            eng.train_step()
        if step0:
            eng.adam_m().zero_()
            eng.adam_v().zero_()
        res = {
            "p_before": eng.params().clone(), "params_bf16_before": eng.params_bf16().clone(),
            "ema_before": eng.ema_params().clone() if ema is not None else None,
        }
        eng.train_step()
    torch.cuda.synchronize()
    res = {k: (v.cpu() if v is not None else None) for k, v in res.items()}
    t = step0 + 1
    res.update(
        p_after=eng.params().cpu(), m_after=eng.adam_m().cpu(), v_after=eng.adam_v().cpu(),
        params_bf16=eng.params_bf16().cpu(), ema_after=eng.ema_params().cpu() if ema is not None else None,
        step=int(eng.step_tensor().item()), t=t, lr=float(eng.lr_at_step(step0)),
        ema_decay=float(eng.ema_decay_at_step(t)) if ema is not None else None,
        b1=b1, b2=b2, eps=eps, acts=collect(eng, backward=False),
    )
    if dataset:
        res["x"], res["y"] = data[used].clone(), labels[used].clone()
    else:
        res["x"], res["y"] = x.to(torch.float32).clone(), yi.clone()
    return res


def grads_from_adam_m(m_after, b1=0.9):
    """The gradient a step that started from m = 0 consumed, fp64 on the CPU: the tail writes
    m' = m + (g - m) * c1 = g * c1 with c1 = 1.f - beta1 (exact in fp32 for beta1 in [0.5, 1]), ONE fp32
    rounding, so m' / c1 is g to within 2^-24 relative per element -- in every region, whatever the
    order the slabs were summed in."""
    c1 = float(np.float32(1.0) - np.float32(b1))
    return torch.as_tensor(m_after).detach().cpu().to(torch.float64) / c1


def fused_allowance(key, ref, dtype, local_bf16):
    """What check_fused adds to bound_for(key, ref, dtype). Derived from the number formats, not
    measured:

      the recovery  g_used = m' / c1 carries the one fp32 rounding of g * c1: |g_used - g| <= 2^-24 |g|
                    per element. Over any slice that is a relative L2 error <= 2^-24; an element is off by
                    <= 2^-24 max|g|, which the "elem" measure divides by RMS(g). Both doubled: 2^-23 and
                    2^-23 max|g| / RMS(g).
      local_bf16    the fc backward stores the fc-region gradient (wd1, bd1, out, out_b) as bf16 and the
                    tail reads that: one round-to-nearest to 8 significant bits, <= 2^-9 |g| per element,
                    so <= 2^-9 relative L2 per slice and <= 2^-9 max|g| for an element. Doubled: 2^-8 and
                    2^-8 max|g| / RMS(g). (bf16 dtype only: the fp32 step has no such option.)

    Everything that is not a gradient gets 0."""
    t, s = key
    if t not in GRADS:
        return 0.0
    g = ref["grads"][t]
    peak = g.abs().max().item() / _rms(g) if s == "elem" else 1.0
    a = 2.0 ** -23 * peak
    if local_bf16 and t in FC_GRADS:
        a += 2.0 ** -8 * peak
    return a


def fused_bound_for(key, ref, dtype, local_bf16):
    """The bound of one class on the fused step: FUSED_BOUNDS where the class has an entry (with the
    softmax allowance bound_for adds), else bound_for; plus fused_allowance."""
    base = bound_for(key, ref, dtype)
    if key in FUSED_BOUNDS[dtype]:
        base += FUSED_BOUNDS[dtype][key] - (BOUNDS[dtype][key] or ZERO_FLOOR[dtype])
    return base + fused_allowance(key, ref, dtype, local_bf16)


def fused_got(res):
    """A fused step's result (run_fused_step) in ``measure``'s format: the forward's activations plus
    the gradient the tail consumed, split per tensor."""
    got = dict(res["acts"])
    got["grads"] = {k: v.clone() for k, v in M.dict_from_flat(grads_from_adam_m(res["m_after"], res["b1"])).items()}
    return got


def fused_oracle(res, dtype, keep=1.0, step=0):
    """The oracle's step on what the fused step read: p_before, the rows it used, the dropout mask of
    global step ``step``, the kernel's side of near ties (``follow``)."""
    B = res["x"].shape[0]
    mask = M.native_dropout_mask(B, step, 0, 1234, keep) if keep < 1.0 else None
    params = {k: v.clone() for k, v in M.dict_from_flat(res["p_before"]).items()}
    return oracle_step(params, res["x"], res["y"], dtype, keep, mask, follow=res["acts"])


def measure_fused(res, ref, dtype, local_bf16, only=None):
    """{(tensor, slicing): (error, bound, index)} of every class of the fused step (all of them, passing
    or not)."""
    out = {}
    for key, (e, i) in measure(fused_got(res), ref).items():
        if only is None or key[0] in only:
            out[key] = (e, fused_bound_for(key, ref, dtype, local_bf16), i)
    return out


def check_fused(res, ref, dtype, local_bf16, only=None):
    """``check`` for a fused step: the classes above bound_for + fused_allowance, in the same
    {(tensor, slicing): (error, bound, index)} shape. Empty when the step passes."""
    return {k: v for k, v in measure_fused(res, ref, dtype, local_bf16, only).items() if not v[0] <= v[1]}


def adam_reference(p_before, g_used, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """fp64 (m, v, p') of TF's ApplyAdam from m = v = 0:  m = g (1 - b1), v = g^2 (1 - b2),
    p' = p - lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps).  b1, b2, eps and lr are rounded to the
    fp32 values the kernel holds (pass lr = lr_at_step(t - 1) under a schedule); t = step0 + 1."""
    b1, b2, eps, lr = _f32(b1), _f32(b2), _f32(eps), _f32(lr)
    p = torch.as_tensor(p_before).detach().cpu().to(torch.float64)
    g = torch.as_tensor(g_used).to(torch.float64)
    m = g * (1.0 - b1)
    v = g * g * (1.0 - b2)
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return m, v, p - lr_t * m / (v.sqrt() + eps)


FP32_TINY = 2.0 ** -126  # the smallest normal fp32 number: below it a product has no relative precision


def update_ratios(res):
    """The fused step's v and p' against adam_reference from its own consumed gradient, as the worst
    ratios error / tolerance (<= 1 passes):
      v   |v - v_ref| <= 2^-22 v_ref (+ FP32_TINY: g * g below the normal range is flushed or rounded
          with no relative precision; such a v is 1e-30 of sqrt's eps-sized partner in the update);
      p   |p' - p_ref| <= 2^-24 |p_ref| + 2^-18 |p_ref - p_before|."""
    g = grads_from_adam_m(res["m_after"], res["b1"])
    _, v_ref, p_ref = adam_reference(res["p_before"], g, res["t"], res["lr"], res["b1"], res["b2"], res["eps"])
    v, p, p0 = res["v_after"].double(), res["p_after"].double(), res["p_before"].double()
    rv = (v - v_ref).abs() / (2.0 ** -22 * v_ref + FP32_TINY)
    rp = (p - p_ref).abs() / (2.0 ** -24 * p_ref.abs() + 2.0 ** -18 * (p_ref - p0).abs()).clamp_min(1e-300)
    rp = torch.where(p == p_ref, torch.zeros_like(rp), rp)
    iv, ip = int(rv.argmax()), int(rp.argmax())
    return {"v": (rv[iv].item(), iv), "p": (rp[ip].item(), ip)}
