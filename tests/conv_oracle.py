"""fp64 oracles of the generic NHWC kernel library (conv / dense / batch norm / pooling / softmax
cross-entropy, csrc/conv_kernels.h) and a localised per-element checker.

A helper module (like tests/mnist_oracle.py), shared by tests/test_conv_oracle_checker_cpu.py,
tests/test_conv_oracle_gpu.py and tools/conv_oracle_rel.py.

References: plain torch / numpy on the CPU in fp64, NHWC activations, HWIO filters. The convolutions
are written as one matrix product per filter tap, not through torch's conv, so they are independent of
it (the CPU test compares them with torch's fp64 autograd).

Two families of cases.

Exact: integer-valued operands with sum |a||b| < 2^24 for every output element. A bf16 x bf16 product is
exact in fp32 and an fp32 sum of integers below 2^24 is exact in any order (split-K and slot-mode
atomics included), so every fp32 output has exactly one right bit pattern -- the integer -- and every
bf16 output is ``bf16_rne`` of it. The generators assert exactness on the host: a failing assertion
means wrong inputs, a failing comparison a wrong kernel.

Random: bf16-rounded normal operands, reduction length L <= 1152, with the derived bound

    fp32 output   |got - ref| <= e                         e = L * 2^-23 * A
    bf16 output   |got - ref| <= 2^-8 (|ref| + e) + e

where A is the same operation on the operands' absolute values (|add| included). Every partial sum
of an fp32 accumulation of L terms is bounded by A and rounded at 2^-24 relative, L - 1 roundings in
any order: (L - 1) 2^-24 A. The factor 2 on top covers the matrix core's internal order (several
products summed per instruction before one rounding) and the split-K final add. bf16 keeps 8
significant bits, so rounding a value v to nearest moves it by at most half a spacing, which is at
most 2^-8 |v| (reached just above a power of two); with |v| <= |ref| + e that is the first term, and
a store that truncates (up to 2^-7 |v|) exceeds it. None of this is measured on the kernels
(tools/conv_oracle_rel.py records how much of each bound they use: up to 0.99 of the bf16 bounds, a
few percent of the fp32 ones).
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

F64 = torch.float64
EXACT_LIMIT = float(2 ** 24)
U = 2.0 ** -24  # fp32 unit roundoff


# ---------------------------------------------------------------- bf16 rounding on bit patterns
def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16, nearest even, on the fp32 bit pattern (no torch cast): fp64 values out.
    The operand is taken through fp32 first (exact for the integers of the exact family)."""
    f = np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy())
    u = f.view(np.uint32).astype(np.uint64)
    lsb = (u >> np.uint64(16)) & np.uint64(1)
    r = ((u + np.uint64(0x7FFF) + lsb) & np.uint64(0xFFFF0000)).astype(np.uint32)
    nan = np.isnan(f)
    if nan.any():
        r[nan] = np.uint32(0x7FC00000)
    return torch.from_numpy(r.view(np.float32).astype(np.float64)).reshape(t.shape)


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
    """The wrong rounding (toward zero) -- a mutation for the checker's own test."""
    f = np.ascontiguousarray(t.detach().to(torch.float32).cpu().numpy())
    r = f.view(np.uint32) & np.uint32(0xFFFF0000)
    return torch.from_numpy(r.view(np.float32).astype(np.float64)).reshape(t.shape)


# ---------------------------------------------------------------- convolution, one product per tap
def out_hw(H, W, R, S, st, pad):
    return (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1


def _pad_hw(x, pad):
    return torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x


def _tap(xp, r, s, st, Ho, Wo):
    return xp[:, r:r + st * (Ho - 1) + 1:st, s:s + st * (Wo - 1) + 1:st, :]


def conv_fwd(x, w, st, pad, tap_scale=None):
    """y[n,ho,wo,k] = sum_{r,s,c} x[n, ho*st - pad + r, wo*st - pad + s, c] w[r,s,c,k]; x NHWC, w HWIO.
    tap_scale {(r, s): f} scales single taps (mutations for the checker's test)."""
    x, w = x.to(F64), w.to(F64)
    N, H, W, C = x.shape
    R, S, _, K = w.shape
    Ho, Wo = out_hw(H, W, R, S, st, pad)
    xp = _pad_hw(x, pad)
    y = torch.zeros(N, Ho, Wo, K, dtype=F64)
    for r in range(R):
        for s in range(S):
            f = 1.0 if tap_scale is None else tap_scale.get((r, s), 1.0)
            y += f * (_tap(xp, r, s, st, Ho, Wo) @ w[r, s])
    return y


def apply_add(dx, add=None, bits=None, sub2=False):
    """The dgrad epilogue's add operand: plain; masked by relu bits [M][C/8] (bit j of byte (m, c/8) keeps
    channel 8 (c/8) + j); or a [N, ceil(H/2), ceil(W/2), C] operand added at the even pixels."""
    if add is None:
        return dx
    add = add.to(F64)
    if bits is not None:
        add = add * unpack_bits(bits, add.shape[-1]).reshape(add.shape).to(F64)
    if sub2:
        dx = dx.clone()
        dx[:, ::2, ::2, :] += add
        return dx
    return dx + add


def conv_dgrad(dy, w, xshape, st, pad, add=None, bits=None, sub2=False, drop_phase=None):
    """dx = conv-transpose(dy, w) (+ add). drop_phase (ph, pw): that (h mod st, w mod st) phase of the
    conv part is left zero (a mutation)."""
    dy, w = dy.to(F64), w.to(F64)
    N, H, W, C = xshape
    R, S, _, K = w.shape
    Ho, Wo = out_hw(H, W, R, S, st, pad)
    assert tuple(dy.shape) == (N, Ho, Wo, K), (dy.shape, (N, Ho, Wo, K))
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=F64)
    for r in range(R):
        for s in range(S):
            _tap(dxp, r, s, st, Ho, Wo).add_(dy @ w[r, s].t())
    dx = dxp[:, pad:pad + H, pad:pad + W, :].clone()
    if drop_phase is not None:
        dx[:, drop_phase[0]::st, drop_phase[1]::st, :] = 0
    return apply_add(dx, add, bits, sub2)


def conv_wgrad(x, dy, R, S, st, pad):
    """dw[r,s,c,k] = sum_{n,ho,wo} x[n, ho*st - pad + r, wo*st - pad + s, c] dy[n,ho,wo,k]."""
    x, dy = x.to(F64), dy.to(F64)
    N, H, W, C = x.shape
    _, Ho, Wo, K = dy.shape
    xp = _pad_hw(x, pad)
    dw = torch.zeros(R, S, C, K, dtype=F64)
    for r in range(R):
        for s in range(S):
            dw[r, s] = _tap(xp, r, s, st, Ho, Wo).reshape(-1, C).t() @ dy.reshape(-1, K)
    return dw


def bn_relu_in(x, mean, invstd, gamma, beta):
    """The folded conv input: relu(bn(x)) with the forward's constants sc = invstd gamma, sh = beta -
    mean sc, rounded to bf16 (the loader stages bf16). Zero-padded taps stay zero: the affine acts
    on the pixels only, the conv pads afterwards."""
    sc = invstd.to(F64) * gamma.to(F64)
    sh = beta.to(F64) - mean.to(F64) * sc
    return bf16_rne(torch.relu(x.to(F64) * sc + sh))


def linear_fwd(x, w, b=None):
    y = x.to(F64) @ w.to(F64)
    return y if b is None else y + b.to(F64)


def linear_dgrad(dy, w):
    return dy.to(F64) @ w.to(F64).t()


def linear_wgrad(x, dy):
    return x.to(F64).t() @ dy.to(F64)


# ---------------------------------------------------------------- relu bits
def pack_bits(mask):
    """bool [M, C] -> uint8 [M, C/8], bit j of byte (m, c/8) = channel 8 (c/8) + j."""
    M, C = mask.shape
    m = mask.reshape(M, C // 8, 8).to(torch.int64)
    return (m << torch.arange(8)).sum(-1).to(torch.uint8)


def unpack_bits(bits, C, reverse=False):
    """uint8 [M, C/8] -> bool [M, C]. reverse: bit 7 - j (the wrong order, a mutation)."""
    b = bits.reshape(-1, C // 8).to(torch.int64)
    sh = torch.arange(7, -1, -1) if reverse else torch.arange(8)
    return ((b.unsqueeze(-1) >> sh) & 1).reshape(-1, C).bool()


# ---------------------------------------------------------------- statistics partials (column sums)
def fwd_stats(y_exact):
    """Column sums and sums of squares of the STORED bf16 output [2, K] (the M real rows only)."""
    yb = bf16_rne(y_exact).reshape(-1, y_exact.shape[-1])
    return torch.stack([yb.sum(0), (yb * yb).sum(0)])


def bn_mask(mode, y, mean, invstd, gamma, beta, bits):
    """The BN-backward relu mask [M, C]: mode 0 none; 2 recomputed from y (fma(y, invstd gamma, beta -
    mean invstd gamma) > 0); 3 the given relu bits."""
    C = y.shape[-1]
    y2 = y.to(F64).reshape(-1, C)
    if mode == 0:
        return torch.ones_like(y2, dtype=torch.bool)
    if mode == 2:
        sc = invstd.to(F64) * gamma.to(F64)
        return (y2 * sc + (beta.to(F64) - mean.to(F64) * sc)) > 0
    assert mode == 3
    return unpack_bits(bits, C)


def dgrad_bn_stats(dx_exact, y, mean, invstd, mask):
    """[2, C]: column sums of d and d (y - mean) invstd with d = the stored bf16 gradient through mask."""
    C = y.shape[-1]
    d = bf16_rne(dx_exact).reshape(-1, C) * mask.to(F64)
    xhat = (y.to(F64).reshape(-1, C) - mean.to(F64)) * invstd.to(F64)
    return torch.stack([d.sum(0), (d * xhat).sum(0)])


# ---------------------------------------------------------------- batch norm
def bn_fwd(y, gamma, beta, res=None, relu=False, eps=1e-5):
    """Training-mode BN over the rows of [M, C]: out (unrounded fp64), mean, invstd, var (biased)."""
    y = y.to(F64)
    C = y.shape[-1]
    y2 = y.reshape(-1, C)
    mean = y2.mean(0)
    var = ((y2 - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    z = (y2 - mean) * invstd * gamma.to(F64) + beta.to(F64)
    if res is not None:
        z = z + res.to(F64).reshape(-1, C)
    if relu:
        z = torch.relu(z)
    return z.reshape(y.shape), mean, invstd, var


def bn_running(rm, rv, mean, var, M, momentum):
    """TF decay semantics, unbiased variance: r = r m + x (1 - m)."""
    return (rm.to(F64) * momentum + mean * (1 - momentum),
            rv.to(F64) * momentum + var * (M / max(M - 1, 1)) * (1 - momentum))


def bn_bwd(dout, y, gamma, mean, invstd, mask=None):
    """dz = dout through mask; dbeta = sum dz, dgamma = sum dz xhat,
    dy = gamma invstd (dz - dbeta / M - xhat dgamma / M); dres = dz."""
    C = y.shape[-1]
    y2, d = y.to(F64).reshape(-1, C), dout.to(F64).reshape(-1, C)
    M = y2.shape[0]
    dz = d if mask is None else d * mask.reshape(-1, C).to(F64)
    xhat = (y2 - mean.to(F64)) * invstd.to(F64)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dy = gamma.to(F64) * invstd.to(F64) * (dz - dbeta / M - xhat * dgamma / M)
    return dy.reshape(y.shape), dz.reshape(y.shape), dgamma, dbeta


def bn_infer(y, gamma, beta, rm, rv, eps, relu):
    z = (y.to(F64) - rm.to(F64)) / torch.sqrt(rv.to(F64) + eps) * gamma.to(F64) + beta.to(F64)
    return torch.relu(z) if relu else z


# ---------------------------------------------------------------- pooling
def _windows(x, k, st, pad, fill):
    """[N,H,W,C] -> [N,Ho,Wo,C,k*k], window axis in (r, s) order; out-of-image taps = fill."""
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, k, k, st, pad)
    xp = torch.full((N, H + 2 * pad, W + 2 * pad, C), fill, dtype=F64)
    xp[:, pad:pad + H, pad:pad + W, :] = x.to(F64)
    return torch.stack([_tap(xp, r, s, st, Ho, Wo) for r in range(k) for s in range(k)], -1)


def maxpool_fwd(x, k, st, pad, last=False):
    """Max pool and its argmax r*k + s: the FIRST maximum in (r, s) order (the kernels' strict >).
    last=True takes the last one (a mutation)."""
    win = _windows(x, k, st, pad, -math.inf).numpy()
    if last:
        idx = win.shape[-1] - 1 - win[..., ::-1].argmax(-1)
    else:
        idx = win.argmax(-1)
    idx = torch.from_numpy(np.ascontiguousarray(idx))
    y = torch.from_numpy(win).gather(-1, idx[..., None])[..., 0]
    return y, idx.to(torch.uint8)


def maxpool_bwd(dy, am, xshape, k, st, pad):
    """Every input element sums the gradients of the windows whose argmax points at it."""
    N, H, W, C = xshape
    _, Ho, Wo, _ = dy.shape
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=F64)
    am = am.to(torch.int64)
    for r in range(k):
        for s in range(k):
            _tap(dxp, r, s, st, Ho, Wo).add_(dy.to(F64) * (am == r * k + s).to(F64))
    return dxp[:, pad:pad + H, pad:pad + W, :].clone()


def avgpool_fwd(x):
    return x.to(F64).mean((1, 2))


def avgpool_bwd(dy, xshape):
    N, H, W, C = xshape
    return (dy.to(F64) / (H * W))[:, None, None, :].expand(N, H, W, C).clone()


# ---------------------------------------------------------------- softmax cross-entropy
def softmax_xent(z, labels):
    """loss rows, correct rows (prediction = the first maximal logit), dlogits = (softmax - onehot) / N."""
    z = z.to(F64)
    N, K = z.shape
    lab = labels.long()
    mx = z.max(1, keepdim=True).values
    lse = mx[:, 0] + torch.log(torch.exp(z - mx).sum(1))
    loss = lse - z.gather(1, lab[:, None])[:, 0]
    pred = torch.from_numpy(z.numpy().argmax(1))
    dl = (torch.exp(z - lse[:, None]) - torch.nn.functional.one_hot(lab, K).to(F64)) / N
    return loss, (pred == lab).to(F64), dl


# ---------------------------------------------------------------- exact cases
def _ints(g, shape, amp, density):
    v = torch.randint(-amp, amp + 1, shape, generator=g).to(F64)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).to(F64)
    return v


def assert_exact(*abs_results):
    """Each argument: the operation evaluated on the operands' absolute values. All below 2^24."""
    for a in abs_results:
        m = float(a.abs().max()) if a.numel() else 0.0
        assert m < EXACT_LIMIT, f"case is not exact: sum |a||b| reaches {m:.3e} >= 2^24 (inputs, not the kernel)"


# (amp, density) from rich (outputs beyond 256, bf16 ties) to thin (large-M statistics)
_LADDER = [(12, 1.0), (8, 1.0), (5, 1.0), (3, 1.0), (2, 1.0), (1, 1.0), (1, 0.5), (1, 0.25), (1, 0.1), (1, 0.04)]


def exact_fwd_case(shape, seed=0, stats=False, fold=False):
    """(N,H,W,C,K,R,st,pad) -> dict x, w, y (exact), and with stats the column sums. Takes the
    richest rung of _LADDER on which the case is exact (sum |x||w| < 2^24; with stats also every
    per-channel sum of y^2 of the stored output < 2^24).
    fold: x is a pre-BN tensor and the conv input is relu(bn(x)) with integer mean / beta and
    power-of-two invstd / gamma (keys mean, invstd, gamma, beta, xin)."""
    N, H, W, C, K, R, st, pad = shape
    for amp, dens in _LADDER:
        g = torch.Generator().manual_seed(seed)
        x = _ints(g, (N, H, W, C), amp, dens)
        w = _ints(g, (R, R, C, K), amp, 1.0)
        case = {"x": x, "w": w}
        xin = x
        if fold:
            case.update(_bn_consts(g, C, False))
            xin = bn_relu_in(x, case["mean"], case["invstd"], case["gamma"], case["beta"])
            assert torch.equal(xin, torch.round(xin)) and float(xin.abs().max()) <= 256  # exact bf16 integers
        case["xin"] = xin
        ya = conv_fwd(xin.abs(), w.abs(), st, pad)
        if float(ya.max()) >= EXACT_LIMIT:
            continue
        y = conv_fwd(xin, w, st, pad)
        if stats:
            s = fwd_stats(y)
            if float(s[1].max()) >= EXACT_LIMIT:
                continue
            case["stats"] = s
            assert_exact(s[1])
        assert_exact(ya)
        case["y"] = y
        return case
    raise AssertionError(f"no exact rung for {shape}")


def _bn_consts(g, C, backward):
    """Integer mean and beta, power-of-two invstd and gamma (either sign), so that the affine, xhat and
    the mode-2 mask are exact integers. Forward fold: invstd in {1, 2}. Backward: invstd in {1/2, 1}
    with an even mean (the case's y is even)."""
    sign = (1 - 2 * torch.randint(0, 2, (C,), generator=g)).to(F64)
    mean = torch.randint(-2, 3, (C,), generator=g).to(F64)
    inv = 2.0 ** torch.randint(0, 2, (C,), generator=g).to(F64)
    return {"mean": 2 * mean if backward else mean, "invstd": inv / 2 if backward else inv,
            "gamma": sign * 2.0 ** torch.randint(0, 2, (C,), generator=g).to(F64),
            "beta": torch.randint(-2, 3, (C,), generator=g).to(F64)}


def exact_dgrad_case(shape, seed=0, add=None, bn_mode=None):
    """dy, w integers; add: None | "plain" | "bits" | "sub2". bn_mode 0/2/3: also y (the BN's pre-norm
    input, even integers so that xhat = (y - mean) invstd is an integer), its constants, relu bits and
    the statistics partials. Exactness: sum |dy||w| + |add| < 2^24; sum |d xhat| < 2^24 per channel."""
    N, H, W, C, K, R, st, pad = shape
    Ho, Wo = out_hw(H, W, R, R, st, pad)
    for amp, dens in _LADDER:
        g = torch.Generator().manual_seed(seed + 1)
        dy = _ints(g, (N, Ho, Wo, K), amp, dens)
        w = _ints(g, (R, R, C, K), amp, 1.0)
        case = {"dy": dy, "w": w, "add": None, "bits": None, "sub2": add == "sub2"}
        if add is not None:
            ashape = (N, (H + 1) // 2, (W + 1) // 2, C) if add == "sub2" else (N, H, W, C)
            case["add"] = _ints(g, ashape, 3 * amp, 1.0)
            if add == "bits":
                case["bits"] = pack_bits(torch.rand(N * H * W, C, generator=g) < 0.5)
        dxa = conv_dgrad(dy.abs(), w.abs(), (N, H, W, C), st, pad,
                         None if case["add"] is None else case["add"].abs(), case["bits"], case["sub2"])
        if float(dxa.max()) >= EXACT_LIMIT:
            continue
        dx = conv_dgrad(dy, w, (N, H, W, C), st, pad, case["add"], case["bits"], case["sub2"])
        case["dx"] = dx
        if bn_mode is not None:
            case.update(_bn_consts(g, C, True))
            case["y"] = 2 * _ints(g, (N, H, W, C), 4, 1.0)
            case["mask_bits"] = pack_bits(torch.rand(N * H * W, C, generator=g) < 0.5) if bn_mode == 3 else None
            mask = bn_mask(bn_mode, case["y"], case["mean"], case["invstd"], case["gamma"], case["beta"], case["mask_bits"])
            case["mask"] = mask
            d = bf16_rne(dx).reshape(-1, C).abs() * mask.to(F64)
            xh = ((case["y"].reshape(-1, C) - case["mean"]) * case["invstd"]).abs()
            if float((d * xh).sum(0).max()) >= EXACT_LIMIT or float(d.sum(0).max()) >= EXACT_LIMIT:
                continue
            assert_exact((d * xh).sum(0), d.sum(0))
            case["stats"] = dgrad_bn_stats(dx, case["y"], case["mean"], case["invstd"], mask)
        assert_exact(dxa)
        return case
    raise AssertionError(f"no exact rung for {shape}")


def exact_wgrad_case(shape, seed=0, fold=False):
    """x, dy integers, dw exact: sum over the N Ho Wo pixels of |x||dy| < 2^24."""
    N, H, W, C, K, R, st, pad = shape
    Ho, Wo = out_hw(H, W, R, R, st, pad)
    for amp, dens in _LADDER:
        g = torch.Generator().manual_seed(seed + 2)
        x = _ints(g, (N, H, W, C), amp, dens)
        dy = _ints(g, (N, Ho, Wo, K), amp, 1.0)
        case = {"x": x, "dy": dy}
        xin = x
        if fold:
            case.update(_bn_consts(g, C, False))
            xin = bn_relu_in(x, case["mean"], case["invstd"], case["gamma"], case["beta"])
        case["xin"] = xin
        dwa = conv_wgrad(xin.abs(), dy.abs(), R, R, st, pad)
        if float(dwa.max()) >= EXACT_LIMIT:
            continue
        assert_exact(dwa)
        case["dw"] = conv_wgrad(xin, dy, R, R, st, pad)
        return case
    raise AssertionError(f"no exact rung for {shape}")


def exact_gemm_case(M, Kin, N, seed=0):
    """Integer x [M, Kin], w [Kin, N], dy [M, N], bias [N] with every product sum below 2^24."""
    for amp, _ in _LADDER:
        g = torch.Generator().manual_seed(seed + 3)
        x, w, dy = _ints(g, (M, Kin), amp, 1.0), _ints(g, (Kin, N), amp, 1.0), _ints(g, (M, N), amp, 1.0)
        b = _ints(g, (N,), 50, 1.0)
        big = max(float((x.abs() @ w.abs()).max()) + 50, float((dy.abs() @ w.abs().t()).max()),
                  float((x.abs().t() @ dy.abs()).max()))
        if big < EXACT_LIMIT:
            assert_exact(x.abs() @ w.abs() + 50, dy.abs() @ w.abs().t(), x.abs().t() @ dy.abs())
            return {"x": x, "w": w, "dy": dy, "b": b}
    raise AssertionError("no exact rung")


def tie_count(exact):
    """How many exact values lie beyond 256 on a bf16 tie (halfway between two bf16 numbers)."""
    dn = bf16_trunc(exact)
    step = 2.0 ** (torch.floor(torch.log2(exact.abs().clamp_min(1))) - 7)
    return int(((exact.abs() > 256) & ((exact - dn).abs() == step / 2)).sum())


# ---------------------------------------------------------------- random cases and the derived bound
def rb(t):
    return t.to(torch.bfloat16).to(F64)


def randn_bf16(g, shape, scale=1.0):
    return rb(torch.randn(shape, generator=g) * scale)


def err_e(L, A):
    """e = L 2^-23 A: fp32 accumulation of L terms whose absolute values sum to A (module docstring)."""
    return L * 2.0 ** -23 * A


def bound_f32(L, A):
    return err_e(L, A)


def bound_bf16(ref, L, A):
    e = err_e(L, A)
    return 2.0 ** -8 * (ref.abs() + e) + e


# ---------------------------------------------------------------- the checker
def layout_nhwc(N, H, W, C, stride=1, name="out-channel"):
    """Slicings of an [N,H,W,C] tensor (a conv output, or a dgrad's dx): channel 8- and 64-chunks,
    64/128/256-row M tiles, image, border against interior, stride phase, 8x16 halo tile."""
    n, h, w, c = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    m = (n * H + h) * W + w
    lay = {f"{name} 8-chunk": (c // 8, lambda i: f"channels {8 * i}..{8 * i + 7}"),
           f"{name} 64-chunk": (c // 64, lambda i: f"channels {64 * i}..{64 * i + 63}"),
           "image": (n, lambda i: f"image {i}")}
    for t in (64, 128, 256):
        lay[f"m_tile{t}"] = (m // t, lambda i, t=t: f"rows {i * t}..{min(N * H * W, (i + 1) * t) - 1}")
    border = (h == 0) * 1 + (h == H - 1) * 2 + (w == 0) * 4 + (w == W - 1) * 8
    lay["border"] = (border, lambda i: "interior" if i == 0 else "+".join(
        nm for b, nm in ((1, "top row"), (2, "bottom row"), (4, "left column"), (8, "right column")) if i & b))
    if stride > 1:
        lay["phase"] = ((h % stride) * stride + (w % stride), lambda i: f"phase (h%{stride}, w%{stride}) = ({i // stride}, {i % stride})")
    tw = (W + 15) // 16
    lay["halo tile"] = ((h // 8) * tw + (w // 16), lambda i: f"tile (h/8, w/16) = ({i // tw}, {i % tw})")
    return lay


def layout_hwio(R, S, C, K):
    """Slicings of a filter gradient [R,S,C,K]: tap, input-channel 8/64-chunk, output-channel 8-chunk."""
    r, s, c, k = torch.meshgrid(torch.arange(R), torch.arange(S), torch.arange(C), torch.arange(K), indexing="ij")
    return {"tap": (r * S + s, lambda i: f"tap (r, s) = ({i // S}, {i % S})"),
            "in-channel 8-chunk": (c // 8, lambda i: f"in channels {8 * i}..{8 * i + 7}"),
            "in-channel 64-chunk": (c // 64, lambda i: f"in channels {64 * i}..{64 * i + 63}"),
            "out-channel 8-chunk": (k // 8, lambda i: f"out channels {8 * i}..{8 * i + 7}")}


def layout_rows(M, C, name="channel"):
    """Slicings of a plain [M, C] matrix (dense layers, BN, statistics rows)."""
    m, c = torch.meshgrid(torch.arange(M), torch.arange(C), indexing="ij")
    lay = {f"{name} 8-chunk": (c // 8, lambda i: f"channels {8 * i}..{8 * i + 7}"),
           f"{name} 64-chunk": (c // 64, lambda i: f"channels {64 * i}..{64 * i + 63}")}
    for t in (64, 128, 256):
        lay[f"m_tile{t}"] = (m // t, lambda i, t=t: f"rows {i * t}..{min(M, (i + 1) * t) - 1}")
    return lay


def layout_stats(C):
    """Slicings of the summed statistics partials [2, C]."""
    r, c = torch.meshgrid(torch.arange(2), torch.arange(C), indexing="ij")
    return {"statistic": (r, lambda i: ("sum a", "sum b")[i]), "channel 8-chunk": (c // 8, lambda i: f"channels {8 * i}..{8 * i + 7}"),
            "channel 64-chunk": (c // 64, lambda i: f"channels {64 * i}..{64 * i + 63}")}


def layout_vec(C):
    c = torch.arange(C)
    return {"channel": (c, lambda i: f"channel {i}"), "channel 8-chunk": (c // 8, lambda i: f"channels {8 * i}..{8 * i + 7}")}


class Mismatch(AssertionError):
    """report: {slicing: [(slice name, bad count, slice size, worst |err|), ...]} (bad slices only)."""

    def __init__(self, msg, report):
        super().__init__(msg)
        self.report = report

    def names(self, slicing):
        return [r[0] for r in self.report.get(slicing, [])]

    def only(self, slicing):
        """The name of the single bad slice of a slicing (None when several or none are bad)."""
        n = self.names(slicing)
        return n[0] if len(n) == 1 else None


def slice_report(got, ref, bound, layout):
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    bad = err > (bound if torch.is_tensor(bound) else float(bound))
    rep = {}
    if not bad.any():
        return bad, err, rep, {}
    layout = layout() if callable(layout) else (layout or {})  # built only when there is something to report
    for name, (idx, label) in layout.items():
        idx = idx.reshape(-1).long()
        n = int(idx.max()) + 1
        cnt = torch.bincount(idx, weights=bad.reshape(-1).to(F64), minlength=n)
        size = torch.bincount(idx, minlength=n)
        worst = torch.zeros(n, dtype=F64).scatter_reduce(0, idx, torch.where(bad, err, torch.zeros_like(err)).reshape(-1),
                                                         "amax", include_self=True)
        rep[name] = [(label(i), int(cnt[i]), int(size[i]), float(worst[i])) for i in range(n) if cnt[i] > 0]
    return bad, err, rep, layout


def check(got, ref, bound, layout, what="tensor"):
    """Assert |got - ref| <= bound for every element (bound 0: equality; a non-finite got always
    fails). On failure the Mismatch names where the bad elements lie, per slicing of ``layout`` --
    reporting only, no slice gets a tolerance of its own."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    bad, err, rep, layout = slice_report(got, ref, bound, layout)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    i = int(torch.where(bad.reshape(-1), err.reshape(-1), torch.zeros(1, dtype=F64)).argmax())
    at = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
    lines = [f"{what}: {nbad} of {bad.numel()} elements beyond the bound; worst |err| {float(err.reshape(-1)[i]):.6g} at {at} "
             f"(got {float(got.reshape(-1)[i]):.9g}, want {float(ref.reshape(-1)[i]):.9g})"]
    for name, rows in rep.items():
        total = int(layout[name][0].max()) + 1
        head = f"  {name}: {len(rows)} of {total} slices bad"
        shown = sorted(rows, key=lambda r: -r[1])[:6]
        lines.append(head + ": " + "; ".join(f"{n} ({c}/{s}, worst {w:.4g})" for n, c, s, w in shown)
                     + (" ..." if len(rows) > 6 else ""))
    raise Mismatch("\n".join(lines), rep)


def check_bf16_exact(got, exact, layout, what="tensor"):
    check(got, bf16_rne(exact), 0.0, layout, what)


# taps of a weight gradient or a forward output cannot be told apart in the output itself; for an
# output-side mismatch the tap is found by which single-tap correction explains it
def blame_tap(got, x, w, st, pad, ref):
    """Which tap's contribution, scaled, best explains got - ref of a conv forward: returns
    ((r, s), residual norm ratio). Used to name a tap for an output-side error."""
    R, S = w.shape[:2]
    diff = (got.to(F64) - ref).reshape(-1)
    best = None
    for r, s in itertools.product(range(R), range(S)):
        wt = torch.zeros_like(w, dtype=F64)
        wt[r, s] = w[r, s].to(F64)
        t = conv_fwd(x, wt, st, pad).reshape(-1)
        a = float(diff @ t) / max(float(t @ t), 1e-300)
        res = float((diff - a * t).norm()) / max(float(diff.norm()), 1e-300)
        if best is None or res < best[1]:
            best = ((r, s), res, a)
    return best


# ================================================================ shape tables of the GPU test
# (N, H, W, C, K, R, stride, pad): the smallest shapes that reach each tile path with a ragged tail
T64 = [(2, 9, 7, 16, 24, 3, 1, 1), (1, 5, 13, 8, 72, 3, 1, 1), (3, 8, 8, 40, 16, 1, 1, 0)]
# 128x64 tiles: K = 64 and ceil(M / 128) >= 256 (M = 32761, last tile 121 rows)
T128x64 = [(1, 181, 181, 8, 64, 3, 1, 1), (1, 181, 181, 16, 64, 1, 1, 0)]
# 128x128 tiles: width >= 128 and >= 256 tiles; the second has ragged M (16383) and ragged N (136)
T128 = [(1, 181, 181, 8, 128, 3, 1, 1), (1, 127, 129, 8, 136, 1, 1, 0)]
G256_WIDTHS = [64, 72, 128, 136, 256, 264]  # g256_bn 64 / 128 / 256, each with a ragged N tail
G256_MAPS = [(1, 15, 17, 3, 1), (1, 1, 257, 1, 0), (1, 25, 40, 3, 1)]  # (N, H, W, R, pad): M = 255, 257, 1000
HALO = [(1, 3, 5, 64, 64, 3, 1, 1), (2, 9, 23, 192, 64, 3, 1, 1), (3, 7, 7, 128, 64, 3, 1, 1), (2, 20, 36, 64, 128, 3, 1, 1)]
STRIDED = [(2, 11, 8, 16, 24, 3, 2, 1), (2, 12, 12, 8, 16, 3, 2, 0), (1, 7, 9, 8, 8, 3, 3, 1), (2, 9, 9, 16, 32, 1, 2, 0),
           (2, 16, 16, 8, 16, 7, 2, 3)]
WGRAD = [(2, 9, 7, 8, 24, 3, 1, 1), (4, 23, 25, 16, 72, 3, 1, 1), (8, 24, 24, 16, 128, 3, 1, 1), (4, 23, 25, 16, 128, 3, 1, 1),
         (2, 24, 48, 64, 64, 1, 1, 0), (2, 11, 8, 16, 24, 3, 2, 1)]
STEM = [(2, 32, 30, 64), (3, 23, 16, 16)]  # N, H, W, K (7x7, stride 2, pad 3, 3 input channels)
LINEAR = [(1, 8, 8), (24, 64, 40), (130, 72, 136), (257, 1152, 264)]  # M, Kin, N
GEMM_NT = [(256, 256, 64), (300, 264, 72), (1000, 520, 1032), (513, 2048, 576)]  # M, N, K
FOLD = [(2, 9, 7, 16, 24, 3, 1, 1), (2, 10, 10, 16, 32, 3, 2, 1), (3, 8, 8, 40, 16, 1, 1, 0)]
POOLS = [(2, 16, 16, 64, 3, 2, 1), (3, 15, 13, 32, 3, 2, 1), (2, 9, 11, 16, 2, 2, 0), (2, 10, 10, 8, 3, 3, 1), (2, 8, 8, 16, 3, 1, 1),
         (2, 2, 2, 8, 3, 2, 1), (1, 1, 5, 8, 3, 2, 1), (2, 3, 1, 16, 3, 1, 1)]  # N, H, W, C, k, stride, pad; the last three: H or W < k
BN_SHAPES = [(1, 8), (5, 24), (33, 8), (300, 64), (300, 520), (64, 2048)]  # M, C
XENT = [(1, 8), (5, 8), (1, 10), (5, 10), (1, 1000), (5, 1000), (1, 1001), (5, 1001)]  # N, K
MAX_L = 1152


def swap_ck(shape):
    """The same map with C and K swapped: the dgrad tile chooser looks at C."""
    N, H, W, C, K, R, st, pad = shape
    return (N, H, W, K, C, R, st, pad)


def g256_shapes(dgrad=False):
    out = []
    for wd in G256_WIDTHS:
        for N, H, W, R, pad in G256_MAPS:
            out.append((N, H, W, wd, 8, R, 1, pad) if dgrad else (N, H, W, 8, wd, R, 1, pad))
    return out


FWD_SHAPES = T64 + T128x64 + T128 + HALO + STRIDED + g256_shapes()
DGRAD_SHAPES = T64 + [swap_ck(s) for s in T128x64 + T128] + HALO + STRIDED + g256_shapes(True)
# dgrad + BN-backward partials: stride-1 pointwise, stride-1 3x3 (gather, halo), stride-2 3x3, the big tiles
DGRAD_BN_SHAPES = [T64[2], T64[0], HALO[2], STRIDED[0], STRIDED[1], swap_ck(T128x64[0]), swap_ck(T128[1]),
                   (1, 15, 17, 136, 8, 3, 1, 1)]


def dgrad_adds(shape):
    """The add forms a dgrad shape takes: relu bits need stride 1; the stride-2 operand sits on the even
    pixels of a stride-1 or stride-2 dgrad whose even phase has taps."""
    st, pad = shape[6], shape[7]
    adds = [None, "plain"]
    if st == 1:
        adds.append("bits")
    if st == 1 or (st == 2 and (shape[5] >= 2 or pad % 2 == 0)):
        adds.append("sub2")
    return adds


def conv_L(shape, op):
    N, H, W, C, K, R, st, pad = shape
    Ho, Wo = out_hw(H, W, R, R, st, pad)
    return {"fwd": R * R * C, "dgrad": R * R * K, "wgrad": N * Ho * Wo}[op]


# the random family runs where the reduction length stays within MAX_L (e stays well under a bf16
# half-ulp): that leaves out the forward of the 192-channel halo shape (L = 1728) and the weight
# gradient of the 20x36 one (L = 1440); the exact family covers both
RANDOM_SHAPES = T64 + HALO
RANDOM_CASES = [(s, op) for s in RANDOM_SHAPES for op in ("fwd", "dgrad", "wgrad") if conv_L(s, op) <= MAX_L]


# ================================================================ runs on the device
# Every run_* returns a list of (what, got, ref, bound, layout): what check() takes. The GPU test
# asserts each; tools/conv_oracle_rel.py counts mismatches / records |got - ref| / bound.
def _exact_bf16(t):
    b = t.to(torch.bfloat16)
    assert torch.equal(b.to(F64), t.to(F64)), "operand is not exactly a bf16 number"
    return b


def _dev(t, dev):
    return None if t is None else _exact_bf16(t).to(dev)


def _f32(t, dev):
    return t.to(torch.float32).to(dev)


_CASES = {}


def cached(fn, *key, **kw):
    """Exact and random cases are generated once per process and left unchanged."""
    k = (fn.__name__, key, tuple(sorted(kw.items())))
    if k not in _CASES:
        c = fn(*key, **kw)
        # the large exact results are kept as their bf16 rounding (what the test compares with)
        for name in (("y",) if fn is exact_fwd_case else ("dx",) if fn is exact_dgrad_case else ()):
            if c[name].numel() > (1 << 20):
                c[name + "_ties"] = tie_count(c[name])
                c[name + "_ref"] = bf16_rne(c[name]).to(torch.bfloat16)
                del c[name]
        _CASES[k] = c
    return _CASES[k]


def _ref_bf16(case, name):
    return case[name + "_ref"].to(F64) if name + "_ref" in case else bf16_rne(case[name])


def _nhwc(shape4, stride=1, name="out-channel"):
    return lambda: layout_nhwc(*shape4, stride=stride, name=name)


def run_fwd_exact(ops, dev, shape):
    N, H, W, C, K, R, st, pad = shape
    c = cached(exact_fwd_case, shape)
    y = ops.conv2d_fwd(_dev(c["x"], dev), _dev(c["w"], dev), st, pad)
    return [(f"conv2d_fwd {shape}", y, _ref_bf16(c, "y"), 0.0, _nhwc(y.shape))]


def run_fwd_stats_exact(ops, dev, shape):
    N, H, W, C, K, R, st, pad = shape
    c = cached(exact_fwd_case, shape, stats=True)
    x, w = _dev(c["x"], dev), _dev(c["w"], dev)
    y0 = ops.conv2d_fwd(x, w, st, pad)
    y, part = ops.conv2d_fwd_stats(x, w, st, pad)
    ref = _ref_bf16(c, "y")
    return [(f"conv2d_fwd_stats y {shape}", y, ref, 0.0, _nhwc(y.shape)),
            (f"conv2d_fwd_stats y against conv2d_fwd {shape}", y, y0.cpu().to(F64), 0.0, _nhwc(y.shape)),
            (f"conv2d_fwd_stats partials {shape}", part.sum(0), c["stats"], 0.0, lambda: layout_stats(K))]


def run_dgrad_exact(ops, dev, shape, add):
    N, H, W, C, K, R, st, pad = shape
    c = cached(exact_dgrad_case, shape, add=add)
    bits = None if c["bits"] is None else c["bits"].to(dev)
    dx = ops.conv2d_dgrad(_dev(c["dy"], dev), _dev(c["w"], dev), [N, H, W, C], st, pad, _dev(c["add"], dev), bits, c["sub2"])
    return [(f"conv2d_dgrad add={add} {shape}", dx, _ref_bf16(c, "dx"), 0.0, _nhwc((N, H, W, C), st, "in-channel"))]


def run_dgrad_bn_exact(ops, dev, shape, mode, add):
    N, H, W, C, K, R, st, pad = shape
    c = cached(exact_dgrad_case, shape, add=add, bn_mode=mode)
    bits = None if c["bits"] is None else c["bits"].to(dev)
    y = _dev(c["y"], dev)
    mean, invstd, gamma, beta = (_f32(c[k], dev) for k in ("mean", "invstd", "gamma", "beta"))
    mb = None if c["mask_bits"] is None else c["mask_bits"].to(dev)
    dx, part = ops.conv2d_dgrad_bn(_dev(c["dy"], dev), _dev(c["w"], dev), [N, H, W, C], st, pad, _dev(c["add"], dev), y, mean,
                                   invstd, gamma, beta if mode == 2 else None, mb, mode != 0, bits, None, c["sub2"])
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ops.bn_bwd(dx, torch.empty_like(dx), y, gamma, mean, invstd, mode != 0, False, dg, db, beta if mode == 2 else None, mb, part)
    tag = f"mode={mode} add={add} {shape}"
    return [(f"conv2d_dgrad_bn dx {tag}", dx, _ref_bf16(c, "dx"), 0.0, _nhwc((N, H, W, C), st, "in-channel")),
            (f"conv2d_dgrad_bn partials {tag}", part.sum(0), c["stats"], 0.0, lambda: layout_stats(C)),
            (f"bn_bwd(partials) dbeta {tag}", db, c["stats"][0], 0.0, lambda: layout_vec(C)),
            (f"bn_bwd(partials) dgamma {tag}", dg, c["stats"][1], 0.0, lambda: layout_vec(C))]


def run_wgrad_exact(ops, dev, shape, zeroed):
    N, H, W, C, K, R, st, pad = shape
    c = cached(exact_wgrad_case, shape)
    # zeroed: the caller's zero buffer; else the op must overwrite whatever is there
    dw = torch.zeros(R, R, C, K, device=dev) if zeroed else torch.full((R, R, C, K), 7.0, device=dev)
    ops.conv2d_wgrad(_dev(c["x"], dev), _dev(c["dy"], dev), dw, st, pad, zeroed)
    return [(f"conv2d_wgrad zeroed={zeroed} {shape}", dw, c["dw"], 0.0, lambda: layout_hwio(R, R, C, K))]


def run_fold_exact(ops, dev, shape):
    """The folded-BN-input forms against the oracle itself (integer mean / beta, power-of-two invstd /
    gamma): forward, forward + statistics, weight gradient."""
    N, H, W, C, K, R, st, pad = shape
    c = cached(exact_fwd_case, shape, stats=True, fold=True)
    act = [_f32(c[k], dev) for k in ("mean", "invstd", "gamma", "beta")]
    x, w = _dev(c["x"], dev), _dev(c["w"], dev)
    y = ops.conv2d_fwd(x, w, st, pad, *act)
    y2, part = ops.conv2d_fwd_stats(x, w, st, pad, *act)
    ref = _ref_bf16(c, "y")
    out = [(f"conv2d_fwd folded {shape}", y, ref, 0.0, _nhwc(y.shape)),
           (f"conv2d_fwd_stats folded y {shape}", y2, ref, 0.0, _nhwc(y.shape)),
           (f"conv2d_fwd_stats folded partials {shape}", part.sum(0), c["stats"], 0.0, lambda: layout_stats(K))]
    cw = cached(exact_wgrad_case, shape, fold=True)
    actw = [_f32(cw[k], dev) for k in ("mean", "invstd", "gamma", "beta")]
    dw = torch.zeros(R, R, C, K, device=dev)
    ops.conv2d_wgrad(_dev(cw["x"], dev), _dev(cw["dy"], dev), dw, st, pad, True, *actw)
    out.append((f"conv2d_wgrad folded {shape}", dw, cw["dw"], 0.0, lambda: layout_hwio(R, R, C, K)))
    return out


def exact_stem_case(N, H, W, K, seed=0):
    g = torch.Generator().manual_seed(seed + 4)
    x = _ints(g, (N, H, W, 3), 2, 1.0)
    w = _ints(g, (7, 7, 8, K), 2, 1.0)
    w[:, :, 3:] = 0
    xpad = torch.zeros(N, H, W, 8, dtype=F64)
    xpad[..., :3] = x
    y = conv_fwd(xpad, w, 2, 3)
    dy = _ints(g, tuple(y.shape), 3, 1.0)
    stats = fwd_stats(y)
    dw = conv_wgrad(xpad, dy, 7, 7, 2, 3)
    assert_exact(conv_fwd(xpad.abs(), w.abs(), 2, 3), stats[1], conv_wgrad(xpad.abs(), dy.abs(), 7, 7, 2, 3))
    return {"x": x, "w": w, "y": y, "dy": dy, "stats": stats, "dw": dw}


def run_stem_exact(ops, dev, shape):
    from tensorflow_distributed_amd.models.resnet import pair_stem_weight, unpair_stem_grad
    N, H, W, K = shape
    c = cached(exact_stem_case, N, H, W, K)
    xp = ops.stem_pack(_f32(c["x"], dev))
    pk = torch.zeros(N, H, W // 2, 8, dtype=F64)
    pk[..., :6] = c["x"].reshape(N, H, W // 2, 6)
    w = _dev(c["w"], dev)
    y, part = ops.conv2d_fwd_stats_w2(xp, pair_stem_weight(w), 2, 3)
    dwp = torch.full((7, 4, 8, K), 7.0, device=dev)
    ops.conv2d_wgrad_w2(xp, _dev(c["dy"], dev), dwp, 2, 3, False)
    dw = torch.full((7, 7, 8, K), float("nan"), device=dev)
    unpair_stem_grad(dwp, dw)
    return [(f"stem_pack {shape}", xp, pk, 0.0, _nhwc(pk.shape)),
            (f"conv2d_fwd_stats_w2 y {shape}", y, bf16_rne(c["y"]), 0.0, _nhwc(c["y"].shape)),
            (f"conv2d_fwd_stats_w2 partials {shape}", part.sum(0), c["stats"], 0.0, lambda: layout_stats(K)),
            (f"conv2d_wgrad_w2 {shape}", dw, c["dw"], 0.0, lambda: layout_hwio(7, 7, 8, K))]


def run_linear_exact(ops, dev, shape):
    M, Kin, N = shape
    c = cached(exact_gemm_case, M, Kin, N)
    x, w, dy = _dev(c["x"], dev), _dev(c["w"], dev), _dev(c["dy"], dev)
    y = ops.linear_fwd(x, w, _f32(c["b"], dev))
    y0 = ops.linear_fwd(x, w, None)
    dx = ops.linear_dgrad(dy, w)
    dw = torch.full((Kin, N), 7.0, device=dev)
    ops.linear_wgrad(x, dy, dw)
    return [(f"linear_fwd {shape}", y, linear_fwd(c["x"], c["w"], c["b"]), 0.0, lambda: layout_rows(M, N)),
            (f"linear_fwd no bias {shape}", y0, linear_fwd(c["x"], c["w"]), 0.0, lambda: layout_rows(M, N)),
            (f"linear_dgrad {shape}", dx, bf16_rne(linear_dgrad(c["dy"], c["w"])), 0.0, lambda: layout_rows(M, Kin)),
            (f"linear_wgrad {shape}", dw, linear_wgrad(c["x"], c["dy"]), 0.0, lambda: layout_rows(Kin, N))]


def run_gemm_nt_exact(ops, dev, shape):
    M, N, K = shape
    c = cached(exact_gemm_case, M, K, N)
    got = ops.gemm_nt(_dev(c["x"], dev), _dev(c["w"].t().contiguous(), dev))
    return [(f"gemm_nt {shape}", got, bf16_rne(linear_fwd(c["x"], c["w"])), 0.0, lambda: layout_rows(M, N))]


def tie_pool_input(N, H, W, C, seed=0):
    """Integers in -2..2: nearly every window holds its maximum several times."""
    return _ints(torch.Generator().manual_seed(seed + 5), (N, H, W, C), 2, 1.0)


def run_maxpool_exact(ops, dev, shape):
    N, H, W, C, k, st, pad = shape
    x = cached(tie_pool_input, N, H, W, C)
    y, am = maxpool_fwd(x, k, st, pad)
    dy = _ints(torch.Generator().manual_seed(6), tuple(y.shape), 9, 1.0)
    gy, gam = ops.maxpool2d_fwd(_dev(x, dev), k, st, pad)
    gdx = ops.maxpool2d_bwd(_dev(dy, dev), gam, [N, H, W, C], k, st, pad)
    return [(f"maxpool2d_fwd {shape}", gy, y, 0.0, _nhwc(y.shape, name="channel")),
            (f"maxpool2d_fwd argmax {shape}", gam, am.to(F64), 0.0, _nhwc(y.shape, name="channel")),
            (f"maxpool2d_bwd {shape}", gdx, bf16_rne(maxpool_bwd(dy, am, (N, H, W, C), k, st, pad)), 0.0,
             _nhwc((N, H, W, C), name="channel"))]


# ---------------------------------------------------------------- random family
def random_conv_case(shape, seed=0):
    N, H, W, C, K, R, st, pad = shape
    Ho, Wo = out_hw(H, W, R, R, st, pad)
    g = torch.Generator().manual_seed(seed + 7)
    x, w = randn_bf16(g, (N, H, W, C)), randn_bf16(g, (R, R, C, K), 0.2)
    dy, add = randn_bf16(g, (N, Ho, Wo, K)), randn_bf16(g, (N, H, W, C))
    c = {"x": x, "w": w, "dy": dy, "add": add}
    xs = (N, H, W, C)
    c["y"], c["yA"] = conv_fwd(x, w, st, pad), conv_fwd(x.abs(), w.abs(), st, pad)
    c["dx"], c["dxA"] = conv_dgrad(dy, w, xs, st, pad), conv_dgrad(dy.abs(), w.abs(), xs, st, pad)
    c["dw"], c["dwA"] = conv_wgrad(x, dy, R, R, st, pad), conv_wgrad(x.abs(), dy.abs(), R, R, st, pad)
    return c


def run_conv_random(ops, dev, shape, op):
    N, H, W, C, K, R, st, pad = shape
    c = cached(random_conv_case, shape)
    L = conv_L(shape, op)
    assert L <= MAX_L
    x, w, dy = _dev(c["x"], dev), _dev(c["w"], dev), _dev(c["dy"], dev)
    if op == "fwd":
        y = ops.conv2d_fwd(x, w, st, pad)
        return [(f"random conv2d_fwd {shape}", y, c["y"], bound_bf16(c["y"], L, c["yA"]), _nhwc(y.shape))]
    if op == "dgrad":
        lay = _nhwc((N, H, W, C), st, "in-channel")
        dx = ops.conv2d_dgrad(dy, w, [N, H, W, C], st, pad)
        dx2 = ops.conv2d_dgrad(dy, w, [N, H, W, C], st, pad, _dev(c["add"], dev))
        ref2 = c["dx"] + c["add"]
        return [(f"random conv2d_dgrad {shape}", dx, c["dx"], bound_bf16(c["dx"], L, c["dxA"]), lay),
                (f"random conv2d_dgrad + add {shape}", dx2, ref2, bound_bf16(ref2, L + 1, c["dxA"] + c["add"].abs()), lay)]
    dw = torch.zeros(R, R, C, K, device=dev)
    ops.conv2d_wgrad(x, dy, dw, st, pad, True)
    return [(f"random conv2d_wgrad {shape}", dw, c["dw"], bound_f32(L, c["dwA"]), lambda: layout_hwio(R, R, C, K))]


# Batch norm. u = 2^-24. Forward (bn_final / the inline finalize, then bn_apply):
#   S1 = sum y, S2 = sum y^2 (y^2 of a bf16 is exact in fp32) over M rows in fp32, any order:
#     |dS1| <= g A1, |dS2| <= g S2 with A1 = sum |y| and g = 2 M u (the module docstring's L 2^-23)
#   mean = S1 / M:                    dm   <= g A1 / M + u |mean|
#   var  = S2 / M - mean^2:           dvar <= (g + 2u) S2 / M + 2 |mean| dm + 2u mean^2 + u |var|
#   invstd = rsqrt(var + eps), the hardware rsqrt within 1 ulp (2u) plus the add's rounding:
#                                     dis  <= invstd (dvar / (2 (var + eps)) + 4u)
#   sc = invstd gamma:                dsc  <= |gamma| dis + u |sc|
#   sh = fma(-mean, sc, beta), z = fma(y, sc, sh) [+ res]: with z = (y - mean) sc + beta,
#     z^ - z = (y - mean)(sc^ - sc) - (mean^ - mean) sc^ + roundings of sh, z (and the residual add)
#                                     ez   <= |y - mean| dsc + (|sc| + dsc) dm + u (|sh| + 2 |z| + |z + res|)
#   relu is 1-Lipschitz; then one bf16 rounding: 2^-8 (|ref| + ez) + ez.
def bn_fwd_bound(y, gamma, beta, res, eps):
    C = y.shape[-1]
    y2 = y.to(F64).reshape(-1, C)
    M = y2.shape[0]
    g = 2 * M * U
    mean, S2 = y2.mean(0), (y2 * y2).sum(0)
    var = ((y2 - mean) ** 2).mean(0)
    dm = g * y2.abs().sum(0) / M + U * mean.abs()
    dvar = (g + 2 * U) * S2 / M + 2 * mean.abs() * dm + 2 * U * mean * mean + U * var
    invstd = 1 / torch.sqrt(var + eps)
    dis = invstd * (dvar / (2 * (var + eps)) + 4 * U)
    sc = invstd * gamma.to(F64)
    dsc = gamma.to(F64).abs() * dis + U * sc.abs()
    sh = beta.to(F64) - mean * sc
    z = (y2 - mean) * sc + beta.to(F64)
    zr = z if res is None else z + res.to(F64).reshape(-1, C)
    ez = (y2 - mean).abs() * dsc + (sc.abs() + dsc) * dm + U * (sh.abs() + 2 * z.abs() + zr.abs())
    return {"mean": dm, "var": dvar, "invstd": dis, "ez": ez.reshape(y.shape)}


# Backward, from the SAME fp32 mean / invstd the kernel is given (no statistics error to propagate):
#   dbeta = sum dz, dgamma = sum dz xhat, xhat = (y - mean) invstd in fp32 (2 roundings), fma'd:
#     ddb <= g sum |dz|, ddg <= (g + 3u) sum |dz xhat|, g = 2 M u
#   dy = k1 dz + k2 y + k3, k1 = gamma invstd, k2 = -k1 invstd dgamma / M, k3 = -k1 (dbeta / M - mean invstd dgamma / M)
#     dk1 <= u |k1|;  dk2 <= 5u |k2| + |k1 invstd / M| ddg
#     a = dbeta / M (1 / M rounded, one product), b = mean invstd dgamma / M:
#       da <= 3u |a| + ddb / M, db_ <= 4u |b| + |mean invstd / M| ddg
#     dk3 <= |k1| (da + db_ + u |a - b|) + 2u |k3|
#   two fmas: e <= |dz| dk1 + |y| dk2 + dk3 + u (|k2 y + k3| + |dy|); then one bf16 rounding.
def bn_bwd_bound(dz, y, gamma, mean, invstd):
    C = y.shape[-1]
    y2, dz = y.to(F64).reshape(-1, C), dz.to(F64).reshape(-1, C)
    M = y2.shape[0]
    g = 2 * M * U
    mean, invstd, gamma = mean.to(F64), invstd.to(F64), gamma.to(F64)
    xhat = (y2 - mean) * invstd
    db, dg = dz.sum(0), (dz * xhat).sum(0)
    ddb, ddg = g * dz.abs().sum(0), (g + 3 * U) * (dz * xhat).abs().sum(0)
    k1 = gamma * invstd
    k2 = -k1 * invstd * dg / M
    a, b = db / M, mean * invstd * dg / M
    k3 = -k1 * (a - b)
    dk1 = U * k1.abs()
    dk2 = 5 * U * k2.abs() + (k1 * invstd / M).abs() * ddg
    da, db_ = 3 * U * a.abs() + ddb / M, 4 * U * b.abs() + (mean * invstd / M).abs() * ddg
    dk3 = k1.abs() * (da + db_ + U * (a - b).abs()) + 2 * U * k3.abs()
    dy = k1 * dz + k2 * y2 + k3
    e = dz.abs() * dk1 + y2.abs() * dk2 + dk3 + U * ((k2 * y2 + k3).abs() + dy.abs())
    return {"dbeta": ddb, "dgamma": ddg, "e": e.reshape(y.shape)}


def random_bn_case(M, C, seed=0):
    g = torch.Generator().manual_seed(seed + 8 + M + C)
    return {"y": rb(torch.randn((M, C), generator=g) * 3 + 1), "res": randn_bf16(g, (M, C)), "dout": randn_bf16(g, (M, C)),
            "gamma": (torch.rand(C, generator=g) + 0.5).to(torch.float32), "beta": torch.randn(C, generator=g).to(torch.float32),
            "rm": torch.randn(C, generator=g).to(torch.float32), "rv": (torch.rand(C, generator=g) + 0.5).to(torch.float32)}


def _with_bf16(ref, e):
    return 2.0 ** -8 * (ref.abs() + e) + e


def run_bn_random(ops, dev, M, C, relu, res, src):
    """src: the backward's mask source -- "out" (the forward's output), "y" (recomputed, beta given;
    residual-free only), "bits" (the forward's relu bits)."""
    c = cached(random_bn_case, M, C)
    eps, mom = 1e-5, 0.9
    y, gamma, beta = c["y"], c["gamma"], c["beta"]
    r = c["res"] if res else None
    yd, gd, bd = _dev(y, dev), gamma.to(dev), beta.to(dev)
    rd = _dev(r, dev) if res else None
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    bits = torch.empty(M, C // 8, dtype=torch.uint8, device=dev) if (relu and src == "bits") else None
    out, mean, invstd = ops.bn_fwd(yd, gd, bd, rd, relu, rm, rv, mom, eps, None, bits)
    ref, mu, istd, var = bn_fwd(y, gamma, beta, r, relu, eps)
    b = bn_fwd_bound(y, gamma, beta, r, eps)
    rm_ref, rv_ref = bn_running(torch.zeros(C), torch.ones(C), mu, var, M, mom)
    lay = lambda: layout_rows(M, C)  # noqa: E731
    vec = lambda: layout_vec(C)  # noqa: E731
    tag = f"M={M} C={C} relu={relu} res={res} mask={src}"
    checks = [(f"bn_fwd out {tag}", out, ref, _with_bf16(ref, b["ez"]), lay),
              (f"bn_fwd mean {tag}", mean, mu, b["mean"], vec),
              (f"bn_fwd invstd {tag}", invstd, istd, b["invstd"], vec),
              (f"bn_fwd running_mean {tag}", rm, rm_ref, (1 - mom) * b["mean"] + 3 * U * rm_ref.abs(), vec),
              (f"bn_fwd running_var {tag}", rv, rv_ref,
               (1 - mom) * (M / max(M - 1, 1)) * (b["var"] + 3 * U * var) + 3 * U * rv_ref.abs(), vec)]
    # backward from the kernel's own stored output, mean and invstd
    outc, mean64, istd64 = out.cpu().to(F64), mean.cpu().to(F64), invstd.cpu().to(F64)
    mask = None
    if relu:
        if src == "y":
            # recomputed by the same fp32 fma as the forward's: positive exactly where the stored output is
            mask = outc > 0
        elif src == "bits":
            mask = unpack_bits(bits.cpu(), C)
            checks.append((f"bn_fwd relu bits {tag}", mask.to(F64), (outc > 0).to(F64), 0.0, lay))
        else:
            mask = outc > 0
    dout = c["dout"]
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    dy, dres = ops.bn_bwd(_dev(dout, dev), out if src == "out" else torch.empty_like(out), yd, gd, mean, invstd, relu, res, dg, db,
                          bd if (relu and src == "y") else None, bits, None)
    rdy, rdz, rdg, rdb = bn_bwd(dout, y, gamma, mean64, istd64, mask)
    bb = bn_bwd_bound(rdz, y, gamma, mean64, istd64)
    checks += [(f"bn_bwd dy {tag}", dy, rdy, _with_bf16(rdy, bb["e"]), lay),
               (f"bn_bwd dbeta {tag}", db, rdb, bb["dbeta"], vec),
               (f"bn_bwd dgamma {tag}", dg, rdg, bb["dgamma"], vec)]
    if res:
        checks.append((f"bn_bwd dres {tag}", dres, rdz, 0.0, lay))  # dout through the mask: a copy
    return checks


def bn_combos():
    """(relu, res, mask source): every combination the ops take. The mask recomputed from y needs a
    residual-free forward; without relu there is no mask."""
    out = [(False, False, "none"), (False, True, "none")]
    for res in (False, True):
        for src in ("out", "y", "bits"):
            if src == "y" and res:
                continue
            out.append((True, res, src))
    return out


def run_bn_infer_random(ops, dev, M, C, relu):
    """z = (y - rm) rsqrt(rv + eps) gamma + beta: the sum rv + eps, the rsqrt (1 ulp), the difference,
    two products and the add round once each (or fuse): |dz| <= 8u |z - beta| + u |z|, then bf16."""
    c = cached(random_bn_case, M, C)
    y = c["y"]
    got = ops.bn_infer(_dev(y, dev), c["gamma"].to(dev), c["beta"].to(dev), c["rm"].to(dev), c["rv"].to(dev), 1e-5, relu)
    z = bn_infer(y, c["gamma"], c["beta"], c["rm"], c["rv"], 1e-5, False)
    e = 8 * U * (z - c["beta"].to(F64)).abs() + U * z.abs()
    ref = torch.relu(z) if relu else z
    return [(f"bn_infer M={M} C={C} relu={relu}", got, ref, _with_bf16(ref, e), lambda: layout_rows(M, C))]


# Softmax cross-entropy. The kernel: mx = max z (exact), se = sum __expf(z - mx), lse = mx + __logf(se),
# loss = lse - z[label], dlogits = bf16((__expf(z - lse) - onehot) / N).
# The ROCm tree documents no error for the two intrinsics; its header defines __expf(x) as the hardware
# exp2 of the ROUNDED product log2(e) x and __logf as the builtin logarithm. Taken here: exp2 and log
# within 2 ulp (4u relative); the rounded product moves the exponent by |x| log2(e) u, a relative
# 2 |x| u at most. With x_k = z_k - mx <= 0:
#   rel(se) <= 4u + 2u sum |x_k| e^x_k / se + (K / 256 + 12) u      (the last term: the sum's own roundings)
#   |d log se| <= rel(se) + 4u |log se|
#   the roundings of x_k, lse and loss: u (|z| + |mx| + |lse| + |loss|) <= 2^-22 max |z| + 2u |log se|
# so |dloss| <= 2^-22 max(|z|, 1) + E with E = rel(se) + 6u |log se|. tools/conv_oracle_rel.py records
# the measured |got - ref| / bound (profiles/conv_oracle_r8.txt).
def xent_bounds(z, labels):
    z = z.to(F64)
    N, K = z.shape
    mx = z.max(1, keepdim=True).values
    x = z - mx
    se = torch.exp(x).sum(1)
    rel = 4 * U + 2 * U * (x.abs() * torch.exp(x)).sum(1) / se + (K / 256 + 12) * U
    E = rel + 6 * U * torch.log(se).abs()
    loss_b = 2.0 ** -22 * z.abs().max(1).values.clamp_min(1.0) + E
    lse = mx[:, 0] + torch.log(se)
    xa = z - lse[:, None]
    p = torch.exp(xa)
    # the argument z - lse carries lse's error; then __expf, the subtraction and the product with 1 / N
    ep = p * (loss_b[:, None] + 4 * U + 2 * U * xa.abs() + U * xa.abs()) + 3 * U * (p + 1)
    return loss_b, ep / N


def xent_cases():
    """name -> (logits fp32 [N, K], labels): normal rows; rows of equal logits (prediction 0); logits
    of +-80; the label on a tied maximum."""
    out = {}
    for N, K in XENT:
        g = torch.Generator().manual_seed(N * 1009 + K)
        z = (torch.randn(N, K, generator=g) * 3).to(torch.float32)
        lab = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
        out[f"normal N={N} K={K}"] = (z, lab)
        out[f"equal N={N} K={K}"] = (torch.full((N, K), 1.25), lab)
        big = torch.where(torch.rand(N, K, generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0))
        big[:, K // 2] = 80.0
        out[f"pm80 N={N} K={K}"] = (big, lab)
        t = z.clone()
        top = t.max(1).values + 1
        t[:, 1], t[:, K - 1] = top, top
        out[f"tied N={N} K={K}"] = (t, torch.full((N,), K - 1, dtype=torch.int32))  # the label is the LAST maximum
    return out


def run_xent(ops, dev, name):
    z, lab = cached(xent_cases)[name]
    N, K = z.shape
    loss, corr, dl = ops.softmax_xent(z.to(dev), lab.to(dev))
    rl, rc, rdl = softmax_xent(z, lab)
    lb, db = xent_bounds(z, lab)
    assert torch.isfinite(rl).all()
    return [(f"softmax_xent loss {name}", loss, rl, lb, lambda: {"row": (torch.arange(N), lambda i: f"row {i}")}),
            (f"softmax_xent correct {name}", corr, rc, 0.0, lambda: {"row": (torch.arange(N), lambda i: f"row {i}")}),
            (f"softmax_xent dlogits {name}", dl, rdl, _with_bf16(rdl, db), lambda: layout_rows(N, K, "class"))]
