"""The OCP MX block formats of the block-scaled fc1 inference path (csrc/mnist_mx.h), in numpy: the definition the
device kernels are held to.

A block is 32 consecutive elements along one axis with one E8M0 scale byte ``s`` (scale ``2^(s - 127)``); elements
are e4m3 (finite-only, maximum 448: ``"mxfp8"``) or e2m1 (maximum 6: ``"mxfp4"``). Encoding is defined on the bits:

    amax = max |x| over the block;  E = (bits(amax) >> 23) & 0xff;  s = clamp(E - emax, 0, 254)   (emax 8 / 2)
    code = x * 2^(127 - s), rounded to nearest even in the element format, saturated to its maximum

so values in (448, 512) become 448 and values in (6, 8) become 6, and a zero block has ``s = 0`` and zero codes.
Inputs are finite; results on Inf / NaN are unspecified. The e4m3 rounding is torch's ``float8_e4m3fn`` cast, the
one ``optimizers.q8_encode`` uses, behind the saturation (the bare cast turns 465 and above into NaN).
"""
from __future__ import annotations

import numpy as np
import torch

MX_BLOCK = 32
MX_FORMATS = ("mxfp8", "mxfp4")
INFER_FORMATS = ("bf16",) + MX_FORMATS
_EMAX = {"mxfp8": 8, "mxfp4": 2}
_MAX = {"mxfp8": 448.0, "mxfp4": 6.0}
_E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _blocks(a: np.ndarray, axis: int):
    """``a`` with ``axis`` last and split into blocks: ``[..., blocks, 32]``"""
    a = np.moveaxis(a, axis, -1)
    if a.shape[-1] % MX_BLOCK:
        raise ValueError(f"mx: the blocked axis has {a.shape[-1]} elements, not a multiple of {MX_BLOCK}")
    return a.reshape(a.shape[:-1] + (a.shape[-1] // MX_BLOCK, MX_BLOCK))


def _unblocks(b: np.ndarray, axis: int) -> np.ndarray:
    return np.moveaxis(b.reshape(b.shape[:-2] + (-1,)), -1, axis)


def mx_encode(x, fmt: str, axis: int = -1):
    """``(codes, scales)`` of ``x`` blocked along ``axis``: ``codes`` uint8 of ``x``'s shape (an e2m1 code in the low
    four bits of its byte), ``scales`` uint8 with ``axis`` shortened 32-fold."""
    emax, top = _EMAX[fmt], _MAX[fmt]
    b = _blocks(np.ascontiguousarray(np.asarray(x, dtype=np.float32)), axis)
    amax = np.abs(b).max(-1)
    s = np.clip(((amax.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - emax, 0, 254)
    y = np.clip(np.ldexp(b.astype(np.float64), (127 - s)[..., None]), -top, top)  # exact: a power of two, then the band
    if fmt == "mxfp8":
        codes = torch.from_numpy(y.astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    else:
        a = np.abs(y)
        step = np.where(a < 2.0, 0.5, np.where(a < 4.0, 1.0, 2.0))  # the spacing of e2m1 around a
        q = np.rint(a / step) * step  # rint: ties to the even multiple, which is the even mantissa
        codes = (np.searchsorted(_E2M1, q) | (np.signbit(y).astype(np.int64) << 3)).astype(np.uint8)
    return _unblocks(codes, axis), np.moveaxis(s.astype(np.uint8), -1, axis)


def mx_decode(codes, scales, fmt: str, axis: int = -1) -> np.ndarray:
    """float64 values of ``mx_encode``'s ``(codes, scales)``: exact."""
    c = _blocks(np.ascontiguousarray(np.asarray(codes, dtype=np.uint8)), axis)
    if fmt == "mxfp8":
        v = torch.from_numpy(c.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    else:
        v = np.where(c & 8, -1.0, 1.0) * _E2M1[c & 7]
    s = np.moveaxis(np.asarray(scales, dtype=np.uint8), axis, -1).astype(np.int64)
    return _unblocks(np.ldexp(v, (s - 127)[..., None]), axis)


def mx_quantise(x, fmt: str, axis: int = -1) -> np.ndarray:
    """``mx_decode(mx_encode(x))``: the float64 values the block-scaled product multiplies"""
    return mx_decode(*mx_encode(x, fmt, axis), fmt, axis)


def mx_fc1_ref(p2, w, fmt: str) -> np.ndarray:
    """fc1's product ``[rows, 1024]`` in fp64 as the device forms it in format ``fmt``: the activations ``p2``
    ``[rows, 3136]`` as MXFP8 in blocks along each row, the weights ``w`` ``[3136, 1024]`` as ``fmt`` in blocks along
    K (one block per ``(k // 32, n)``). The bias is not added."""
    if fmt not in MX_FORMATS:
        raise ValueError(f"mx_fc1_ref: fmt is one of {MX_FORMATS}, got {fmt!r}")
    return mx_quantise(p2, "mxfp8", 1) @ mx_quantise(w, fmt, 0)
