"""Train-time data augmentation: the fp64 reference of the device kernel (csrc/mnist_augment.h).

Random shifts, rotations and scales plus Simard-style elastic distortion of 28 x 28 images. The device
kernel (csrc/kernels/mnist_augment.hip) and this module implement ONE definition:

* sample ``i = step * B + b`` reads ``row = perm[i % n]``;
* Philox4x32-10 with counter ``(i lo, i hi, draw, rank)`` and key ``(seed, AUGMENT_KEY)`` gives four 24-bit
  uniforms per call: draw 0 -> ``ty, tx, theta, s``; draws ``1 + k`` / ``197 + k`` (``k`` in ``[0, 196)``)
  -> elements ``4k .. 4k + 3`` of the noise fields ``N_x`` / ``N_y``; every uniform enters as ``2u - 1``;
* ``S = alpha G N G^T`` with ``G[i][j] = g[|i - j|]``, ``g`` the normalised Gaussian of the config;
* ``(y, x) = ctr + (1 / s) R(theta) ((r, c) - ctr) - (ty, tx) + (S_y, S_x)[r][c]``, ``ctr = 13.5``;
* bilinear sampling, zero outside ``[0, 27]^2``.

The config's numbers are rounded to fp32 first, as the device holds them; everything after is fp64.
``TorchMnistRunner.set_augment`` trains on this reference, so ``--augment_*`` works on the CPU too.
"""
from __future__ import annotations

import math

import numpy as np

from ..models.mnist_cnn import _philox4x32_10

AUGMENT_KEY = 0xA06E17A1  # csrc/mnist_augment.h kAugmentKey
SIDE, CTR = 28, 13.5
DRAW_AFFINE, DRAW_NX, DRAW_NY = 0, 1, 197
FIELDS = ("shift_px", "rotate_rad", "scale", "elastic_alpha", "elastic_sigma")


def augment_config(shift_px=0.0, rotate_deg=0.0, scale=0.0, elastic_alpha=0.0, elastic_sigma=0.0) -> dict:
    """The device's AugmentConfig: the five magnitudes rounded to fp32 (rotation in radians) and the
    table ``g[d] = exp(-d^2 / 2 sigma^2) / sum_{k=-27..27} exp(-k^2 / 2 sigma^2)``, fp64 rounded to fp32
    (zeros without elastic distortion)."""
    if not (shift_px >= 0 and rotate_deg >= 0 and 0 <= scale < 1 and elastic_alpha >= 0 and elastic_sigma >= 0):
        raise ValueError("augment: shift, rotate, alpha, sigma >= 0 and 0 <= scale < 1")
    if elastic_alpha > 0 and not elastic_sigma > 0:
        raise ValueError("augment: elastic_alpha > 0 needs elastic_sigma > 0")
    vals = (shift_px, rotate_deg * (math.pi / 180.0), scale, elastic_alpha, elastic_sigma)
    cfg = {k: float(np.float32(v)) for k, v in zip(FIELDS, vals)}
    g = np.zeros(SIDE, np.float32)
    if elastic_alpha > 0:
        e = np.exp(-np.arange(SIDE, dtype=np.float64) ** 2 / (2.0 * float(elastic_sigma) ** 2))
        g = (e / (e[0] + 2.0 * e[1:].sum())).astype(np.float32)
    cfg["g"] = g
    return cfg


def augment_on(cfg: dict) -> bool:
    return any(cfg[k] != 0.0 for k in FIELDS[:4])


def native_augment_draws(B: int, step: int, rank: int, seed: int) -> dict:
    """The numbers the device draws for batch ``step`` of ``B`` rows, each already ``2u - 1`` (exact in
    fp32): ``affine [B, 4]`` = (ty, tx, theta, s) and the noise fields ``nx``, ``ny`` ``[B, 28, 28]``, fp64."""
    i = np.uint64(int(step) * int(B)) + np.arange(B, dtype=np.uint64)
    draw = np.arange(DRAW_NY + 196, dtype=np.uint64)
    shape = (B, draw.size)
    c0 = np.broadcast_to((i & np.uint64(0xFFFFFFFF))[:, None], shape)
    c1 = np.broadcast_to((i >> np.uint64(32))[:, None], shape)
    c2 = np.broadcast_to(draw[None, :], shape)
    c3 = np.full(shape, rank & 0xFFFFFFFF, dtype=np.uint64)
    out = _philox4x32_10((c0, c1, c2, c3), seed & 0xFFFFFFFF, AUGMENT_KEY)
    u = np.stack([(v >> np.uint64(8)).astype(np.float64) / 16777216.0 for v in out], axis=-1)  # [B, draws, 4]
    v = 2.0 * u - 1.0
    return {"affine": v[:, DRAW_AFFINE], "nx": v[:, DRAW_NX:DRAW_NY].reshape(B, SIDE, SIDE),
            "ny": v[:, DRAW_NY:].reshape(B, SIDE, SIDE)}


def source_coords(cfg: dict, draws: dict):
    """(y, x) ``[B, 28, 28]`` fp64: where each destination pixel samples the source image."""
    a = draws["affine"]
    ty, tx = cfg["shift_px"] * a[:, 0], cfg["shift_px"] * a[:, 1]
    theta, s = cfg["rotate_rad"] * a[:, 2], 1.0 + cfg["scale"] * a[:, 3]
    dy, dx = np.meshgrid(np.arange(SIDE) - CTR, np.arange(SIDE) - CTR, indexing="ij")
    cs, sn, inv = (v[:, None, None] for v in (np.cos(theta), np.sin(theta), 1.0 / s))
    y = CTR + inv * (cs * dy - sn * dx) - ty[:, None, None]
    x = CTR + inv * (sn * dy + cs * dx) - tx[:, None, None]
    if cfg["elastic_alpha"] != 0.0:
        d = np.abs(np.arange(SIDE)[:, None] - np.arange(SIDE)[None, :])
        G = cfg["g"].astype(np.float64)[d]
        y = y + cfg["elastic_alpha"] * (G @ draws["ny"] @ G.T)
        x = x + cfg["elastic_alpha"] * (G @ draws["nx"] @ G.T)
    return y, x


def warp_rows_ref(rows, cfg: dict, draws: dict) -> np.ndarray:
    """``rows [B, 784]`` sampled bilinearly at ``source_coords``, zero outside the image; fp64."""
    B = rows.shape[0]
    img = np.zeros((B, SIDE + 3, SIDE + 3))  # pixel (r, c) at [r + 1, c + 1]; zeros around
    img[:, 1:SIDE + 1, 1:SIDE + 1] = np.asarray(rows, dtype=np.float64).reshape(B, SIDE, SIDE)
    y, x = (np.clip(v, -1.0, float(SIDE)) for v in source_coords(cfg, draws))
    y0, x0 = np.floor(y), np.floor(x)
    wy, wx = y - y0, x - x0
    bi = np.arange(B)[:, None, None]
    iy, ix = y0.astype(np.int64) + 1, x0.astype(np.int64) + 1
    top = (1.0 - wx) * img[bi, iy, ix] + wx * img[bi, iy, ix + 1]
    bot = (1.0 - wx) * img[bi, iy + 1, ix] + wx * img[bi, iy + 1, ix + 1]
    return ((1.0 - wy) * top + wy * bot).reshape(B, SIDE * SIDE)


def augment_batch_ref(data, labels, perm, step: int, B: int, seed: int, rank: int, cfg: dict, draws: dict = None):
    """What ``tfd::augment_batch`` computes, in numpy fp64: ``(x [B, 784] fp64, y [B] int32)``. ``draws``
    replaces the Philox draws (``native_augment_draws``'s layout)."""
    data, labels, perm = np.asarray(data), np.asarray(labels), np.asarray(perm)
    n = data.shape[0]
    rows = perm[[(int(step) * int(B) + b) % n for b in range(B)]]
    if draws is None:
        draws = native_augment_draws(B, step, rank, seed)
    return warp_rows_ref(data[rows], cfg, draws), labels[rows].astype(np.int32)
