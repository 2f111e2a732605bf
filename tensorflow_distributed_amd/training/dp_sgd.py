"""DP-SGD (Abadi et al. 2016; TF Privacy's ``DPAdamGaussianOptimizer`` on this same MNIST CNN), defined plainly.

``g_i`` is the gradient of example ``i``'s own loss over all eight variables (not divided by ``B``), with that
step's dropout mask; ``n_i = ||g_i||_2``; ``c_i = min(1, C / n_i)`` (1 at ``n_i = 0``: ``g / max(1, n / C)``). The
update's gradient is ``(sum_i c_i g_i + sigma C z) / B`` with ``z ~ N(0, I)`` over the ``NUM_PARAMS`` real elements
of the flat layout; its pad elements keep a zero gradient.

* ``dp_sgd_gradient_ref``: per-example fp64 autograd through ``models/mnist_cnn.conv_net``: what the CPU runner
  trains on and what the device engine is compared against.
* ``per_example_sqnorms_from_factors``: the device kernel's own computation (``csrc/mnist_dp.h``) in numpy fp64
  from the factors the bf16 step leaves in memory, rounding points included. Columns follow the flat layout:
  ``wc1, bc1, wc2, bc2, wd1, bd1, out, out_b``.
* ``dp_noise_ref``: the device's draws. Philox4x32-10, counter ``(q, step lo, step hi, 0)`` for element group
  ``q = j // 4``, key ``(seed, NOISE_KEY)`` -- no rank. With ``u_k`` the 24-bit uniform of word ``k``:
  ``r0 = sqrt(-2 ln(1 - u_0))``, ``r1 = sqrt(-2 ln(1 - u_2))`` (``1 - u`` lies in ``(0, 1]``) and
  ``z[4q .. 4q + 3] = r0 cos(2 pi u_1), r0 sin(2 pi u_1), r1 cos(2 pi u_3), r1 sin(2 pi u_3)``.
"""
from __future__ import annotations

import numpy as np
import torch

from ..models import mnist_cnn as M
from ..models.mnist_cnn import _philox4x32_10
from .adversarial import _params64, conv2_dgrad_ref, round_bf16

NOISE_KEY = 0xD95A11CE  # csrc/mnist_dp.h kDpNoiseKey
VARIABLES = tuple(M.OFFSETS)  # flat order


def clip_factors(norms, C: float) -> np.ndarray:
    """``min(1, C / n)`` per example, 1 where ``n <= C`` (a zero norm included)"""
    n = np.asarray(norms, dtype=np.float64)
    return np.where(n > C, C / np.where(n > C, n, 1.0), 1.0)


def dp_noise_ref(n: int, step: int, seed: int) -> np.ndarray:
    """``z[0 .. n)`` fp64, ``n`` a multiple of 4: the standard normals the device draws at ``global_step = step``"""
    assert n % 4 == 0
    q = np.arange(n // 4, dtype=np.uint64)
    c1 = np.full(q.shape, step & 0xFFFFFFFF, dtype=np.uint64)
    c2 = np.full(q.shape, (step >> 32) & 0xFFFFFFFF, dtype=np.uint64)
    out = _philox4x32_10((q, c1, c2, np.zeros_like(q)), seed & 0xFFFFFFFF, NOISE_KEY)
    u = [(v >> np.uint64(8)).astype(np.float64) / 16777216.0 for v in out]
    z = np.empty((n // 4, 4))
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(1.0 - u[2 * h]))
        z[:, 2 * h], z[:, 2 * h + 1] = r * np.cos(2.0 * np.pi * u[2 * h + 1]), r * np.sin(2.0 * np.pi * u[2 * h + 1])
    return z.reshape(-1)


def wgrad_ref(inp, dz):
    """Per-example 5x5 SAME weight gradient ``im2col(inp)^T dz`` [B,25,Ci,Co] and bias gradient ``sum_p dz[p]``
    [B,Co] of inp [B,H,W,Ci] and dz [B,H,W,Co]"""
    H = inp.shape[1]
    ip = np.pad(inp, ((0, 0), (2, 2), (2, 2), (0, 0)))
    w = np.stack([np.einsum("bhwi,bhwo->bio", ip[:, t // 5:t // 5 + H, t % 5:t % 5 + H, :], dz) for t in range(25)], 1)
    return w, dz.sum((1, 2))


def unpool1(dz1p, idx1) -> np.ndarray:
    """``dz1`` [B,28,28,32]: the pooled gradient [B,14,14,32] at its window position ``idx1``, zero elsewhere"""
    idx1 = np.asarray(idx1).astype(np.int64)
    dz1 = np.zeros((dz1p.shape[0], 28, 28, M.C1))
    for wi in range(4):
        dz1[:, wi >> 1::2, wi & 1::2, :] = dz1p * (idx1 == wi)
    return dz1


def _wgrad_sq(inp, dz):
    w, b = wgrad_ref(inp, dz)
    return (w ** 2).sum((1, 2, 3)), (b ** 2).sum(1)


def per_example_sqnorms_from_factors(x, p1, idx1, dz2, p2, hd, dh, dlogits, W2, B: int) -> np.ndarray:
    """``sq`` [n,8] fp64 from the bf16 step's factors (every gradient factor carries the ``1 / B`` that the head
    folds into ``dlogits``; ``B^2`` undoes it): ``x`` [n,784], ``p1`` / ``idx1`` [n,14,14,32], ``dz2`` [n,14,14,64],
    ``p2`` [n,3136], ``hd`` / ``dh`` [n,1024], ``dlogits`` [n,10], ``W2`` [5,5,32,64]."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    x, p1, dz2, p2, hd, dh, dl = f(x), f(p1), f(dz2), f(p2), f(hd), f(dh), f(dlogits)
    n = dz2.shape[0]
    dz1 = unpool1(round_bf16(conv2_dgrad_ref(dz2, W2)) * (p1 != 0), idx1)
    sq = np.zeros((n, 8))
    sq[:, 0], sq[:, 1] = _wgrad_sq(round_bf16(x).reshape(n, 28, 28, 1), dz1)
    sq[:, 2], sq[:, 3] = _wgrad_sq(p1, dz2)
    s = lambda a: (a.reshape(n, -1) ** 2).sum(1)
    sq[:, 4], sq[:, 5], sq[:, 6], sq[:, 7] = s(p2) * s(dh), s(dh), s(hd) * s(dl), s(dl)
    return sq * float(B) ** 2


def per_example_grads_ref(params, x, y, keep_prob: float = 1.0, mask=None) -> np.ndarray:
    """``g_i`` [n, TOTAL] fp64 by autograd, one row at a time; ``mask`` [n,1024] is the step's 0/1 dropout mask"""
    p = {k: v.requires_grad_(True) for k, v in _params64(params).items()}
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(-1, 784)
    y = torch.as_tensor(np.asarray(y)).long()
    out = np.zeros((x.shape[0], M.TOTAL))
    for i in range(x.shape[0]):
        m = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.float64))[i:i + 1]
        loss = M.softmax_xent_mean(M.conv_net(x[i:i + 1], p, keep_prob, dropout_mask=m), y[i:i + 1])
        gs = torch.autograd.grad(loss, [p[k] for k in VARIABLES])
        out[i] = _flat64(dict(zip(VARIABLES, gs)))
    return out


def _flat64(d) -> np.ndarray:
    flat = np.zeros(M.TOTAL)
    for k, off in M.OFFSETS.items():
        v = d[k].detach().reshape(-1).numpy()
        flat[off:off + v.size] = v
    return flat


def dp_sgd_gradient_ref(params, x, y, C: float, sigma: float = 0.0, step: int = 0, seed: int = 0, keep_prob: float = 1.0,
                        mask=None):
    """``((sum_i c_i g_i + sigma C z) / n [TOTAL], norms [n], c [n])`` in fp64; ``z = dp_noise_ref(TOTAL, step, seed)``
    over the real elements, ``step`` the global step the update makes"""
    g = per_example_grads_ref(params, x, y, keep_prob, mask)
    norms = np.sqrt((g ** 2).sum(1))
    c = clip_factors(norms, C)
    total = (c[:, None] * g).sum(0)
    if sigma > 0:
        total[:M.NUM_PARAMS] += sigma * C * dp_noise_ref(M.TOTAL, step, seed)[:M.NUM_PARAMS]
    return total / g.shape[0], norms, c
