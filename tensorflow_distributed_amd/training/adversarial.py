"""The input gradient and the fast gradient sign method (FGSM), defined plainly.

``tf.gradients(cost, x)`` of the reference's ``cost = reduce_mean(softmax_cross_entropy(...))`` and the
adversarial example ``x_adv = clip(x + eps * sign(dcost/dx), 0, 1)`` (Goodfellow et al. 2015) made from it.
``input_gradient_ref`` / ``fgsm_ref`` are torch autograd in fp64 through ``models/mnist_cnn.conv_net`` at
``keep_prob = 1``: what the CPU runner trains on and what the device engine is compared against.
``input_grad_from_factors`` is the device kernel's own computation (``csrc/mnist_input_grad.h``) in numpy fp64,
from the operands the bf16 step leaves in memory, rounding point included.
"""
from __future__ import annotations

import numpy as np
import torch

from ..models import mnist_cnn as M


def _params64(params):
    if isinstance(params, torch.Tensor):
        params = M.dict_from_flat(params.detach().cpu())
    return {k: v.detach().cpu().double() for k, v in params.items()}


def input_gradient_ref(params, x, y) -> np.ndarray:
    """``d mean_loss / d x`` [n,784] fp64 of rows ``x`` [n,784] and class ids ``y`` [n]; ``params``: the
    flat buffer or the dict of ``mnist_cnn``."""
    p = _params64(params)
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)).reshape(-1, 784).requires_grad_(True)
    if x.shape[0] == 0:
        return np.zeros((0, 784))
    loss = M.softmax_xent_mean(M.conv_net(x, p, 1.0), torch.as_tensor(np.asarray(y)).long())
    g, = torch.autograd.grad(loss, x)
    return g.numpy()


def fgsm_rows(x, dx, eps: float, adv_rows: int = -1) -> np.ndarray:
    """``clip(x + eps_b * sign(dx), 0, 1)`` in fp32, ``eps_b = eps`` for rows ``b < adv_rows`` (-1: all); the
    other rows are ``x`` itself. The device epilogue, element for element."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 784)
    n = x.shape[0]
    k = n if adv_rows < 0 else min(int(adv_rows), n)
    out = x.copy()
    if eps != 0 and k:
        out[:k] = np.clip(x[:k] + np.float32(eps) * np.sign(np.asarray(dx)[:k]).astype(np.float32), np.float32(0), np.float32(1))
    return out


def fgsm_ref(params, x, y, eps: float, adv_rows: int = -1) -> np.ndarray:
    """The FGSM batch [n,784] fp32 of the fp64 input gradient."""
    return fgsm_rows(x, input_gradient_ref(params, x, y), eps, adv_rows)


def round_bf16(a: np.ndarray) -> np.ndarray:
    """fp64 values rounded to the nearest bf16 (8 significant bits, ties to even), as fp64"""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def conv2_dgrad_ref(dz2: np.ndarray, W2: np.ndarray) -> np.ndarray:
    """``dp1[b][p][ci] = sum_{tap,co} dz2[b][p - tap][co] W2[tap][ci][co]`` (SAME padding: ``p - (kh - 2, kw - 2)``)"""
    dz2 = np.asarray(dz2, dtype=np.float64)
    W2 = np.asarray(W2, dtype=np.float64).reshape(5, 5, M.C1, M.C2)
    dzp = np.pad(dz2, ((0, 0), (2, 2), (2, 2), (0, 0)))
    dp1 = np.zeros(dz2.shape[:3] + (M.C1,))
    for kh in range(5):
        for kw in range(5):
            dp1 += dzp[:, 4 - kh:18 - kh, 4 - kw:18 - kw, :] @ W2[kh, kw].T
    return dp1


def input_grad_from_factors(dz2, p1, idx1, W2, W1) -> np.ndarray:
    """``dx`` [B,784] fp64 from the bf16 step's operands: ``dz2`` [B,14,14,64] the conv2 pre-activation
    gradient, ``p1`` [B,14,14,32] the pooled conv1 activations (ReLU live iff ``!= 0``), ``idx1`` the window
    position ``wi`` of each (row ``wi >> 1``, column ``wi & 1``), ``W2`` [5,5,32,64], ``W1`` [5,5,1,32].
    Phase 1 conv2 dgrad; phase 2 ``dz1[2q + wi][c] = bf16(dp1[q][c])`` where live; phase 3 the tap products
    ``T[p][tap] = sum_c dz1[p][c] W1[tap][c]`` gathered as ``dx[u][v] = sum_{i,j} T[(u - i + 2, v - j + 2)][5i + j]``."""
    return conv1_dgrad_ref(round_bf16(conv2_dgrad_ref(dz2, W2)) * (np.asarray(p1, dtype=np.float64) != 0), idx1, W1)


def conv1_dgrad_ref(dz1p, idx1, W1) -> np.ndarray:
    """Phases 2 and 3 without the mask and the rounding: ``dz1p`` [B,14,14,32] placed at the window positions
    ``idx1``, through conv1's transpose, [B,784]. Linear in ``dz1p``: on absolute values it carries an error bound."""
    dz1p = np.asarray(dz1p, dtype=np.float64)
    idx1 = np.asarray(idx1).astype(np.int64)
    B = dz1p.shape[0]
    dz1 = np.zeros((B, 28, 28, M.C1))
    for wi in range(4):
        dz1[:, wi >> 1::2, wi & 1::2, :] = dz1p * (idx1 == wi)
    T = dz1 @ np.asarray(W1, dtype=np.float64).reshape(25, M.C1).T
    Tp = np.pad(T, ((0, 0), (2, 2), (2, 2), (0, 0)))
    dx = np.zeros((B, 28, 28))
    for i in range(5):
        for j in range(5):
            dx += Tp[:, 4 - i:32 - i, 4 - j:32 - j, 5 * i + j]
    return dx.reshape(B, 784)
