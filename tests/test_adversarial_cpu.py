"""training/adversarial.py: input_grad_from_factors, the definition the GPU tests of the input-gradient kernel
trust, against fp64 autograd through the same chain on random integer factors (every sum and the bf16 rounding of
dz1 exact, so the two are equal)."""
import numpy as np
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import adversarial as A


def test_input_grad_from_factors_equals_autograd():
    g = np.random.default_rng(3)
    B = 2
    dz2 = g.integers(-2, 3, (B, 14, 14, 64)) * (g.random((B, 14, 14, 64)) < 0.1)
    W2, W1 = g.integers(-1, 2, (5, 5, 32, 64)), g.integers(-2, 3, (5, 5, 1, 32))
    p1, idx1 = g.integers(0, 2, (B, 14, 14, 32)), g.integers(0, 4, (B, 14, 14, 32))
    assert np.abs(A.conv2_dgrad_ref(dz2, W2)).max() <= 256  # integers that bf16 holds
    x = torch.zeros(B, 28, 28, 1, dtype=torch.float64, requires_grad=True)
    z1 = M.conv2d_same_nhwc(x, torch.from_numpy(W1).double(), None)
    win = z1.reshape(B, 14, 2, 14, 2, 32).permute(0, 1, 3, 5, 2, 4).reshape(B, 14, 14, 32, 4)  # [..., wi = 2 dr + dc]
    pooled = win.gather(4, torch.from_numpy(idx1)[..., None]).squeeze(4) * torch.from_numpy(p1 != 0)
    z2 = M.conv2d_same_nhwc(pooled, torch.from_numpy(W2).double(), None)
    want, = torch.autograd.grad((z2 * torch.from_numpy(dz2)).sum(), x)
    got = A.input_grad_from_factors(dz2, p1, idx1, W2, W1)
    assert np.abs(got).max() > 0 and np.array_equal(got, want.numpy().reshape(B, 784))

