"""DP-SGD's plain definitions (training/dp_sgd.py), the CPU runner that trains on them, and the accountant."""
import math

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
from tensorflow_distributed_amd.training import dp_sgd as D
from tensorflow_distributed_amd.training import privacy as P
from tensorflow_distributed_amd.training.optimizers import AdamOptimizer


def test_clip_factor_edges():
    c = D.clip_factors([0.0, 2.0, 2.0 + 1e-12, 8.0, 1e-300], 2.0)
    assert list(c[:2]) == [1.0, 1.0] and c[2] < 1.0 and c[3] == 0.25 and c[4] == 1.0


def test_cpu_runner_trains_on_the_reference_gradient():
    g = np.random.default_rng(3)
    x, y = g.random((3, 784), dtype=np.float32), g.integers(0, 10, 3).astype(np.int32)
    r = TorchMnistRunner(3, AdamOptimizer(0.01), keep_prob=1.0, seed=5)
    r.set_params(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(2).items()}))
    flat = r.params().clone()
    norms = D.dp_sgd_gradient_ref(flat, x, y, 1e30)[1]
    clip = float(np.median(norms))
    r.set_dp_sgd(clip, 1.1)
    got, _ = r.compute_grads(torch.from_numpy(x), torch.from_numpy(y))
    want, _, c = D.dp_sgd_gradient_ref(flat, x, y, clip, 1.1, step=1, seed=5)
    assert (c < 1).sum() == 1 and r.dp_clipped_fraction() == pytest.approx(1 / 3)
    assert np.array_equal(got.numpy(), want.astype(np.float32)) and not got[M.NUM_PARAMS:].any()
    # without noise the clipped sum is what the definitions say, row by row
    gi = D.per_example_grads_ref(flat, x, y)
    assert np.allclose(D.dp_sgd_gradient_ref(flat, x, y, clip)[0], (D.clip_factors(norms, clip)[:, None] * gi).mean(0), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        r.set_dp_sgd(0.0, 1.0)


@pytest.mark.parametrize("sigma", [0.7, 1.1, 4.0])
def test_accountant(sigma):
    for a in (2, 5, 32, 256):
        assert P.rdp_sampled_gaussian(1.0, sigma, a) == pytest.approx(a / (2 * sigma ** 2), rel=1e-12)
        assert P.rdp_sampled_gaussian(0.0, sigma, a) == 0.0
        assert 0 < P.rdp_sampled_gaussian(0.01, sigma, a) < a / (2 * sigma ** 2)
    q, delta = 256 / 60000, 1e-5
    eps = [P.epsilon(q, sigma, s, delta) for s in (1, 10, 100, 1000)]
    assert all(a < b for a, b in zip(eps, eps[1:])) and eps[0] > 0
    assert P.epsilon(q, sigma, 100, delta) > P.epsilon(q, 2 * sigma, 100, delta)
    assert P.epsilon(0.0, sigma, 100, delta) == 0.0 and P.epsilon(q, 0.0, 100, delta) == math.inf
