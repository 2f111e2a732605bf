"""training/augment.py, the fp64 reference of the device augmentation kernel, and the CPU runner's use of it."""
import os
import subprocess
import sys

import numpy as np

from tensorflow_distributed_amd.training import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n=7):
    g = np.random.default_rng(0)
    return g.random((n, 784), dtype=np.float32), g.integers(0, 10, n).astype(np.int32), g.permutation(n).astype(np.int32)


def test_identity_returns_the_gathered_rows():
    x, y, perm = _data()
    out, lab = A.augment_batch_ref(x, y, perm, 5, 3, 1, 0, A.augment_config())
    rows = perm[(15 + np.arange(3)) % 7]
    assert np.array_equal(out, x[rows].astype(np.float64)) and np.array_equal(lab, y[rows])


def test_g_sums_to_one_over_an_interior_row():
    rounding = 28 * 2.0 ** -24  # g is fp32: each entry is off by at most 2^-24 of itself
    for sigma in (1.0, 4.0):  # the taps beyond 13 of the middle row carry < 1e-3 at sigma 4
        g = A.augment_config(elastic_alpha=8, elastic_sigma=sigma)["g"].astype(np.float64)
        assert abs(g[0] + 2 * g[1:].sum() - 1.0) < rounding
        assert abs(g[np.abs(13 - np.arange(28))].sum() - 1.0) < (rounding if sigma == 1.0 else 2e-3)
    assert not A.augment_config()["g"].any()


def test_draws_lie_in_range_and_differ_across_step_row_and_rank():
    d = A.native_augment_draws(4, 9, 0, 1)
    for v in d.values():
        assert v.min() >= -1.0 and v.max() < 1.0 and np.array_equal(v, v.astype(np.float32))
    assert d["affine"].shape == (4, 4) and d["nx"].shape == d["ny"].shape == (4, 28, 28)
    assert len({tuple(r) for r in d["affine"]}) == 4 and not np.array_equal(d["nx"], d["ny"])
    for other in (A.native_augment_draws(4, 10, 0, 1), A.native_augment_draws(4, 9, 1, 1), A.native_augment_draws(4, 9, 0, 2)):
        assert not np.array_equal(other["affine"], d["affine"]) and not np.array_equal(other["nx"], d["nx"])
    # a sample's draws depend on its number alone: batch 9 of 4 rows is the first half of batch 4 of 8, shifted
    assert np.array_equal(A.native_augment_draws(8, 4, 0, 1)["nx"][4:], d["nx"])


def test_an_integer_translation_is_a_shifted_image():
    x, y, perm = _data()
    draws = {"affine": np.tile([1.0, -0.5, 0.0, 0.0], (2, 1)), "nx": np.zeros((2, 28, 28)), "ny": np.zeros((2, 28, 28))}
    out, _ = A.augment_batch_ref(x, y, perm, 0, 2, 0, 0, A.augment_config(shift_px=2.0), draws)  # ty = 2, tx = -1
    src = x[perm[:2]].astype(np.float64).reshape(2, 28, 28)
    want = np.zeros_like(src)
    want[:, 2:, :27] = src[:, :26, 1:]  # out[r][c] = src[r - 2][c + 1]
    assert np.array_equal(out.reshape(2, 28, 28), want)


def test_mnist_single_trains_with_augmentation_on_the_cpu(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "mnist_single.py"), "--cpu", "--training_iters", "48", "--batch_size", "16",
           "--augment_shift", "2", "--eval_batches", "1", "--data_dir", str(tmp_path)]
    t = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert t.returncode == 0 and "Optimization Finished!" in t.stdout, t.stdout + t.stderr
