"""Monte-Carlo dropout off the device: the fp64 definition and the mask replay (training/inference.py), the CPU
runner's predict_mc and the drivers' --mc_dropout_samples."""
import contextlib

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import inference as I


def test_ref_on_a_hand_case():
    """Two samples, keep_prob 0.5: sample 0 keeps unit 0 (logits (2 ln 3, 0, ..)), sample 1 keeps nothing (uniform);
    unit 1 is negative and never counts."""
    h, W, masks = np.zeros((1, 1024)), np.zeros((1024, 10)), np.zeros((1, 2, 1024))
    h[0, :2], W[0, 0], W[1, 1] = (np.log(3.0), -5.0), 1.0, 1.0
    masks[0, 0, :2] = 1
    r = I.mc_dropout_ref(h, W, np.zeros(10), masks, 0.5, labels=[0])
    p0 = np.array([9.0] + [1.0] * 9) / 18.0
    pbar = (p0 + 0.1) / 2
    ent = lambda p: -(p * np.log(p)).sum()
    assert np.allclose(r["mean_prob"][0], pbar, rtol=0, atol=1e-15) and r["classes"][0] == 0 and r["correct_rows"][0] == 1
    assert np.isclose(r["entropy"][0], ent(pbar), atol=1e-14) and np.isclose(r["expected_entropy"][0], (ent(p0) + np.log(10)) / 2, atol=1e-14)
    assert np.isclose(r["mutual_info"][0], ent(pbar) - (ent(p0) + np.log(10)) / 2, atol=1e-14) and r["mutual_info"][0] > 0.05
    assert np.allclose(r["var_prob"][0], (p0 - 0.1) ** 2 / 4, rtol=0, atol=1e-15) and np.isclose(r["loss_rows"][0], -np.log(0.3), atol=1e-14)


@pytest.mark.parametrize("keep_prob", [0.5, 0.25])
def test_mask_statistics(keep_prob):
    """The kept fraction is within 5 sigma of keep_prob, and the masks of two rows, two samples, two seeds and two
    ranks each differ in more than 40 % of the positions where either keeps (independent masks at keep_prob k differ
    in 2 (1 - k) / (2 - k) of them: 0.67 and 0.86)."""
    row0 = 2 ** 32 - 1  # the two rows differ in both counter words
    m = I.mc_dropout_masks(2, 64, row0, 1, 9, keep_prob)
    n = m.size
    assert m.shape == (2, 64, 1024) and abs(m.mean() - keep_prob) < 5 * np.sqrt(keep_prob * (1 - keep_prob) / n)
    for other in (m[1], np.roll(m[0], 1, 0), I.mc_dropout_masks(1, 64, row0, 1, 10, keep_prob)[0], I.mc_dropout_masks(1, 64, row0, 2, 9, keep_prob)[0]):
        either = (m[0] + other) > 0
        assert ((m[0] != other) & either).sum() > 0.4 * either.sum()
    assert np.array_equal(I.mc_dropout_masks(1, 3, row0 + 1, 1, 9, keep_prob)[0], m[1, :3])  # a row's masks are its own


def test_cpu_runner_predict_mc():
    from tensorflow_distributed_amd.models.mnist_runner import MC_KEYS, TorchMnistRunner
    from tensorflow_distributed_amd.training.optimizers import AdamOptimizer

    r = TorchMnistRunner(4, AdamOptimizer(0.01), keep_prob=0.75, seed=3)
    r.set_params(M.flat_from_dict({k: 0.05 * v for k, v in M.init_params(1).items()}))
    x, y = torch.rand(5, 784, generator=torch.Generator().manual_seed(0)), torch.tensor([1, 2, 3, 4, 5])
    out = r.predict_mc(x, y, samples=6)
    assert tuple(out) == MC_KEYS and tuple(out["mean_prob"].shape) == (5, 10) == tuple(out["var_prob"].shape)
    assert all(tuple(out[k].shape) == (5,) for k in MC_KEYS if not k.endswith("_prob")) and out["classes"].dtype == torch.int32
    assert torch.allclose(out["mean_prob"].sum(1), torch.ones(5), atol=1e-6) and (out["mutual_info"] > 0).all()


@pytest.mark.parametrize("argv,word", [([], None), (["--mc_dropout_samples=20"], None),
                                       (["--mc_dropout_samples=-1"], "must be in"), (["--mc_dropout_samples=5000"], "must be in"),
                                       (["--mc_dropout_samples=20", "--model=resnet18"], "with --model resnet18"),
                                       (["--mc_dropout_samples=20", "--sync_replicas=False"], "parameter-server role"),
                                       (["--mc_dropout_samples=20", "--replicas_to_aggregate=1"], "parameter-server role")])
def test_flag_refusals(argv, word):
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog"] + argv)
        with contextlib.nullcontext() if word is None else pytest.raises(ValueError, match=word):
            dist_main.check_mc_dropout_flags(2)
    finally:
        F.FLAGS.reset()
