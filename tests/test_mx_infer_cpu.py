"""The OCP MX formats of the block-scaled fc1 (training/mx_quant.py; csrc/mnist_mx.h is the same definition on the
device): the encode rule on hand-written blocks, idempotence, and TorchMnistRunner.set_infer_format."""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
from tensorflow_distributed_amd.training import mx_quant as Q
from tensorflow_distributed_amd.training.optimizers import AdamOptimizer


def _block(*head):
    b = np.zeros(32, dtype=np.float32)
    b[:len(head)] = head
    return b


# per format: (the block's leading values, its scale byte, their decoded values)
VECTORS = {
    "mxfp8": [
        ((0.0,), 0, (0.0,)),                                          # a zero block
        ((4.0, -1.0), 121, (4.0, -1.0)),                              # amax at a power of two: E = 129, s = E - 8
        ((450.0, -3.0), 127, (448.0, -3.0)),                          # 450: the saturation band
        ((256.0, 17.0, 19.0, -17.0), 127, (256.0, 16.0, 20.0, -16.0)),  # ties at spacing 2: to the even mantissa
        ((256.0, 2.0 ** -10, 2.0 ** -9, 3 * 2.0 ** -10), 127, (256.0, 0.0, 2.0 ** -9, 2.0 ** -8)),  # flush; subnormal tie
    ],
    "mxfp4": [
        ((0.0,), 0, (0.0,)),
        ((4.0, -1.0), 127, (4.0, -1.0)),                              # E = 129, s = E - 2
        ((7.0, 1.0), 127, (6.0, 1.0)),                                # 7: the saturation band
        ((4.0, 2.5, 3.5, 5.0, -1.25, 0.75), 127, (4.0, 2.0, 4.0, 4.0, -1.0, 1.0)),  # ties
        ((4.0, 0.25, 0.2, -0.26), 127, (4.0, 0.0, 0.0, -0.5)),        # small members flush to 0 (0.25 is a tie)
    ],
}


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
def test_hand_written_blocks(fmt):
    for head, s, want in VECTORS[fmt]:
        codes, scales = Q.mx_encode(_block(*head), fmt)
        assert scales.tolist() == [s], (head, scales)
        dec = Q.mx_decode(codes, scales, fmt)
        assert np.array_equal(dec, _block(*want).astype(np.float64)), (head, dec[:len(head)])
    assert not Q.mx_encode(_block(), fmt)[0].any()


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
@pytest.mark.parametrize("axis", [0, 1])
def test_decode_encode_is_idempotent(fmt, axis):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((64, 96)) * np.exp2(rng.integers(-20, 20, (64, 96)))).astype(np.float32)
    codes, scales = Q.mx_encode(x, fmt, axis)
    assert codes.shape == x.shape and scales.shape == ((2, 96) if axis == 0 else (64, 3))
    d = Q.mx_decode(codes, scales, fmt, axis)
    codes2, scales2 = Q.mx_encode(d, fmt, axis)
    assert np.array_equal(Q.mx_decode(codes2, scales2, fmt, axis), d)


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
def test_torch_runner_predicts_with_mx_fc1_ref(fmt):
    r = TorchMnistRunner(8, AdamOptimizer(0.01), 1.0, 0, 0, torch.device("cpu"))
    r.flat.copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(7).items()}))
    x = torch.rand(5, 784, generator=torch.Generator().manual_seed(1))
    base = r.predict(x)[0]
    r.set_infer_format(fmt)
    p = M.dict_from_flat(r.flat)
    a = x.reshape(-1, 28, 28, 1)
    a = M.maxpool_same_nhwc(torch.relu(M.conv2d_same_nhwc(a, p["wc1"], p["bc1"])), 2)
    a = M.maxpool_same_nhwc(torch.relu(M.conv2d_same_nhwc(a, p["wc2"], p["bc2"])), 2).reshape(-1, M.FEAT)
    h = Q.mx_fc1_ref(a.to(torch.bfloat16).float().numpy(), p["wd1"].numpy(), fmt) + p["bd1"].numpy().astype(np.float64)
    want = np.maximum(h, 0) @ p["out"].numpy().astype(np.float64) + p["out_b"].numpy()
    got = r.predict(x)[0].numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    r.set_infer_format("bf16")
    assert torch.equal(r.predict(x)[0], base)
