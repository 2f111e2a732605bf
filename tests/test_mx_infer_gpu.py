"""Block-scaled fc1 on the device (csrc/mnist_mx.h): tfd::mx_pack_fc1 + tfd::mnist_fc1_mx against the numpy
definition (training/mx_quant.py), and MnistEngine.set_infer_format.

Exact cases compare with == (-0 equals +0): one-hot activations return the decoded weights, selector weights the decoded
activations, and on small dyadic operands every fp32 partial sum is exact in any order. Dense random operands are held to
the worst case of 3136 truncating fp32 additions, 3136 * 2^-23 * sum_k |a_k| |w_k|.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import mx_quant as Q

import infer_oracle as IO
import mnist_oracle as O

pytestmark = pytest.mark.gpu
FEAT, HID = 3136, 1024
# edge blocks' leading values (bf16s): amax a power of two, the saturation band, ties, members that flush to 0
EDGE = {"mxfp8": [(4.0, 1.0), (452.0, 3.0), (256.0, 17.0, 19.0, 21.0), (256.0, 2.0 ** -10, 2.0 ** -9, 3 * 2.0 ** -10)],
        "mxfp4": [(4.0, 1.0), (7.0, 1.0), (4.0, 2.5, 3.5, 5.0, 1.25, 0.75), (4.0, 0.25, 0.2001953125, 0.26171875)]}


def _plant(a, fmt, signed):
    """edge blocks (and a zero block) over leading blocks of `a`'s rows, each at several block positions"""
    blocks = [()] + EDGE[fmt]
    for i, head in enumerate(blocks):
        for r, kb in ((i, 0), (a.shape[0] - 1 - i, a.shape[1] // 32 - 1), (3 * i + 1, 13 + i)):
            a[r, 32 * kb:32 * kb + 32] = 0
            a[r, 32 * kb:32 * kb + len(head)] = head
            if signed and head:
                a[r, 32 * kb + 1] *= -1
    return a


def _bytes(t):
    return t.cpu().numpy().tobytes()  # the copy waits for the stream


def _fc1(cuda, p2, w, fmt):
    """the two ops on host operands; the slabs summed over the splits in fp64 on the host"""
    packed = torch.ops.tfd.mx_pack_fc1(torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(cuda), fmt)
    slabs = torch.ops.tfd.mnist_fc1_mx(torch.from_numpy(np.ascontiguousarray(p2, dtype=np.float32)).to(cuda).to(torch.bfloat16), packed, fmt)
    assert tuple(slabs.shape) == (7, p2.shape[0], HID) and slabs.dtype == torch.float32
    return slabs.double().sum(0).cpu().numpy()


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
def test_one_hot_rows_return_the_decoded_weights(cuda, fmt):
    rng = np.random.default_rng(1)
    w = _plant(rng.standard_normal((HID, FEAT)).astype(np.float32), fmt, True).T  # blocks run along K
    got = _fc1(cuda, np.eye(FEAT, dtype=np.float32), w, fmt)
    want = Q.mx_decode(*Q.mx_encode(w, fmt, 0), fmt, 0)
    assert (got == want).all(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
@pytest.mark.parametrize("off", [0, 1024, 2048, 2112])
def test_selector_weights_return_the_decoded_activations(cuda, fmt, off):
    rng = np.random.default_rng(2)
    p2 = np.abs(rng.standard_normal((37, FEAT))) * np.exp2(rng.integers(-6, 6, (37, 1)))
    p2 = _plant(torch.from_numpy(p2).to(torch.bfloat16).float().numpy(), "mxfp8", False)
    w = np.zeros((FEAT, HID), dtype=np.float32)
    w[off + np.arange(HID), np.arange(HID)] = 1.0
    got = _fc1(cuda, p2, w, fmt)
    want = Q.mx_decode(*Q.mx_encode(p2, "mxfp8", 1), "mxfp8", 1)[:, off:off + HID]
    assert (got == want).all(), np.argwhere(got != want)[:8]


@pytest.fixture(scope="module")
def dyadic():
    """weights +-{0, .5, 1, 1.5, 2, 3, 4, 6} * 2^sw, sw per (k // 32, n) block in {-1, 0, 1}: shared, read only"""
    rng = np.random.default_rng(3)
    w = rng.choice([0, .5, 1, 1.5, 2, 3, 4, 6], (FEAT, HID)) * rng.choice([-1.0, 1.0], (FEAT, HID))
    return w * np.exp2(np.repeat(rng.integers(-1, 2, (FEAT // 32, HID)), 32, 0))


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
@pytest.mark.parametrize("rows", [1, 31, 33, 65, 130])
def test_dense_dyadic_operands_are_exact(cuda, dyadic, fmt, rows):
    rng = np.random.default_rng(rows)
    a = rng.integers(0, 8, (rows, FEAT)) * np.exp2(np.repeat(rng.integers(-1, 2, (rows, FEAT // 32)), 32, 1))
    assert np.array_equal(Q.mx_quantise(a, "mxfp8", 1), a) and np.array_equal(Q.mx_quantise(dyadic, fmt, 0), dyadic)
    assert np.array_equal(np.rint(a * 2) , a * 2) and np.array_equal(np.rint(dyadic * 4), dyadic * 4)  # products: multiples of 2^-3
    assert (np.abs(a) @ np.abs(dyadic)).max() <= FEAT * 168 < 2 ** 20  # so every partial sum fits 24 bits
    got = _fc1(cuda, a, dyadic, fmt)
    want = a @ dyadic
    assert (got == want).all(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
def test_dense_random_within_the_fp32_summation_bound(cuda, fmt):
    rng = np.random.default_rng(4)
    p2 = torch.from_numpy(np.abs(rng.standard_normal((65, FEAT)))).to(torch.bfloat16).float().numpy()
    w = (0.05 * rng.standard_normal((FEAT, HID))).astype(np.float32)
    got = _fc1(cuda, p2, w, fmt)
    want = Q.mx_fc1_ref(p2, w, fmt)
    bound = FEAT * 2.0 ** -23 * (np.abs(Q.mx_quantise(p2, "mxfp8", 1)) @ np.abs(Q.mx_quantise(w, fmt, 0)))
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("fmt", Q.MX_FORMATS)
@pytest.mark.parametrize("rows", [5, 130])
def test_engine(cuda, fmt, rows):
    params, x, y = O.random_case(rows)
    e = torch.classes.tfd.MnistEngine(128, 0, 1.0, 1234, 0)
    e.set_adam(2.0 ** -7, 0.9, 0.999, 1e-8)
    none = torch.empty(0, dtype=torch.int32, device=cuda)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        e.params().copy_(M.flat_from_dict(params).to(cuda))
        e.sync_shadow()
        xd, yd = x.to(cuda), y.to(torch.int32).to(cuda)
        base = e.predict(xd, none, False)[0].clone()
        e.set_infer_format(fmt)
        assert e.infer_format() == fmt
        with pytest.raises(RuntimeError, match="set_infer_format"):
            e.set_dtype("fp32")
        logits = e.predict(xd, none, False)[0]
        nb = rows % 128  # the last chunk
        slabs = e.infer_slabs().clone()
        w1 = e.params()[M.OFFSETS["wd1"]:M.OFFSETS["wd1"] + FEAT * HID].view(FEAT, HID)
        want = torch.ops.tfd.mnist_fc1_mx(e.pool2()[:nb].contiguous(), torch.ops.tfd.mx_pack_fc1(w1.contiguous(), fmt), fmt)
        assert tuple(slabs.shape) == (7, nb, HID) and torch.equal(slabs.view(torch.int32), want.view(torch.int32))
        h = np.maximum(slabs.double().sum(0).cpu().numpy() + params["bd1"].double().numpy(), 0)
        ref = h @ params["out"].double().numpy() + params["out_b"].double().numpy()
        assert IO.logit_rel(logits[rows - nb:].cpu().numpy(), ref) <= IO.LOGIT_BOUND["bf16"]
        e.set_eval_dataset(xd, yd)
        e.capture_eval("ev", 0, rows, rows, False)
        recs = []
        for step in range(2):
            e.set_infer_format(Q.MX_FORMATS[fmt == "mxfp8"])  # the other one: a graph keeps its format and its buffers
            e.replay("ev", 1)
            recs.append(_bytes(e.eval_records("ev")))
            e.set_infer_format(fmt)
            assert recs[-1] == _bytes(e.evaluate_dataset(0, rows, rows, False))
            e.feed_x().copy_(xd[:128].repeat(26, 1)[:128])
            e.feed_y().copy_(yd[:128].repeat(26)[:128])
            e.train_step()
        assert recs[0] != recs[1]
        e.params().copy_(M.flat_from_dict(params).to(cuda))
        e.sync_shadow()
        e.set_infer_format("bf16")
        again = e.predict(xd, none, False)[0]
    assert torch.equal(again.view(torch.int32), base.view(torch.int32))
