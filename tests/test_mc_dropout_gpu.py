"""Monte-Carlo dropout on the device (csrc/mnist_mc.h): tfd::mnist_mc_head against the fp64 definition
(training/inference.py mc_dropout_ref over mc_dropout_masks), and MnistEngine.predict_mc.

Bounds, from the formats alone (U = 2^-23; expf, logf and the division at 1 ulp <= U), per row:
  ez     |logit error|: a 1024-term fp32 dot product and hr / keep_prob, (1024 + 3) U max_sc sum_k |a_k| |W_kc|;
         0 in the integer cases, whose logits are exact whatever the order
  rel    relative error of one softmax value: the numerator's and the denominator's exp see ez and the rounding of
         z - max (<= R U, R the row's logit range) each, plus two expf, a sum of 10 and a division:
         rel = 2 ez + (2 R + 16) U
  dp[c]  |mean_prob error|: rel * pbar_c, plus the running mean's and the 16-lane merge's roundings, each relative to
         the values it handles (<= pmax_c = max_s p_sc): (2 T + 96) U pmax_c, plus fp32 underflow 1e-37
  dH     entropy of the mean, first order: sum_c (|ln pbar_c| + 1) dp[c] + 16 U
  dEH    a sample's H = log(se) - sum_c p_c z'_c: rel (S + 3) with S = max_s sum_c p_sc |z'_sc|, the logf and the
         sum of ten products 32 U, the depth-T mean 3 T U
  mutual_info: dH + dEH;  var_prob[c]: 6 dp[c] (a mean of squares of differences of values each within dp).
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import inference as I

import mnist_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -23
MI_ERR_MEASURED = 3.5675e-07  # max |mutual_info - reference| at test_op_random's case (profiles/mc_dropout_rel.txt)
NAMES = ("mean_prob", "classes", "entropy", "expected_entropy", "mutual_info", "var_prob", "loss_rows", "correct_rows")


@pytest.fixture(scope="module")
def held(cuda):
    """held(h, W, b, T, kp, ...): run the op on hidden vectors h [rows,1024] (split into `splits` slabs), hold every
    statistic to the bounds above, return (device results, reference, bounds)."""
    def run(h, W, b, T, kp, splits=1, row0=0, rank=0, seed=11, labels=None, exact=False):
        h, W, b = (np.asarray(a, dtype=np.float32) for a in (h, W, b))
        rows = h.shape[0]
        first = np.floor(h / 2) if splits == 2 else h  # integers stay integers; floats: fp32 a + (h - a) below
        slabs = np.stack([first, h - first][:splits]).astype(np.float32)
        hsum = slabs.sum(0, dtype=np.float32) if splits == 2 else h
        p32 = torch.zeros(M.TOTAL)
        p32[M.OFFSETS["out"]:M.OFFSETS["out"] + W.size] = torch.from_numpy(W.reshape(-1))
        p32[M.OFFSETS["out_b"]:M.OFFSETS["out_b"] + 10] = torch.from_numpy(b)
        y = torch.empty(0, dtype=torch.int32) if labels is None else torch.as_tensor(labels, dtype=torch.int32)
        out = torch.ops.tfd.mnist_mc_head(torch.from_numpy(slabs).to(cuda), rows, p32.to(cuda), y.to(cuda), T, kp, seed, rank, row0)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in zip(NAMES, out)}
        masks = I.mc_dropout_masks(rows, T, row0, rank, seed, kp)
        ref = I.mc_dropout_ref(hsum, W, b, masks, kp, labels)
        z, p = ref["logits"], ref["probs"]
        a = masks * (np.maximum(hsum, 0.0).astype(np.float64) / kp)[:, None, :]
        ez = 0.0 if exact else 1027 * U * (a @ np.abs(W).astype(np.float64)).max((1, 2))
        R = z.max((1, 2)) - z.min((1, 2))
        rel = 2 * ez + (2 * R + 16) * U
        dp = rel[:, None] * ref["mean_prob"] + (2 * T + 96) * U * p.max(1) + 1e-37
        dH = ((np.abs(np.log(np.maximum(ref["mean_prob"], 1e-300))) + 1) * dp).sum(1) + 16 * U
        S = (p * np.abs(z - z.max(-1, keepdims=True))).sum(-1).max(1)
        bnd = {"mean_prob": dp, "entropy": dH, "expected_entropy": rel * (S + 3) + (32 + 3 * T) * U, "var_prob": 6 * dp}
        bnd["mutual_info"] = bnd["entropy"] + bnd["expected_entropy"]
        for k, bd in bnd.items():
            err = np.abs(got[k] - ref[k])
            print("%s T=%d rows=%d: worst error / bound %.3f (bound %.3e)" % (k, T, rows, (err / bd).max(), bd.max()))
            assert (err <= bd).all(), (k, err.max(), bd.max())
        assert (got["var_prob"] >= 0).all() and (got["mutual_info"] >= 0).all()
        top2 = np.sort(ref["mean_prob"], 1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 2 * dp.max(1)
        assert np.array_equal(got["classes"][clear], ref["classes"][clear])
        if labels is not None:
            assert np.array_equal(got["correct_rows"][clear], ref["correct_rows"][clear])
            pl, dl = ref["mean_prob"][np.arange(rows), labels], dp[np.arange(rows), labels]
            fits = pl > 1e-30
            assert (np.abs(got["loss_rows"] - ref["loss_rows"])[fits] <= (1.01 * dl / pl + U * (1 + ref["loss_rows"]))[fits]).all()
            assert (got["loss_rows"][~fits] > 60).all()
        return got, ref, bnd
    return run


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("T", [1, 16, 17, 50])
def test_op_on_integers(held, T, rows, splits):
    """Integer h in [-3, 3], W_out in [-2, 2], keep_prob 0.5 (scale 2): every logit is an exact integer; T = 17 and 50
    end in a ragged tile; row0 = 2^32 + 5 puts the row number in both counter words."""
    g = np.random.default_rng(100 * T + 10 * rows + splits)
    h, W, b = g.integers(-3, 4, (rows, 1024)), g.integers(-2, 3, (1024, 10)), g.integers(-2, 3, 10)
    held(h, W, b, T, 0.5, splits=splits, row0=2 ** 32 + 5, rank=3, labels=g.integers(0, 10, rows), exact=True)


def test_op_random(held):
    """B = 5, T = 48, keep_prob 0.75, h ~ N(0, 1), W_out ~ N(0, 0.05): the format bounds hold. They are worst-case over
    1024-term dot products (mutual_info: 3.4e-2 of values near 0.16, worked out on the CPU), too wide to refuse the
    reference's own mutual_info scaled by 1.02; 3x the measured distance is not, and holds as well."""
    g = np.random.default_rng(5)
    h, W, b = g.standard_normal((5, 1024)), 0.05 * g.standard_normal((1024, 10)), 0.05 * g.standard_normal(10)
    got, ref, bnd = held(h, W, b, 48, 0.75, splits=2, labels=g.integers(0, 10, 5))
    assert MI_ERR_MEASURED is not None and 3 * MI_ERR_MEASURED < 0.02 * ref["mutual_info"].min() / 4
    assert (np.abs(got["mutual_info"] - ref["mutual_info"]) <= 3 * MI_ERR_MEASURED).all()
    assert (np.abs(1.02 * ref["mutual_info"] - got["mutual_info"]) > 3 * MI_ERR_MEASURED).all()


def test_mask_identity(held):
    """h = 1, W_out[:, 0] = 1, keep_prob 0.5: logit 0 of a sample is 2 kept(sample), exactly. With an output bias of
    -1024 on class 0 (the mean of 2 kept) mean_prob[0] is about the share of samples that kept more than half
    their units, which held() compares with the definition's."""
    W, b = np.zeros((1024, 10)), np.zeros(10)
    W[:, 0], b[0] = 1, -1024
    got, _, _ = held(np.ones((2, 1024)), W, b, 17, 0.5, row0=7, exact=True)
    assert 0.05 < got["mean_prob"][:, 0].min() and got["mean_prob"][:, 0].max() < 0.95  # not saturated: held() saw the counts


def _engine(cuda, batch, dtype, flat):
    e = torch.classes.tfd.MnistEngine(batch, 0, 0.75, 1234, 2)
    e.set_dtype(dtype)
    e.set_adam(2.0 ** -7, 0.9, 0.999, 1e-8)
    e.params().copy_(flat.to(cuda))
    e.sync_shadow()
    return e


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine(cuda, held, dtype):
    """B = 5, n = 12 (chunks 5, 5, 2), T = 20: predict_mc is bit-identical run to run, to its three chunks called alone
    with their row0, to an engine of B = 12 and to the op fed the engine's own slabs; at keep_prob 1 it is predict's
    softmax with no spread; and the training state of an engine that called it is the bits of one that never did."""
    params, x, y = O.random_case(12, seed=2)
    flat = M.flat_from_dict(params)
    xd, yd = x.to(cuda), y.to(torch.int32).to(cuda)
    none = torch.empty(0, dtype=torch.int32, device=cuda)
    bits = lambda out: [t.cpu().contiguous().view(torch.int32) for t in out]
    e = _engine(cuda, 5, dtype, flat)
    whole = bits(e.predict_mc(xd, yd, 20, 0.0, 77, False, 0))  # keep_prob 0: the engine's 0.75
    again = bits(e.predict_mc(xd, yd, 20, 0.75, 77, False, 0))
    parts = [bits(e.predict_mc(xd[o:o + 5].contiguous(), yd[o:o + 5].contiguous(), 20, 0.75, 77, False, o)) for o in (0, 5, 10)]
    # the last chunk's slabs are still the engine's: the op on them, as rows 10 and 11
    op = torch.ops.tfd.mnist_mc_head(e.infer_slabs().contiguous(), 2, e.params(), yd[10:], 20, 0.75, 77, 2, 10)
    big = bits(_engine(cuda, 12, dtype, flat).predict_mc(xd, yd, 20, 0.75, 77, False, 0))
    torch.cuda.synchronize()
    for i, w in enumerate(whole):
        assert torch.equal(w, again[i]) and torch.equal(w, torch.cat([p[i] for p in parts])) and torch.equal(w, big[i])
        assert torch.equal(w[10:], bits(op)[i + (i > 2)])  # the op also returns expected_entropy, fourth
    assert len(set(whole[0][:, 0].tolist())) == 12 and not torch.equal(whole[0], bits(e.predict_mc(xd, yd, 20, 0.75, 78, False, 0))[0])
    # keep_prob 1, chunk by chunk (the slabs are a chunk's): T identical samples. predict's softmax (fp64 of its fp32
    # logits, which carry ez) and mean_prob each lie within dp of the exact softmax, so within 2 dp of each other.
    W, b, bd1 = params["out"].numpy(), params["out_b"].numpy(), e.params()[M.OFFSETS["bd1"]:M.OFFSETS["bd1"] + 1024]
    for o in (0, 5, 10):
        xc = xd[o:o + 5].contiguous()
        logits, classes = (t.cpu().numpy().astype(np.float64) for t in e.predict(xc, none, False)[:2])
        one = [t.cpu().numpy() for t in e.predict_mc(xc, none, 20, 1.0, 77, False, o)]
        bnd = held((e.infer_slabs().sum(0) + bd1).cpu().numpy(), W, b, 20, 1.0)[2]
        soft = np.exp(logits - logits.max(1, keepdims=True))
        assert (np.abs(one[0] - soft / soft.sum(1, keepdims=True)) <= 2 * bnd["mean_prob"]).all()
        assert np.array_equal(one[1], classes) and (one[4] == 0).all() and (one[3] <= bnd["mutual_info"]).all() and one[5].size == 0

    def train(between):
        t = _engine(cuda, 5, dtype, flat)
        for i in range(2):
            t.feed_x().copy_(xd[:5])
            t.feed_y().copy_(yd[:5])
            t.train_step()
            if between and i == 0:
                t.predict_mc(xd, yd, 20, 0.0, 77, False, 0)
        torch.cuda.synchronize()
        return bits([t.params(), t.adam_m(), t.adam_v(), t.loss_rows(), t.step_tensor().view(torch.float32)])
    for a, b in zip(train(False), train(True)):
        assert torch.equal(a, b)


def test_refusals(cuda):
    e = _engine(cuda, 5, "bf16", M.flat_from_dict(O.random_case(1)[0]))
    x, none = torch.zeros(3, 784, device=cuda), torch.empty(0, dtype=torch.int32, device=cuda)
    for args, word in (((x, none, 0, 0.5, 1, False, 0), "samples"), ((x, none, I.MC_MAX_SAMPLES + 1, 0.5, 1, False, 0), "samples"),
                       ((x, none, 4, 1.5, 1, False, 0), "keep_prob"), ((x, none, 4, 0.5, 1, True, 0), "set_ema first"),
                       ((x.double(), none, 4, 0.5, 1, False, 0), "must be Float"), ((x.cpu(), none, 4, 0.5, 1, False, 0), "must be on cuda"),
                       ((x, torch.zeros(3, dtype=torch.int64, device=cuda), 4, 0.5, 1, False, 0), "must be Int")):
        with pytest.raises(RuntimeError, match=word):
            e.predict_mc(*args)
