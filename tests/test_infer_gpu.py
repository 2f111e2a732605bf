"""Device inference (csrc/mnist_infer.h, kernels/mnist_infer.hip): MnistEngine.predict,
set_eval_dataset / evaluate_dataset / capture_eval, and the runners' methods over them.

The exact cases (tests/infer_oracle.py) have integer logits, so logits, classes, correct flags and the
records' counts are compared with ==; the inference head is held bit for bit to the training heads'
loss_rows() / correct_rows(); the logits of dense random cases to the fp64 oracle within 3x the
measured error. "Bit-identical" is torch.equal on integer views.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import inference

import infer_oracle as IO
import mnist_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp32")
SEED = 1234


def _bits(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _engine(cuda, batch, dtype, params, keep=1.0):
    e = torch.classes.tfd.MnistEngine(batch, 0, keep, SEED, 0)
    e.set_dtype(dtype)
    e.set_adam(2.0 ** -7, 0.9, 0.999, 1e-8)
    e.params().copy_((params if torch.is_tensor(params) else M.flat_from_dict(params)).to(cuda))
    e.sync_shadow()
    return e


def _none(cuda):
    return torch.empty(0, dtype=torch.int32, device=cuda)


def _predict(e, x, y=None, use_ema=False):
    """predict on a stream of its own; the four results on the host"""
    cuda = torch.device("cuda", 0)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = e.predict(x.to(cuda).contiguous(), _none(cuda) if y is None else y.to(torch.int32).to(cuda), use_ema)
    torch.cuda.synchronize()
    logits, classes, loss, correct = out
    n = x.shape[0]
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (n, 10)
    assert classes.dtype == torch.int32 and tuple(classes.shape) == (n,)
    assert tuple(loss.shape) == tuple(correct.shape) == ((n,) if y is not None else (0,))
    return [t.cpu() for t in out]


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_logits_classes_and_ties(cuda, dtype):
    """Integer cases: the logits EQUAL the oracle's, the classes numpy's first-maximum argmax, the correct
    flags the oracle's -- over chunks 16, 16, 5 of an engine at batch 16, and at batch 5."""
    params, x, y, ref = IO.spread_integer_case(37)
    p5, x5, y5 = O.integer_case(5)
    ref5 = O.oracle_step(p5, x5, y5, dtype, backward=False)
    for batch, (pp, xx, yy, rr) in ((16, (params, x, y, ref)), (5, (p5, x5, y5, ref5))):
        lg = rr["logits"].numpy()
        assert ((lg == lg.max(1, keepdims=True)).sum(1) > 1).any(), "the case has top-logit ties"
        e = _engine(cuda, batch, dtype, pp)
        logits, classes, loss, correct = _predict(e, xx, yy)
        assert np.array_equal(logits.numpy().astype(np.float64), lg)
        assert np.array_equal(classes.numpy(), IO.first_argmax(lg))
        assert np.array_equal(correct.numpy().astype(np.float64), rr["correct_rows"].numpy())
        assert np.isfinite(loss.numpy()).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["random", "saturated"])
def test_bit_equal_to_the_training_head(cuda, dtype, case):
    """predict's loss_rows / correct_rows are the bits evaluate() leaves in loss_rows() / correct_rows();
    without labels the logits and classes are the same."""
    params, x, y = O.random_case(37) if case == "random" else O.saturated_case(37, "argmin")
    e = _engine(cuda, 64, dtype, params)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd, yd = x.to(cuda), y.to(torch.int32).to(cuda)
        e.evaluate(xd, yd, False)
        loss0, correct0 = e.loss_rows()[:37].clone(), e.correct_rows()[:37].clone()
    torch.cuda.synchronize()
    logits, classes, loss, correct = _predict(e, x, y)
    assert torch.equal(_bits(loss), _bits(loss0.cpu()))
    assert torch.equal(_bits(correct), _bits(correct0.cpu()))
    # the inference head wrote none of the training head's outputs
    assert torch.equal(_bits(e.loss_rows()[:37].cpu()), _bits(loss0.cpu()))
    logits1, classes1, loss1, correct1 = _predict(e, x)
    assert loss1.numel() == 0 and correct1.numel() == 0
    assert torch.equal(_bits(logits1), _bits(logits)) and torch.equal(classes1, classes)
    assert np.array_equal(classes.numpy(), IO.first_argmax(logits.numpy()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logits_against_the_fp64_oracle(cuda, dtype):
    """Dense random cases at B = 1, 3, 63, 65: per-element error relative to the logits' rms within 3x the
    measured worst (infer_oracle.LOGIT_BOUND); the oracle's own logits with one class scaled by 1.02 are
    refused by the same criterion."""
    bound = IO.LOGIT_BOUND[dtype]
    assert bound is not None and 0 < bound < 0.02 / 4
    for B in IO.REL_BATCHES:
        params, x, y = O.random_case(B)
        ref = O.oracle_step(params, x, y, dtype, backward=False)["logits"].numpy()
        e = _engine(cuda, B, dtype, params)
        logits = _predict(e, x)[0].numpy()
        rel = IO.logit_rel(logits, ref)
        print("logits %s B=%d rel %.4e (bound %.4e)" % (dtype, B, rel, bound))
        assert rel <= bound, (dtype, B, rel, bound)
        # the class with the largest logit: 2 % of a logit near zero is no error by a criterion relative
        # to the rms (at B = 1 the smallest class moves by 2.3e-3 rms, the largest by 3.2e-2)
        c = int(np.abs(ref).max(0).argmax())
        bad = ref.copy()
        bad[:, c] *= 1.02
        assert IO.logit_rel(bad, ref) > bound, (dtype, B, c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tails_and_position_independence(cuda, dtype):
    """predict on the first n rows is the first n rows of predict on all 150, for n on both sides of the
    engine's batch of 64, n = 0 and n = 1."""
    params, x, y, ref = IO.spread_integer_case(150)
    e = _engine(cuda, 64, dtype, params)
    full = _predict(e, x, y)
    assert np.array_equal(full[0].numpy().astype(np.float64), ref["logits"].numpy())
    for n in (0, 1, 63, 64, 65, 150):
        part = _predict(e, x[:n], y[:n])
        for a, b in zip(part, full):
            assert torch.equal(_bits(a), _bits(b[:n])), n
        nolab = _predict(e, x[:n])
        assert torch.equal(_bits(nolab[0]), _bits(full[0][:n])) and torch.equal(nolab[1], full[1][:n])


def _rec(t):
    torch.cuda.synchronize()
    assert t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == inference.REC_FIELDS
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_records(cuda, dtype):
    """evaluate_dataset's records: counts and matrix EQUAL the host definitions on the oracle's classes,
    loss_sum the fp64 sum of predict's fp32 rows; eager runs, and a captured graph's replay, are
    bit-identical; a replay after a step reflects the new parameters (and, with EMA, the new averages)."""
    params, x, y, ref = IO.spread_integer_case(150)
    classes = IO.first_argmax(ref["logits"].numpy())
    e = _engine(cuda, 16, dtype, params)
    e.set_ema(0.5, False)
    loss_rows = _predict(e, x, y)[2].numpy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd, yd = x.to(cuda), y.to(torch.int32).to(cuda)
        with pytest.raises(RuntimeError, match="labels must be in"):
            bad = yd.clone()
            bad[77] = 10
            e.set_eval_dataset(xd, bad)
        with pytest.raises(RuntimeError, match="set_eval_dataset first"):
            e.evaluate_dataset(0, 150, 50, False)
        e.set_eval_dataset(xd, yd)
        with pytest.raises(RuntimeError, match="outside the evaluation split"):
            e.evaluate_dataset(100, 51, 50, False)
        a = _rec(e.evaluate_dataset(0, 150, 50, False))   # 3 groups of 50 = chunks 16, 16, 16, 2
        b = _rec(e.evaluate_dataset(7, 100, 100, False))  # 1 group = 6 chunks of 16 and one of 4
        a2 = _rec(e.evaluate_dataset(0, 150, 50, False))
        b2 = _rec(e.evaluate_dataset(7, 100, 100, False))
        assert _rec(e.evaluate_dataset(3, 0, 5, False)).shape == (0, inference.REC_FIELDS)
    yn = y.numpy()
    assert IO.records_match(a, yn, classes, loss_rows, 50) == []
    assert IO.records_match(b, yn[7:107], classes[7:107], loss_rows[7:107], 100) == []
    assert a.shape == (3, 104) and b.shape == (1, 104)
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes()
    # the whole split's matrix: every class predicted, not symmetric (a transposed fold is not this one)
    cm = inference.merge_records([inference.record_from_device(r) for r in a])["confusion"]
    assert (cm.sum(0) > 0).all() and not (cm == cm.T).all()
    with torch.cuda.stream(s):
        e.capture_eval("ev", 0, 150, 50, False)
        e.capture_eval("ev7", 7, 100, 100, False)
        e.capture_eval("ema", 0, 150, 50, True)
        e.replay("ev", 1)
        e.replay("ev7", 1)
        e.replay("ema", 1)
        ga, gb, gm = _rec(e.eval_records("ev")), _rec(e.eval_records("ev7")), _rec(e.eval_records("ema"))
    assert ga.tobytes() == a.tobytes() and gb.tobytes() == b.tobytes()
    assert gm.tobytes() == a.tobytes()  # the shadow still holds the parameters it was started from
    with torch.cuda.stream(s):
        e.feed_x().copy_(xd[:16])
        e.feed_y().copy_(yd[:16])
        e.train_step()
        e.replay("ev", 1)
        e.replay("ema", 1)
        ga1, gm1 = _rec(e.eval_records("ev")), _rec(e.eval_records("ema"))
        ea1 = _rec(e.evaluate_dataset(0, 150, 50, False))
        em1 = _rec(e.evaluate_dataset(0, 150, 50, True))
    assert ga1.tobytes() != ga.tobytes() and ga1.tobytes() == ea1.tobytes()  # the new parameters
    assert gm1.tobytes() != gm.tobytes() and gm1.tobytes() == em1.tobytes()  # the new averages ...
    assert gm1.tobytes() != ga1.tobytes()                                    # ... which are not the parameters
    assert (ga1[:, 1] == 50).all() and (gm1[:, 1] == 50).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("log", [0, 16])
def test_training_state_untouched(cuda, dtype, log):
    """Dataset mode, Adam, dropout: 3 steps, predict + evaluate_dataset with a ragged tail, 3 steps leave
    the bits of 6 straight steps -- parameters, both Adam slots, the bf16 shadow, the step counter (and the
    step log's records)."""
    params, x, y = O.random_case(23, seed=3)
    flat = M.flat_from_dict(params)
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(23, generator=gen).to(torch.int32)
    xe, ye = torch.rand(13, 784, generator=gen), torch.randint(0, 10, (13,), generator=gen, dtype=torch.int32)

    def run(between):
        e = _engine(cuda, 5, dtype, flat, keep=0.75)
        if log:
            e.set_step_log(log)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            e.set_dataset(x.to(cuda), y.to(torch.int32).to(cuda), perm.to(cuda))
            e.set_input_mode(1)
            e.set_eval_dataset(xe.to(cuda), ye.to(cuda))
            for _ in range(3):
                e.train_step()
            if between:
                e.predict(xe.to(cuda), ye.to(cuda), False)
                e.predict(xe[:7].to(cuda).contiguous(), _none(cuda), False)
                rec = e.evaluate_dataset(0, 13, 7, False)  # groups 7 and 6: chunks 5, 2 and 5, 1
                assert tuple(rec.shape) == (2, 104)
            for _ in range(3):
                e.train_step()
        torch.cuda.synchronize()
        out = [e.params(), e.adam_m(), e.adam_v(), e.params_bf16(), e.step_tensor()]
        if log:
            out += list(e.step_log())
        return [_bits(t.cpu().clone()) for t in out]

    straight, mixed = run(False), run(True)
    assert int(straight[4].item()) == 6
    for a, b in zip(straight, mixed):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_runner_parity(cuda, dtype):
    """NativeMnistRunner.evaluate_dataset's counts and matrices equal TorchMnistRunner's on the exact case,
    eagerly and through the captured graph; predict's classes equal too."""
    from tensorflow_distributed_amd.models.mnist_runner import NativeMnistRunner, TorchMnistRunner
    from tensorflow_distributed_amd.training.optimizers import AdamOptimizer

    params, x, y, ref = IO.spread_integer_case(37)
    flat = M.flat_from_dict(params)
    cpu = TorchMnistRunner(16, AdamOptimizer(0.01), keep_prob=1.0)
    cpu.set_params(flat)
    cpu.set_eval_dataset(x, y)
    want = cpu.evaluate_dataset(0, 37, 10)
    assert [r["rows"] for r in want] == [10, 10, 10, 7]
    for use_graph in (False, True):
        nat = NativeMnistRunner(16, AdamOptimizer(0.01), keep_prob=1.0, device=cuda, use_graph=use_graph, dtype=dtype)
        nat.set_params(flat)
        nat.set_eval_dataset(x, y)
        for _ in range(2):  # with use_graph: the capture, then a plain replay
            got = nat.evaluate_dataset(0, 37, 10)
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g["rows"] == w["rows"] and g["correct"] == w["correct"]
                assert np.array_equal(g["confusion"], w["confusion"])
                assert abs(g["loss_sum"] - w["loss_sum"]) <= 1e-3 * abs(w["loss_sum"])
        logits, classes = nat.predict(x)
        assert np.array_equal(classes.cpu().numpy(), cpu.predict(x)[1].numpy())
        assert np.array_equal(logits.cpu().numpy().astype(np.float64), ref["logits"].numpy())
