"""Cases, bounds and host models for the device-inference tests (tests/test_infer_gpu.py,
tests/test_infer_cpu.py, tools/infer_rel.py). A helper module like tests/mnist_oracle.py, which it
builds on.

``spread_integer_case`` is ``mnist_oracle.integer_case`` with the output bias moved so that every
class is predicted: the plain case predicts only two classes, which cannot tell the columns of a
confusion matrix apart. Its logits stay small integers, exact in bf16 and fp32 under any summation
order, so the device logits, classes and records can be compared with ``==``.

``LOGIT_BOUND``: the per-element error of the device logits against the fp64 oracle, relative to the
rms of the oracle's logits, on ``mnist_oracle.random_case`` at B in ``REL_BATCHES``. The bound is 3x
the worst value measured on the MI355X (``tools/infer_rel.py`` -> ``profiles/infer_rel.txt``), the
project's convention.

``reduce_model`` is a numpy model of ``eval_reduce_kernel`` (STORE for a group's first chunk, ADD for
the rest) with three faults that can be switched on; tests/test_infer_cpu.py shows that the criteria of
the GPU tests name each of them.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import mnist_oracle as O
from tensorflow_distributed_amd.training import inference

REL_BATCHES = (1, 3, 63, 65)
# worst max|got - ref| / rms(ref) over REL_BATCHES, measured (profiles/infer_rel.txt)
LOGIT_REL_MEASURED = {"bf16": 9.6097e-04, "fp32": 1.5211e-06}
LOGIT_BOUND = {k: 3.0 * v for k, v in LOGIT_REL_MEASURED.items()}

# properties of spread_integer_case(B) checked on the CPU, in the bf16 and the fp32 rounding of the
# oracle: (rows with a top-two tie, populated matrix cells, row sums that differ from the column sum)
SPREAD_FACTS = {37: (5, 34, 10), 150: (23, 76, 9)}
SPREAD_MAX_LOGIT = 18.0


def first_argmax(logits) -> np.ndarray:
    return np.asarray(logits).argmax(1).astype(np.int64)  # numpy: the first maximum


def _check_spread(B, logits, y):
    """The oracle's own properties: a test on this case cannot pass vacuously."""
    lg = logits.numpy()
    assert (lg == np.rint(lg)).all(), "logits are integers"
    pred = first_argmax(lg)
    counts = np.bincount(pred, minlength=10)
    tied = (lg == lg.max(1, keepdims=True)).sum(1) > 1
    cm = inference.confusion_matrix(y.numpy(), pred)
    assert not (cm == cm.T).all(), "the matrix is not symmetric: a transposed one differs"
    if B >= 37:
        assert (counts > 0).all(), ("every class is predicted", counts)
        assert tied.any(), "rows with a top-two tie"
        # a tied row is labelled with its LAST maximum: a last-maximum argmax would be counted correct
        assert (y.numpy()[tied] != pred[tied]).all()
    if B in SPREAD_FACTS:
        ties, cells, differ = SPREAD_FACTS[B]
        assert np.abs(lg).max() == SPREAD_MAX_LOGIT
        assert int(tied.sum()) == ties and int((cm > 0).sum()) == cells, (int(tied.sum()), int((cm > 0).sum()))
        assert int((cm.sum(0) != cm.sum(1)).sum()) == differ
    if B == 150:
        assert 5 <= counts.min() and counts.max() <= 22, counts


@functools.lru_cache(maxsize=None)
def _spread(B):
    params, x, y = O.integer_case(B)
    lg = O.oracle_step(params, x, y, "fp32", backward=False)["logits"]
    params = dict(params)
    params["out_b"] = params["out_b"] - torch.round(lg.median(0).values).float()
    ref = O.oracle_step(params, x, y, "fp32", backward=False)
    tied = ref["logits"] == ref["logits"].max(1, keepdim=True).values
    y = y.clone()
    for b in (tied.sum(1) > 1).nonzero().reshape(-1).tolist():
        y[b] = int(tied[b].nonzero().max())
    ref = O.oracle_step(params, x, y, "fp32", backward=False)
    for dt in ("fp32", "bf16"):
        r = ref if dt == "fp32" else O.oracle_step(params, x, y, dt, backward=False)
        assert torch.equal(r["logits"], ref["logits"]), "exact in both roundings"
        _check_spread(B, r["logits"], y)
    return params, x, y, ref


def spread_integer_case(B):
    """``(params, x, y, ref)``: ``integer_case(B)`` with ``out_b -= round(per-class median of the oracle's
    logits)``, rows whose top logits tie relabelled with the LAST tied class as ``integer_case`` does, and
    the fp64 oracle's forward (the same in both roundings). Computed once per B and shared: do not write
    to it."""
    return _spread(B)


def logit_rel(got, ref) -> float:
    """max |got - ref| over the elements, relative to the rms of ref."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.sqrt((ref ** 2).mean()), 1e-300))


def reduce_model(labels, classes, loss_rows, correct_rows, chunk, group, fault=None):
    """numpy model of the device fold: rows in groups of ``group``, each group in chunks of ``chunk``,
    one fp64 [104] record per group -- the first chunk STOREs the record, the others ADD to it. The
    records start as NaN: nothing is zeroed beforehand. ``fault``: None, "transpose" (cm[p][t]),
    "drop_tail" (a group's last, shorter chunk is not folded) or "add_first" (ADD where STORE belongs)."""
    labels, classes = np.asarray(labels, np.int64), np.asarray(classes, np.int64)
    loss_rows, correct_rows = np.asarray(loss_rows, np.float32), np.asarray(correct_rows, np.float32)
    n = labels.shape[0]
    ng = (n + group - 1) // group
    rec = np.full((ng, inference.REC_FIELDS), np.nan)
    for gi in range(ng):
        g0, g1 = gi * group, min((gi + 1) * group, n)
        for o in range(g0, g1, chunk):
            e = min(o + chunk, g1)
            if fault == "drop_tail" and o > g0 and e - o < chunk:
                continue
            t, p = (classes, labels) if fault == "transpose" else (labels, classes)
            cm = np.bincount(t[o:e] * 10 + p[o:e], minlength=100).astype(np.float64)
            part = np.concatenate([[loss_rows[o:e].astype(np.float64).sum(), float(e - o),
                                    correct_rows[o:e].astype(np.float64).sum(), 0.0], cm])
            if o == g0 and fault != "add_first":
                rec[gi] = part
            else:
                rec[gi] = rec[gi] + part
    return rec


def records_match(rec, labels, classes, loss_rows, group) -> list:
    """The GPU tests' criteria for a device record array, as a list of complaints (empty: it passes):
    rows, correct and the matrix EQUAL the definitions of training/inference.py on each group's rows;
    loss_sum within 1e-12 relative of the host fp64 sum of the group's fp32 loss rows."""
    labels, classes = np.asarray(labels, np.int64), np.asarray(classes, np.int64)
    bad = []
    n = labels.shape[0]
    if rec.shape[0] != (n + group - 1) // group:
        return [f"{rec.shape[0]} records for {n} rows in groups of {group}"]
    for gi in range(rec.shape[0]):
        g0, g1 = gi * group, min((gi + 1) * group, n)
        if not np.isfinite(rec[gi]).all():
            bad.append(f"group {gi}: a field is not finite")
            continue
        r = inference.record_from_device(rec[gi])
        cm = inference.confusion_matrix(labels[g0:g1], classes[g0:g1])
        if r["rows"] != g1 - g0:
            bad.append(f"group {gi}: rows {r['rows']} != {g1 - g0}")
        if r["correct"] != int(np.trace(cm)):
            bad.append(f"group {gi}: correct {r['correct']} != {int(np.trace(cm))}")
        if not (r["confusion"] == cm).all():
            bad.append(f"group {gi}: confusion matrix differs in {int((r['confusion'] != cm).sum())} cells")
        want = float(np.asarray(loss_rows[g0:g1], np.float64).sum())
        if abs(r["loss_sum"] - want) > 1e-12 * max(abs(want), 1e-300):
            bad.append(f"group {gi}: loss_sum {r['loss_sum']!r} != {want!r}")
        if rec[gi][3] != 0.0:
            bad.append(f"group {gi}: the reserved field is {rec[gi][3]!r}")
    return bad
