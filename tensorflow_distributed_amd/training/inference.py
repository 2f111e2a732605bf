"""Evaluation records and confusion matrices: the fp64 / integer definitions.

What the device computes in ``csrc/kernels/mnist_infer.hip`` (``eval_reduce_kernel``) is defined here
on the host, in numpy: the CPU runner evaluates through these functions, the drivers print from their
results, and the GPU tests hold the device records against them.

A confusion matrix ``cm`` is int64 ``[10, 10]``; ``cm[t, p]`` counts the rows with label ``t`` that
were predicted ``p``. A record is ``{"loss_sum", "rows", "correct", "confusion"}``. The predicted
class of a row is the FIRST maximum of its logits (numpy's ``argmax``, the kernels' strict ``>`` in
class order).
"""
from __future__ import annotations

import numpy as np

NCLS = 10
REC_FIELDS = 4 + NCLS * NCLS  # the device record: {loss_sum, rows, correct, 0, cm[10][10]} in fp64


def _ids(a, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError(f"{what}: a 1-d array of class ids, got shape {a.shape}")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: integer class ids, got {a.dtype}")
    return a.astype(np.int64)


def confusion_matrix(labels, classes, num_classes: int = NCLS) -> np.ndarray:
    """``cm[t, p]`` = number of rows with label ``t`` predicted ``p`` (int64 ``[C, C]``)."""
    t, p = _ids(labels, "labels"), _ids(classes, "classes")
    if t.shape != p.shape:
        raise ValueError(f"labels {t.shape} and classes {p.shape} differ in length")
    for name, a in (("labels", t), ("classes", p)):
        if a.size and (a.min() < 0 or a.max() >= num_classes):
            raise ValueError(f"{name} outside [0, {num_classes})")
    return np.bincount(t * num_classes + p, minlength=num_classes * num_classes).reshape(num_classes, num_classes)


def eval_record(logits, labels) -> dict:
    """The record of one group of rows from its logits ``[n, C]`` and labels ``[n]``, in fp64: the sum of
    ``logsumexp(logits) - logits[label]``, the rows, the rows whose first-maximum class is the label,
    and the confusion matrix."""
    z = np.asarray(logits, dtype=np.float64)
    if z.ndim != 2:
        raise ValueError(f"logits: [n, C], got shape {z.shape}")
    y = _ids(labels, "labels")
    if y.shape[0] != z.shape[0]:
        raise ValueError(f"{z.shape[0]} rows of logits, {y.shape[0]} labels")
    n, c = z.shape
    classes = z.argmax(1) if n else np.zeros(0, np.int64)
    cm = confusion_matrix(y, classes, c)
    if n:
        mx = z.max(1)
        lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
        loss = float((lse - z[np.arange(n), y]).sum())
    else:
        loss = 0.0
    return {"loss_sum": loss, "rows": int(n), "correct": int(np.trace(cm)), "confusion": cm}


def record_from_device(rec) -> dict:
    """One fp64 ``[104]`` device record as a record dict (the counts are exact in fp64)."""
    r = np.asarray(rec, dtype=np.float64)
    if r.shape != (REC_FIELDS,):
        raise ValueError(f"a device record has {REC_FIELDS} fields, got shape {r.shape}")
    return {"loss_sum": float(r[0]), "rows": int(r[1]), "correct": int(r[2]),
            "confusion": np.rint(r[4:]).astype(np.int64).reshape(NCLS, NCLS)}


def merge_records(records) -> dict:
    """The record of all the rows of ``records``."""
    records = list(records)
    cm = sum((np.asarray(r["confusion"], dtype=np.int64) for r in records), np.zeros((NCLS, NCLS), np.int64))
    return {"loss_sum": float(sum(r["loss_sum"] for r in records)), "rows": int(sum(r["rows"] for r in records)),
            "correct": int(sum(r["correct"] for r in records)), "confusion": cm}


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    out = np.full(num.shape, np.nan, dtype=np.float64)
    np.divide(num, den, out=out, where=den > 0)
    return out


def per_class_recall(cm) -> np.ndarray:
    """``cm[c, c] / sum(cm[c, :])``; NaN for a class with no rows."""
    cm = np.asarray(cm, dtype=np.float64)
    return _ratio(np.diag(cm).copy(), cm.sum(1))


def per_class_precision(cm) -> np.ndarray:
    """``cm[c, c] / sum(cm[:, c])``; NaN for a class never predicted."""
    cm = np.asarray(cm, dtype=np.float64)
    return _ratio(np.diag(cm).copy(), cm.sum(0))


def format_confusion(cm) -> str:
    """The matrix as text: a row per label, a column per predicted class, then recall and precision."""
    cm = np.asarray(cm, dtype=np.int64)
    c = cm.shape[0]
    w = max(6, len(str(int(cm.max()) if cm.size else 0)) + 1)
    lines = ["Confusion matrix (rows: label, columns: predicted)",
             " " * 6 + "".join(f"{p:>{w}d}" for p in range(c)) + f"{'total':>{w + 2}}"]
    for t in range(c):
        lines.append(f"{t:>4d} |" + "".join(f"{int(v):>{w}d}" for v in cm[t]) + f"{int(cm[t].sum()):>{w + 2}d}")
    lines.append("total " + "".join(f"{int(v):>{w}d}" for v in cm.sum(0)) + f"{int(cm.sum()):>{w + 2}d}")

    def fmt(v):
        return "".join(f"{'-':>{w}}" if np.isnan(x) else f"{x:>{w}.3f}" for x in v)

    lines.append("recall" + fmt(per_class_recall(cm)))
    lines.append("precis" + fmt(per_class_precision(cm)))
    return "\n".join(lines)
