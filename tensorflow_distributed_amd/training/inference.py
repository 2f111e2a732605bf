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


MC_DROPOUT_KEY = 0x4D43D409  # csrc/mnist_mc.h kMcDropoutKey
MC_MAX_SAMPLES = 4096        # kMcMaxSamples


def mc_dropout_masks(rows: int, samples: int, row0: int, rank: int, seed: int, keep_prob: float) -> np.ndarray:
    """The 0/1 masks ``[rows, samples, 1024]`` (float64) that ``mc_head_kernel`` draws (csrc/mnist_mc.h): hidden
    unit ``u`` of sample ``s`` of global row ``r = row0 + i`` is word ``u % 4`` of the Philox4x32-10 call with
    counter ``(s * 256 + u // 4, r lo, r hi, rank)`` and key ``(seed, MC_DROPOUT_KEY)``; kept iff ``u01 < keep_prob``
    in fp32. The kernel's lane map only decides which lane makes which call."""
    from ..models.mnist_cnn import HID, _philox4x32_10

    r = (np.uint64(row0) + np.arange(rows, dtype=np.uint64))[:, None, None]
    s = np.arange(samples, dtype=np.uint64)[None, :, None]
    g = np.arange(HID // 4, dtype=np.uint64)[None, None, :]
    shape = (rows, samples, HID // 4)
    c0 = np.broadcast_to(s * np.uint64(256) + g, shape)
    c1 = np.broadcast_to(r & np.uint64(0xFFFFFFFF), shape)
    c2 = np.broadcast_to(r >> np.uint64(32), shape)
    c3 = np.full(shape, rank & 0xFFFFFFFF, dtype=np.uint64)
    out = _philox4x32_10((c0, c1, c2, c3), seed & 0xFFFFFFFF, MC_DROPOUT_KEY)
    u = np.stack([(v >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) for v in out], axis=-1)
    return (u < np.float32(keep_prob)).reshape(rows, samples, HID).astype(np.float64)


def mc_dropout_ref(h, W_out, b_out, masks, keep_prob: float, labels=None) -> dict:
    """Monte-Carlo dropout statistics in fp64. ``h`` [rows, 1024] is the hidden layer before its relu, ``masks``
    [rows, T, 1024] the kept units of every sample: ``logits[i, s] = (masks[i, s] * relu(h[i]) / keep_prob) @ W_out
    + b_out``. Returns ``logits`` [rows, T, C], ``mean_prob`` (the mean softmax), ``classes`` (its first maximum),
    ``entropy`` of the mean, ``expected_entropy`` (the mean of the samples' entropies), ``mutual_info`` (their
    difference, BALD), ``var_prob`` (the samples' variance per class, divisor T) and, with labels, ``loss_rows =
    -log mean_prob[label]`` and ``correct_rows``; ``0 log 0 = 0``."""
    h, W, b, mk = (np.asarray(a, dtype=np.float64) for a in (h, W_out, b_out, masks))
    a = mk * (np.maximum(h, 0.0) / float(keep_prob))[:, None, :]
    z = a @ W + b
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)

    def ent(q):
        return -(q * np.log(np.where(q > 0, q, 1.0))).sum(-1)

    pbar = p.mean(1)
    out = {"logits": z, "probs": p, "mean_prob": pbar, "classes": pbar.argmax(1).astype(np.int32), "entropy": ent(pbar),
           "expected_entropy": ent(p).mean(1), "var_prob": ((p - pbar[:, None, :]) ** 2).mean(1)}
    out["mutual_info"] = out["entropy"] - out["expected_entropy"]
    if labels is not None:
        y = _ids(labels, "labels")
        with np.errstate(divide="ignore"):
            out["loss_rows"] = -np.log(pbar[np.arange(len(y)), y])
        out["correct_rows"] = (out["classes"] == y).astype(np.float64)
    return out


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
