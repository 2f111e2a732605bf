"""Inference without a GPU: the fp64 / integer definitions of training/inference.py, the CPU runner's
predict / evaluate_dataset over them, the drivers' --device_eval / --confusion_matrix and the
``python -m tensorflow_distributed_amd.predict`` tool, and a numpy model of the device fold that shows the
GPU tests' criteria (infer_oracle.records_match) name a transposed matrix, a dropped tail chunk and an
ADD where a STORE belongs."""
import re

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
from tensorflow_distributed_amd.training import checkpoint, inference
from tensorflow_distributed_amd.training.optimizers import AdamOptimizer

import infer_oracle as IO


# ---------------------------------------------------------------- the definitions
def test_confusion_matrix_by_hand():
    cm = inference.confusion_matrix([0, 0, 1, 2, 2, 2], [0, 1, 1, 0, 2, 2], 3)
    assert cm.dtype == np.int64 and cm.tolist() == [[1, 1, 0], [0, 1, 0], [1, 0, 2]]
    assert cm[0, 1] == 1 and cm[1, 0] == 0  # [label][predicted], not the transpose
    assert inference.confusion_matrix([], []).shape == (10, 10) and inference.confusion_matrix([], []).sum() == 0
    for bad in (([10], [0]), ([0], [-1]), ([0, 1], [0]), ([0.5], [0])):
        with pytest.raises(ValueError):
            inference.confusion_matrix(*bad)


def test_recall_and_precision_with_an_empty_class_and_with_one_class_only():
    cm = np.zeros((10, 10), np.int64)
    cm[0, 0], cm[0, 1], cm[1, 1], cm[2, 1] = 3, 1, 2, 4  # class 2 is never predicted, classes 3.. have no rows
    rec, pre = inference.per_class_recall(cm), inference.per_class_precision(cm)
    assert rec[0] == 0.75 and rec[1] == 1.0 and rec[2] == 0.0 and np.isnan(rec[3:]).all()
    assert pre[0] == 1.0 and pre[1] == 2 / 7 and np.isnan(pre[2:]).all()
    one = inference.confusion_matrix([4] * 6, [4] * 6)  # all one class
    assert one.sum() == 6 and one[4, 4] == 6
    assert inference.per_class_recall(one)[4] == 1.0 and np.isnan(np.delete(inference.per_class_recall(one), 4)).all()
    text = inference.format_confusion(cm)
    assert len(text.splitlines()) == 15 and "recall" in text and "-" in text.splitlines()[-1]


def test_eval_record_ties_take_the_first_maximum():
    logits = np.array([[1.0, 3.0, 3.0] + [0.0] * 7,     # tie between 1 and 2: predicted 1
                       [2.0] * 10,                      # all tied: predicted 0
                       [0.0] * 9 + [5.0]])
    r = inference.eval_record(logits, [2, 0, 9])
    assert r["rows"] == 3 and r["correct"] == 2
    assert r["confusion"][2, 1] == 1 and r["confusion"][0, 0] == 1 and r["confusion"][9, 9] == 1
    z = logits.astype(np.float64)
    want = sum(np.log(np.exp(z[i]).sum()) - z[i, y] for i, y in enumerate([2, 0, 9]))
    assert abs(r["loss_sum"] - want) <= 1e-12 * want
    empty = inference.eval_record(np.zeros((0, 10)), [])
    assert empty["rows"] == 0 and empty["loss_sum"] == 0.0 and empty["confusion"].sum() == 0
    both = inference.merge_records([r, r])
    assert both["rows"] == 6 and both["correct"] == 4 and (both["confusion"] == 2 * r["confusion"]).all()
    dev = np.concatenate([[r["loss_sum"], 3.0, 2.0, 0.0], r["confusion"].reshape(-1).astype(np.float64)])
    back = inference.record_from_device(dev)
    assert back["rows"] == 3 and back["correct"] == 2 and (back["confusion"] == r["confusion"]).all()


# ---------------------------------------------------------------- the CPU runner
def test_cpu_runner_predicts_and_evaluates_by_the_definitions():
    params, x, y, ref = IO.spread_integer_case(37)
    r = TorchMnistRunner(16, AdamOptimizer(0.01), keep_prob=0.75)
    r.set_params(M.flat_from_dict(params))
    logits, classes = r.predict(x)
    lg = ref["logits"].numpy()
    assert logits.dtype == torch.float32 and classes.dtype == torch.int32
    assert np.array_equal(logits.numpy().astype(np.float64), lg)  # integers: exact; no dropout at keep_prob 0.75
    assert np.array_equal(classes.numpy(), IO.first_argmax(lg))
    assert tuple(r.predict(x[:0])[0].shape) == (0, 10) and r.predict(x[:0])[1].numel() == 0
    with pytest.raises(ValueError, match="set_eval_dataset first"):
        r.evaluate_dataset()
    bad = y.clone()
    bad[3] = 10
    with pytest.raises(ValueError, match="labels must be in"):
        r.set_eval_dataset(x, bad)
    r.set_eval_dataset(x, y)
    with pytest.raises(ValueError, match="outside the evaluation split"):
        r.evaluate_dataset(30, 8, 4)
    recs = r.evaluate_dataset(0, 37, 10)
    assert [q["rows"] for q in recs] == [10, 10, 10, 7]
    for i, q in enumerate(recs):
        want = inference.eval_record(lg[10 * i:10 * i + 10], y.numpy()[10 * i:10 * i + 10])
        assert q["correct"] == want["correct"] and (q["confusion"] == want["confusion"]).all()
        assert q["correct"] == int(ref["correct_rows"][10 * i:10 * i + 10].sum())
        assert abs(q["loss_sum"] - want["loss_sum"]) <= 1e-6 * want["loss_sum"]
    whole = r.evaluate_dataset()
    assert len(whole) == 1 and whole[0]["rows"] == 37
    assert (whole[0]["confusion"] == inference.merge_records(recs)["confusion"]).all()
    assert [q["rows"] for q in r.evaluate_dataset(7, 12, 5)] == [5, 5, 2] and r.evaluate_dataset(5, 0, 3) == []


# ---------------------------------------------------------------- the model of the device fold
def _fold_case():
    params, x, y, ref = IO.spread_integer_case(150)
    classes = IO.first_argmax(ref["logits"].numpy())
    loss = ref["loss_rows"].numpy().astype(np.float32)
    correct = ref["correct_rows"].numpy().astype(np.float32)
    return y.numpy(), classes, loss, correct


def test_fold_model_passes_the_gpu_tests_criteria():
    y, classes, loss, correct = _fold_case()
    for chunk, group, first, count in ((16, 50, 0, 150), (16, 100, 7, 100), (64, 150, 0, 150), (5, 7, 0, 13)):
        sl = slice(first, first + count)
        rec = IO.reduce_model(y[sl], classes[sl], loss[sl], correct[sl], chunk, group)
        assert IO.records_match(rec, y[sl], classes[sl], loss[sl], group) == []


@pytest.mark.parametrize("fault,word", [("transpose", "confusion matrix differs"), ("drop_tail", "rows"),
                                        ("add_first", "not finite")])
def test_the_criteria_name_each_fault_of_the_fold(fault, word):
    """evaluate_dataset(0, 150, 50) at batch 16 (chunks 16, 16, 16, 2 per group) and (7, 100, 100), the GPU
    test's calls: each fault is refused, by the complaint that names it."""
    y, classes, loss, correct = _fold_case()
    for chunk, group, first, count in ((16, 50, 0, 150), (16, 100, 7, 100)):
        sl = slice(first, first + count)
        rec = IO.reduce_model(y[sl], classes[sl], loss[sl], correct[sl], chunk, group, fault=fault)
        complaints = IO.records_match(rec, y[sl], classes[sl], loss[sl], group)
        assert complaints and any(word in c for c in complaints), complaints


# ---------------------------------------------------------------- the drivers
def _with_flags(argv, fn):
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog"] + argv)
        return fn(dist_main)
    finally:
        F.FLAGS.reset()


def test_device_eval_flag_combinations():
    _with_flags([], lambda d: d.check_device_eval_flags(2))
    _with_flags(["--device_eval"], lambda d: d.check_device_eval_flags(2))
    _with_flags(["--device_eval", "--confusion_matrix", "--job_name=ps"], lambda d: d.check_device_eval_flags(2))
    _with_flags(["--device_eval", "--replicas_to_aggregate=1", "--ps_hosts="], lambda d: d.check_device_eval_flags(2))
    for argv, word in ((["--confusion_matrix"], "--confusion_matrix without --device_eval"),
                       (["--device_eval", "--model=resnet18"], "--device_eval with --model resnet18"),
                       (["--device_eval", "--sync_replicas=False"], "--device_eval in the parameter-server role"),
                       (["--device_eval", "--replicas_to_aggregate=1"], "--device_eval in the parameter-server role")):
        with pytest.raises(ValueError, match=word):
            _with_flags(argv, lambda d: d.check_device_eval_flags(2))


@pytest.mark.parametrize("extra,word", [(["--confusion_matrix"], "confusion_matrix without --device_eval"),
                                        (["--device_eval", "--model=resnet18"], "device_eval with --model resnet18")])
def test_flag_errors_come_before_any_worker_starts(monkeypatch, extra, word):
    from tensorflow_distributed_amd.parallel import cluster
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    def no_server(*a, **k):
        raise AssertionError("a Server was built before the flag check")

    monkeypatch.setattr(cluster, "Server", no_server)
    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog", "--synthetic_data", "--data_dir=/nonexistent", "--job_name=worker", "--task_index=0"] + extra)
        with pytest.raises(ValueError, match=word):
            dist_main.main()
    finally:
        F.FLAGS.reset()


def test_mnist_single_device_eval_on_the_cpu(capsys, tmp_path):
    import mnist_single

    with pytest.raises(SystemExit):
        mnist_single.main(["--cpu", "--confusion_matrix"])
    assert "--confusion_matrix" in capsys.readouterr().err
    argv = ["--cpu", "--batch_size", "8", "--training_iters", "32", "--display_step", "2", "--data_dir", str(tmp_path / "none")]
    assert mnist_single.main(argv) == 0
    host = capsys.readouterr().out
    assert mnist_single.main(argv + ["--device_eval", "--confusion_matrix"]) == 0
    dev = capsys.readouterr().out
    mean = [re.search(r"^Mean Accuracy : (\d\.\d{6})$", o, re.M).group(1) for o in (host, dev)]
    assert mean[0] == mean[1]  # 50 x 100 is the whole validation split: the order of the rows does not matter
    assert "Confusion matrix" not in host
    rows = [ln for ln in dev.splitlines() if re.match(r"^\s+\d \|", ln)]
    assert len(rows) == 10
    cells = np.array([[int(v) for v in ln.split("|")[1].split()] for ln in rows])
    assert cells.shape == (10, 11) and cells[:, :10].sum() == 5000 and (cells[:, :10].sum(1) == cells[:, 10]).all()
    assert round(np.trace(cells[:, :10]) / 5000.0, 6) == float(mean[1])


def test_predict_tool_round_trip(capsys, tmp_path, monkeypatch):
    from tensorflow_distributed_amd import predict
    from tensorflow_distributed_amd.utils import input_data

    params, _, _, _ = IO.spread_integer_case(37)
    r = TorchMnistRunner(16, AdamOptimizer(0.01, ema_decay=0.9), keep_prob=1.0)
    r.load_flat(M.flat_from_dict(params), {}, 3)
    r.load_ema(M.flat_from_dict({k: -v for k, v in params.items()}))  # averages that predict something else
    logdir, out, data = str(tmp_path / "ckpt"), str(tmp_path / "p.npz"), str(tmp_path / "none")
    checkpoint.Saver().save(logdir, r.state_dict_tf(), global_step=3)
    with pytest.raises(SystemExit):
        predict.main(["--logdir", str(tmp_path / "empty"), "--cpu"])
    capsys.readouterr()
    sets = input_data.read_data_sets(data, one_hot=True, seed=0, verbose=False)
    monkeypatch.setattr(input_data, "read_data_sets", lambda *a, **k: sets)  # built once: the tool only reads it
    val = sets.validation
    x, y = val.images[:64], val.labels[:64].argmax(1)
    for use_ema in (False, True):
        argv = ["--logdir", logdir, "--cpu", "--rows", "64", "--data_dir", data, "--out", out, "--confusion_matrix"]
        assert predict.main(argv + (["--use_ema"] if use_ema else [])) == 0
        text = capsys.readouterr().out
        got = np.load(out)
        logits, classes = r.predict(x, use_ema=use_ema)
        assert got["classes"].dtype == np.int32 and got["logits"].dtype == np.float32
        assert np.array_equal(got["classes"], classes.numpy()) and np.array_equal(got["labels"], y)
        assert np.array_equal(got["logits"], logits.numpy())
        acc = float((classes.numpy() == y).mean())
        assert "Restored" in text and ("Accuracy : %f" % acc) in text and "Confusion matrix" in text
    assert not np.array_equal(r.predict(x)[1].numpy(), r.predict(x, use_ema=True)[1].numpy())
