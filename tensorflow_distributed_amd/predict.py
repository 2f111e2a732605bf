"""Ask a trained checkpoint what it thinks the images are.

    python -m tensorflow_distributed_amd.predict --logdir DIR [--split validation|test|train] [--use_ema]
        [--dtype bf16|fp32] [--out FILE.npz] [--confusion_matrix] [--data_dir DIR] [--rows N] [--batch_size N] [--cpu]

Restores the latest checkpoint under ``--logdir`` (mnist_single.py --logdir, dist_main's Supervisor),
runs the forward over one split of the data set -- on a GPU through the native engine's inference head
(``MnistEngine.predict`` / ``evaluate_dataset``), otherwise through the fp32 PyTorch runner -- and prints
the accuracy and mean loss and, on request, the confusion matrix with per-class recall and precision.
``--out`` writes ``logits`` [n,10] fp32, ``classes`` [n] int32 and ``labels`` [n] int32 to an npz; the
probabilities are a host softmax of the logits. ``--use_ema`` reads the moving averages the checkpoint
carries (``<var>/ExponentialMovingAverage``).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np
import torch

from .models import mnist_cnn as M
from .models.mnist_runner import EMA_SUFFIX, make_runner
from .training import checkpoint, inference
from .training.optimizers import AdamOptimizer
from .utils import input_data


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m tensorflow_distributed_amd.predict", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--logdir", required=True, help="directory holding the checkpoint to restore")
    ap.add_argument("--split", default="validation", choices=["validation", "test", "train"])
    ap.add_argument("--use_ema", action="store_true", help="predict from the moving averages in the checkpoint")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="GPU compute precision")
    ap.add_argument("--out", default="", help="write logits, classes and labels to this npz")
    ap.add_argument("--confusion_matrix", action="store_true")
    ap.add_argument("--data_dir", default="MNIST_data/")
    ap.add_argument("--batch_size", type=int, default=128, help="rows per forward")
    ap.add_argument("--rows", type=int, default=0, help="only the first N rows of the split (0 = all of it)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the synthetic data set when no IDX files exist")
    ap.add_argument("--cpu", action="store_true", help="force the fp32 PyTorch CPU path")
    a = ap.parse_args(argv)
    if a.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    latest = checkpoint.latest_checkpoint(a.logdir)
    if not latest:
        ap.error("--logdir %s holds no checkpoint" % a.logdir)
    tensors = checkpoint.Saver().restore(latest)
    if a.use_ema and not all(tf_name + EMA_SUFFIX in tensors for _, tf_name, _ in M.PARAM_SPECS):
        ap.error("--use_ema: %s carries no moving averages (train with --ema_decay)" % latest)

    dev = torch.device("cuda", 0) if (torch.cuda.is_available() and not a.cpu) else torch.device("cpu")
    # the optimizer is never applied; with --use_ema its config switches the shadow on so that it is loaded
    opt = AdamOptimizer(0.01, **(dict(ema_decay=0.5, ema_num_updates=False) if a.use_ema else {}))
    runner = make_runner(a.batch_size, opt, dev, keep_prob=1.0, seed=a.seed, use_graph=False, dtype=a.dtype)
    runner.load_state_dict_tf(tensors)
    print("Restored %s (global step %d)%s" % (latest, runner.global_step(), "; predicting from the moving averages"
                                              if a.use_ema else ""))
    split = getattr(input_data.read_data_sets(a.data_dir, one_hot=True, seed=a.seed), a.split)
    images = np.asarray(split.images, dtype=np.float32).reshape(split.num_examples, -1)
    labels = np.asarray(split.labels).argmax(1).astype(np.int32)
    if a.rows > 0:
        images, labels = images[:a.rows], labels[:a.rows]

    runner.set_eval_dataset(images, labels)
    whole = inference.merge_records(runner.evaluate_dataset(0, None, max(len(labels), 1), use_ema=a.use_ema))
    n = whole["rows"]
    print("%s split: %d images, %d correct" % (a.split, n, whole["correct"]))
    print("Accuracy : %f" % (whole["correct"] / float(max(n, 1))))
    print("Mean loss : %f" % (whole["loss_sum"] / float(max(n, 1))))
    if a.confusion_matrix:
        print(inference.format_confusion(whole["confusion"]))
    if a.out:
        logits, classes = runner.predict(images, use_ema=a.use_ema)
        np.savez(a.out, logits=logits.cpu().numpy().astype(np.float32), classes=classes.cpu().numpy().astype(np.int32),
                 labels=labels)
        print("Wrote %s" % a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
