"""Gradient accumulation against one big batch: the figure behind R in tests/test_grad_accum_gpu.py.

K = 4 micro-batches of 32 rows through an accumulating MnistEngine and the same 128 rows through a plain
engine at batch 128 (tests/grad_accum_util.py), both against the fp64 oracle of tests/mnist_oracle.py:
per parameter tensor and dtype the relative L2 errors e_acc (grads() / 4) and e_one, their ratio, and the
worst ratio, which the test's bound is 3x of.

    python tools/grad_accum_rel.py > profiles/grad_accum_err.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tensorflow_distributed_amd import _native  # noqa: E402


def main():
    _native.require()
    import grad_accum_util as U

    dev = torch.device("cuda", 0)
    print("# %s; K = %d micro-batches of %d against one batch of %d, keep_prob 1.0, fp64 oracle at batch %d"
          % (torch.cuda.get_device_name(0), U.K, U.B, U.K * U.B, U.K * U.B))
    print("# dtype tensor e_acc e_one e_acc/e_one")
    worst = 0.0
    for dtype in ("bf16", "fp32"):
        e_acc, e_one, _ = U.accum_vs_one(dev, dtype)
        for k in e_acc:
            r = e_acc[k] / e_one[k]
            worst = max(worst, r)
            print("%s %-5s %.4e %.4e %.4f" % (dtype, k, e_acc[k], e_one[k], r), flush=True)
    print("worst e_acc/e_one %.4f" % worst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
