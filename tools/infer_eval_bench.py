"""What device evaluation costs against the host-fed loop: the figures of profiles/infer_eval.log.

5000 validation rows of the synthetic split, engine batch 128, both dtypes, as 50 x 100 and 5 x 1000:

  host-fed   the loop of mnist_single.py / dist_main: per batch ``validation.next_batch`` on the host, the
             upload, ``MnistEngine.evaluate`` and the read-back of its two sums
  device     ``set_eval_dataset`` once (upload), ``capture_eval`` once, then per pass one graph replay, one
             synchronisation and one copy of the records (``NativeMnistRunner.evaluate_dataset``); also the
             same launches eagerly (``use_graph=False``)

Wall time around work that ends in a synchronisation; each pass is repeated and the median, the minimum
and the maximum are printed. ``--trace`` only replays a few passes, for a kernel trace of its own:

    python tools/infer_eval_bench.py > profiles/infer_eval.log
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/infer_eval_bench.py --trace
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensorflow_distributed_amd import _native  # noqa: E402


def _ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true", help="a few device passes only (for a kernel trace)")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args(argv)
    _native.require()
    from tensorflow_distributed_amd.models import mnist_cnn as M
    from tensorflow_distributed_amd.models.mnist_runner import NativeMnistRunner
    from tensorflow_distributed_amd.training.optimizers import AdamOptimizer
    from tensorflow_distributed_amd.utils import input_data

    dev = torch.device("cuda", 0)
    mnist = input_data.read_data_sets("/nonexistent", one_hot=True, seed=0, verbose=False)
    val = mnist.validation
    flat = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(0).items()})
    print("# %s; %d validation rows, engine batch 128; ms per pass: median (min .. max) of %d"
          % (torch.cuda.get_device_name(0), val.num_examples, a.reps))
    for dtype in ("bf16", "fp32"):
        r = NativeMnistRunner(128, AdamOptimizer(0.01), keep_prob=0.75, device=dev, dtype=dtype)
        eager = NativeMnistRunner(128, AdamOptimizer(0.01), keep_prob=0.75, device=dev, dtype=dtype, use_graph=False)
        for q in (r, eager):
            q.set_params(flat)
        t0 = time.perf_counter()
        r.set_eval_dataset(val.images, val.labels)
        upload = 1e3 * (time.perf_counter() - t0)
        eager.set_eval_dataset(val.images, val.labels)
        print("%s upload of the split, once: %.2f ms" % (dtype, upload))
        for batches, size in ((50, 100), (5, 1000)):
            def host():
                correct = 0
                for _ in range(batches):
                    x, y = val.next_batch(size)
                    correct += r.evaluate(x, y)[1]
                return correct

            def device(q=r):
                return sum(rec["correct"] for rec in q.evaluate_dataset(0, batches * size, size))

            if a.trace:
                for _ in range(3):
                    device()
                continue
            t0 = time.perf_counter()
            want = device()  # the first call captures the graph
            first = 1e3 * (time.perf_counter() - t0)
            assert host() == want == device(eager), "the three passes count the same rows correct"
            h, g, e = _ms(host, a.reps), _ms(device, a.reps), _ms(lambda: device(eager), a.reps)
            tag = "%s %d x %d" % (dtype, batches, size)
            print("%s host-fed evaluate() loop:        %8.3f ms (%.3f .. %.3f)" % ((tag,) + h))
            print("%s device, one graph replay + read: %8.3f ms (%.3f .. %.3f); first call with the capture %.2f ms"
                  % ((tag,) + g + (first,)))
            print("%s device, eager launches + read:   %8.3f ms (%.3f .. %.3f)" % ((tag,) + e), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
