"""Device Monte-Carlo dropout against the fp64 definition: the figure behind MI_ERR_MEASURED in
tests/test_mc_dropout_gpu.py, and the timings of profiles/mc_dropout.log.

    python tools/mc_dropout_rel.py > profiles/mc_dropout_rel.txt     the random case of test_op_random
    python tools/mc_dropout_rel.py --time [--rows 5000 --samples 100] > profiles/mc_dropout.log

The worst-case format bounds the test derives hold for every statistic, but at 1024-term dot products they are too
wide to tell a mutual information from 1.02 times itself; the measured distance (the test takes 3x it) is not.

--time: predict_mc on `rows` random rows at T samples (batch 128, both precisions), and the only route to the same
numbers without the kernel: T train-mode forwards per chunk (MnistEngine.forward(True), which runs head_kernel with its
backward half) with a read-back of the chunk's logits gradient, from which the host would rebuild the softmax.
Medians of 15 windows of 20 calls after 3 warm-up windows (the route: 3 single passes), the device synchronised
around each window. `--time --trace` runs three predict_mc passes per precision and nothing else: the workload of
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mc_dropout_rel.py --time --trace
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensorflow_distributed_amd import _native  # noqa: E402
from tensorflow_distributed_amd.models import mnist_cnn as M  # noqa: E402
from tensorflow_distributed_amd.training import inference as I  # noqa: E402


def random_case():
    """test_op_random's operands"""
    g = np.random.default_rng(5)
    h, W, b = g.standard_normal((5, 1024)), 0.05 * g.standard_normal((1024, 10)), 0.05 * g.standard_normal(10)
    return [a.astype(np.float32) for a in (h, W, b)] + [g.integers(0, 10, 5)]


def rel(dev):
    h, W, b, _ = random_case()
    first = np.floor(h / 2)
    slabs = np.stack([first, h - first]).astype(np.float32)
    p32 = torch.zeros(M.TOTAL)
    p32[M.OFFSETS["out"]:M.OFFSETS["out"] + W.size] = torch.from_numpy(W.reshape(-1))
    p32[M.OFFSETS["out_b"]:M.OFFSETS["out_b"] + 10] = torch.from_numpy(b)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    out = torch.ops.tfd.mnist_mc_head(torch.from_numpy(slabs).to(dev), 5, p32.to(dev), none, 48, 0.75, 11, 0, 0)
    torch.cuda.synchronize()
    ref = I.mc_dropout_ref(slabs.sum(0, dtype=np.float32), W, b, I.mc_dropout_masks(5, 48, 0, 0, 11, 0.75), 0.75)
    print("# %s; mnist_mc_head against mc_dropout_ref, B = 5, T = 48, keep_prob 0.75: max |got - ref|" % torch.cuda.get_device_name(0))
    for k, i in (("mean_prob", 0), ("entropy", 2), ("expected_entropy", 3), ("mutual_info", 4), ("var_prob", 5)):
        print("%s %.4e (smallest reference value %.4e)" % (k, np.abs(out[i].cpu().numpy() - ref[k]).max(), np.abs(ref[k]).min()))


def median_ms(fn, reps=15, warm=3, calls=20):
    """ms per call: `calls` back-to-back calls per timed window (tens of ms), the device synchronised around it"""
    ts = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / calls)
    return float(np.median(ts[warm:])), min(ts[warm:]), max(ts[warm:])


def timing(dev, rows, T, batch=128, trace=False):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(rows, 784, generator=g).to(dev)
    y = torch.randint(0, 10, (rows,), generator=g, dtype=torch.int32).to(dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    flat = M.flat_from_dict({k: 0.05 * v for k, v in M.init_params(7).items()}).to(dev)
    print("# %s; %d rows, T = %d, batch %d; median (min .. max) of 15 windows of 20 calls, ms per call" % (torch.cuda.get_device_name(0), rows, T, batch))
    for dtype in ("bf16", "fp32"):
        e = torch.classes.tfd.MnistEngine(batch, 0, 0.75, 1234, 0)
        e.set_dtype(dtype)
        e.params().copy_(flat)
        e.sync_shadow()
        if trace:  # under a kernel trace: three passes at T, nothing else
            for _ in range(3):
                e.predict_mc(x, y, T, 0.75, 7, False, 0)
            torch.cuda.synchronize()
            continue
        print("%s predict (no dropout)          %.3f (%.3f .. %.3f)" % ((dtype,) + median_ms(lambda: e.predict(x, none, False))))
        for t in sorted({1, 16, T}):
            print("%s predict_mc T=%-4d             %.3f (%.3f .. %.3f)" % ((dtype, t) + median_ms(lambda: e.predict_mc(x, y, t, 0.75, 7, False, 0))))

        def train_head_route():
            whole = rows - rows % batch  # the training forward takes full batches only
            for o in range(0, whole, batch):
                e.feed_x().copy_(x[o:o + batch])
                e.feed_y().copy_(y[o:o + batch])
                for _ in range(T):
                    e.step_tensor().add_(1)  # the training mask follows the step: a new one per pass
                    e.forward(True)
                    e.dlogits().cpu()  # softmax - onehot: what the host would average
        print("%s train-head route, %d rows     %.3f (%.3f .. %.3f)" % ((dtype, rows - rows % batch) + median_ms(train_head_route, reps=3, warm=1, calls=1)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--trace", action="store_true", help="--time: only three predict_mc passes per dtype, for a kernel trace")
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--samples", type=int, default=100)
    a = ap.parse_args()
    _native.require()
    dev = torch.device("cuda", 0)
    timing(dev, a.rows, a.samples, trace=a.trace) if a.time else rel(dev)
