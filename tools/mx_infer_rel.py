"""Block-scaled inference of fc1 (csrc/mnist_mx.h): the timings of profiles/mx_infer.log and the deviations of
profiles/mx_infer_rel.txt.

    python tools/mx_infer_rel.py [--rows 5000 --batch 128]      predict in bf16 / mxfp8 / mxfp4, alternating: median
        (min .. max) of 15 windows of 20 calls after 3 warm-up windows, the device synchronised around each window;
        then the worst logit deviation of the MX formats from the bf16 predict, and the packed bytes
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mx_infer_rel.py --trace [--rows R --batch B]
        five predict passes per format and nothing else: the workload of a kernel trace of its own
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
from tensorflow_distributed_amd.training import mx_quant as Q  # noqa: E402


def window_ms(fn, calls=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--trace", action="store_true", help="five predict passes per format, for a kernel trace")
    a = ap.parse_args()
    _native.require()
    dev = torch.device("cuda", 0)
    x = torch.rand(a.rows, 784, generator=torch.Generator().manual_seed(0)).to(dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    e = torch.classes.tfd.MnistEngine(a.batch, 0, 1.0, 1, 0)
    e.params().copy_(M.flat_from_dict({k: 0.05 * v for k, v in M.init_params(7).items()}).to(dev))
    e.sync_shadow()
    if a.trace:
        for fmt in Q.INFER_FORMATS:
            e.set_infer_format(fmt)
            for _ in range(5):
                e.predict(x, none, False)
        torch.cuda.synchronize()
        return
    print("# %s; predict on %d rows at batch %d; median (min .. max) of 15 windows of 20 calls, ms per call"
          % (torch.cuda.get_device_name(0), a.rows, a.batch))
    ts, logits = {f: [] for f in Q.INFER_FORMATS}, {}
    for i in range(18):  # the formats alternate window by window; the first 3 windows of each warm up
        for fmt in Q.INFER_FORMATS:
            e.set_infer_format(fmt)
            ts[fmt].append(window_ms(lambda: e.predict(x, none, False)))
    for fmt in Q.INFER_FORMATS:
        e.set_infer_format(fmt)
        logits[fmt] = e.predict(x, none, False)[0].double().cpu().numpy()
        t = ts[fmt][3:]
        print("%-5s %.3f (%.3f .. %.3f)" % (fmt, float(np.median(t)), min(t), max(t)))
    rms = float(np.sqrt((logits["bf16"] ** 2).mean()))
    w1 = e.params()[M.OFFSETS["wd1"]:M.OFFSETS["wd1"] + M.FEAT * M.HID].view(M.FEAT, M.HID)
    for fmt in Q.MX_FORMATS:
        d = float(np.abs(logits[fmt] - logits["bf16"]).max())
        agree = float((logits[fmt].argmax(1) == logits["bf16"].argmax(1)).mean())
        print("%s: worst |logit - bf16 logit| %.4e = %.4f of the logits' rms %.4f (random parameters); classes agree on %.4f "
              "of the rows; packed %d bytes" % (fmt, d, d / rms, rms, agree, torch.ops.tfd.mx_pack_fc1(w1, fmt).numel()))


if __name__ == "__main__":
    main()
