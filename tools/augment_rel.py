"""tfd::augment_batch against the fp64 reference: the figures behind tests/test_augment_gpu.py's bound.

1. "sincos": the one constant of the bound that no number format gives, the error of the device sincosf,
   measured through the op. Rotation only (15 degrees), on two ramp images, pixel = c / 32 and pixel =
   r / 32: bilinear sampling reproduces a ramp, so 32 * out is the source coordinate the kernel formed
   wherever all four taps lie inside the image. Its distance from the fp64 coordinate, over (|dy| + |dx|)
   -- the factor sin and cos enter a coordinate with -- bounds the sincosf error from above (it holds the
   coordinate's own roundings too); taken where |dy| + |dx| >= 13.5, so that those do not dominate. The
   test uses 3 x this figure.
2. Per config of the test: the worst |got - ref| over the test's shapes and data, beside the bound.

    python tools/augment_rel.py > profiles/augment_rel.txt
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tensorflow_distributed_amd import _native  # noqa: E402
from tensorflow_distributed_amd.training import augment as A  # noqa: E402


def sincos_error(dev, samples=512):
    import test_augment_gpu as T

    r, c = np.meshgrid(np.arange(28.0), np.arange(28.0), indexing="ij")
    x = np.stack([c.reshape(-1) / 32.0, r.reshape(-1) / 32.0]).astype(np.float32)  # row 0: x ramp, row 1: y ramp
    y, perm = np.zeros(2, np.int32), np.arange(2, dtype=np.int32)
    cfg = (0.0, 15.0, 0.0, 0.0, 0.0)
    got = T._op(dev, x, y, perm, 0, samples, cfg)[0].cpu().numpy().astype(np.float64).reshape(samples, 28, 28) * 32.0
    ys, xs = A.source_coords(A.augment_config(*cfg), A.native_augment_draws(samples, 0, T.RANK, T.SEED))
    inside = (ys >= 0) & (ys <= 27) & (xs >= 0) & (xs <= 27)
    arm = np.abs(r - A.CTR) + np.abs(c - A.CTR)
    ref = np.where((np.arange(samples) % 2 == 0)[:, None, None], xs, ys)  # sample i reads row i % 2
    err = np.where(inside & (arm >= 13.5)[None], np.abs(got - ref) / arm[None], 0.0)
    return err.max(), int((inside & (arm >= 13.5)[None]).sum())


def main():
    _native.require()
    import test_augment_gpu as T

    dev = torch.device("cuda", 0)
    print("# %s; tfd::augment_batch against training/augment.py (fp64)" % torch.cuda.get_device_name(0))
    e, cnt = sincos_error(dev)
    print("sincos %.3e   # worst coordinate error / (|dy| + |dx|), rotation only, %d pixels; the test uses 3 x" % (e, cnt))
    print("# config worst|got - ref| bound")
    for name in sorted(T.CONFIGS):
        cfg, worst = T.CONFIGS[name], 0.0
        for B, n, step in ((1, 7, 0), (3, 7, 5), (65, 97, 2 ** 33 + 3)):
            x, y, perm = T.dataset(n)
            got = T._op(dev, x, y, perm, step, B, cfg)[0].cpu().numpy().astype(np.float64)
            ref = A.augment_batch_ref(x, y, perm, step, B, T.SEED, T.RANK, A.augment_config(*cfg))[0]
            worst = max(worst, float(np.abs(got - ref).max()))
        print("%s %.3e %.3e" % (name, worst, T.bound(cfg)))


if __name__ == "__main__":
    main()
