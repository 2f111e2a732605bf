"""Device logits against the fp64 oracle: the figures behind LOGIT_BOUND in tests/infer_oracle.py.

MnistEngine.predict on mnist_oracle.random_case(B) for B in infer_oracle.REL_BATCHES (an engine of that
batch, both dtypes) against mnist_oracle.oracle_step(..., dtype, backward=False)["logits"]: per case the
largest |got - ref| relative to the rms of the oracle's logits, and the worst per dtype, which the test's
bound is 3x of.

    python tools/infer_rel.py > profiles/infer_rel.txt
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
    import infer_oracle as IO
    import mnist_oracle as O
    from tensorflow_distributed_amd.models import mnist_cnn as M

    dev = torch.device("cuda", 0)
    print("# %s; predict() logits against the fp64 oracle, random_case(B), max|got - ref| / rms(ref)"
          % torch.cuda.get_device_name(0))
    print("# dtype B rel")
    none = torch.empty(0, dtype=torch.int32, device=dev)
    for dtype in ("bf16", "fp32"):
        worst = 0.0
        for B in IO.REL_BATCHES:
            params, x, y = O.random_case(B)
            ref = O.oracle_step(params, x, y, dtype, backward=False)["logits"]
            eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 1234, 0)
            eng.set_dtype(dtype)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                eng.params().copy_(M.flat_from_dict(params).to(dev))
                eng.sync_shadow()
                logits = eng.predict(x.to(dev), none, False)[0]
            torch.cuda.synchronize()
            r = IO.logit_rel(logits.cpu().numpy(), ref.numpy())
            worst = max(worst, r)
            print("%s %d %.4e" % (dtype, B, r), flush=True)
        print("worst %s %.4e" % (dtype, worst), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
