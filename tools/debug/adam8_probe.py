"""adam8_flat against adam_flat over MNIST's TOTAL (alternated in one process), and the adam8 / unfused Adam / fused
Adam step at B = 128. Writes the log named by its argument (profiles/adam8_step.log). Run from the repository root on the GPU."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tensorflow_distributed_amd import _native  # noqa: E402
from tensorflow_distributed_amd.models import mnist_cnn as M  # noqa: E402

_native.require()
ops, dev, N = torch.ops.tfd, torch.device("cuda", 0), M.TOTAL
out = open(sys.argv[1] if len(sys.argv) > 1 else "adam8_step.log", "w")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def timed(fn, reps=200, rounds=7):
    """median over rounds of the mean us of reps back-to-back launches (events around the batch)"""
    for _ in range(50):
        fn()
    res = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / reps)
    return res


say(f"device {torch.cuda.get_device_name(0)}; n = {N}; us per launch: median of 7 rounds of 200 launches [min .. max]")
gen = torch.Generator(device=dev).manual_seed(0)
p = torch.randn(N, device=dev, generator=gen) * 0.05
pbf = p.to(torch.bfloat16)
m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
m8, am = ops.q8_encode(m, "m")
v8, av = ops.q8_encode(v, "v")
for gdt, b8, b32 in ((torch.float32, 18.06, 30.0), (torch.bfloat16, 16.06, 28.0)):
    g = (torch.randn(N, device=dev, generator=gen) * 0.01).to(gdt)
    fns = {
        "adam_flat": lambda: ops.adam_flat(p, m, v, g, pbf, 1e-3, 0.9, 0.999, 1e-8, None, 1.0, 1, "constant", [], [], []),
        "adam8_flat": lambda: ops.adam8_flat(p, m8, v8, am, av, g, pbf, 1e-3, 0.9, 0.999, 1e-8),
    }
    res = {k: [] for k in fns}
    for _ in range(3):  # alternated
        for k, fn in fns.items():
            res[k] += timed(fn)
    for k, r in res.items():
        med, bpp = statistics.median(r), (b32 if k == "adam_flat" else b8)
        say(f"g {str(gdt).split('.')[-1]:9s} {k:16s} {med:7.2f} us [{min(r):.2f} .. {max(r):.2f}]  {bpp:5.2f} B/param -> "
            f"{N * bpp / med / 1e6:.2f} TB/s")
    say(f"g {str(gdt).split('.')[-1]:9s} time ratio adam8 / adam = "
        f"{statistics.median(res['adam8_flat']) / statistics.median(res['adam_flat']):.3f}; byte ratio {b8 / b32:.3f}")

# ---- step against step at B = 128: 20-step graphs, us per step
B = 128
side = torch.cuda.Stream()
g = torch.Generator().manual_seed(3)
x, y = torch.rand(B, 784, generator=g).to(dev), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32).to(dev)
for dtype in ("bf16", "fp32"):
    engs = {}
    for name in ("adam fused (default)", "adam unfused", "adam8"):
        e = torch.classes.tfd.MnistEngine(B, 0, 0.75, 1, 0)
        e.set_dtype(dtype)
        if name == "adam8":
            e.set_adam8(1e-3, 0.9, 0.999, 1e-8)
        else:
            e.set_adam(1e-3, 0.9, 0.999, 1e-8)
            e.set_fused_tail(1 if "fused (" in name else 0)
        e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev) * 0.05)
        e.sync_shadow()
        e.feed_x().copy_(x)
        e.feed_y().copy_(y)
        with torch.cuda.stream(side):
            e.train_step()
            e.capture_train_steps("g", 20)
        engs[name] = e
    res = {k: [] for k in engs}
    with torch.cuda.stream(side):
        for _ in range(3):
            for k, e in engs.items():
                res[k] += [t / 20 for t in timed(lambda: e.replay("g", 1), reps=10, rounds=5)]
    for k, r in res.items():
        say(f"step {dtype} B=128 {k:22s} {statistics.median(r):7.2f} us/step [{min(r):.2f} .. {max(r):.2f}]")
state = 2 * N + 8 * ((N + 255) // 256)
say(f"optimizer state: adam {8 * N / 1e6:.1f} MB, adam8 {state / 1e6:.1f} MB")
