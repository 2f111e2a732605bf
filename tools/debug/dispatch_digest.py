"""SHA-1 digests of the engine's state over the matrix of optimizer launch variants (csrc/optim_launch.h).

One cell = one MnistEngine at batch 8 over a 64-row synthetic device dataset with a piecewise (non-constant)
learning-rate schedule: 3 eager steps, then 4 steps replayed from a 2-step graph. The matrix is

  {adam, sgd, momentum, rmsprop, centered rmsprop with momentum, adagrad, lamb, lars}
    x every subset of {clip, ema, guard} x {bf16, fp32}

plus adam with the fused one-GPU tail switched off (the flat Adam launch of the plain and EMA rows, which the
fused tail otherwise replaces). With the guard, one image of the batch of step 4 -- inside the replayed graph --
carries an inf pixel, so one step is skipped; the line reports the device counter. Every line gives the SHA-1 of
params, adam_m, adam_v, slot3 and ema_params where they exist; a cell the engine refuses gives the error's
first line instead.

The output is a function of the library alone: run it once per library (TFD_NATIVE_LIB selects one), each run a
process of its own, and compare the outputs.

    python tools/debug/dispatch_digest.py > new.txt
    TFD_NATIVE_LIB=/path/to/parent/_C.so python tools/debug/dispatch_digest.py > parent.txt
"""
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, ROWS, LR = 8, 64, 0.01
EAGER, PER_GRAPH, REPLAYS = 3, 2, 2
POISON_STEP = 4  # the second step of the first replay

OPTIMIZERS = {
    "adam": lambda e: e.set_adam(LR, 0.9, 0.999, 1e-8),
    "adam_unfused": lambda e: (e.set_adam(LR, 0.9, 0.999, 1e-8), e.set_fused_tail(0)),
    "sgd": lambda e: e.set_momentum(LR, 0.0, False),
    "momentum": lambda e: e.set_momentum(LR, 0.9, True),
    "rmsprop": lambda e: e.set_rmsprop(LR, 0.9, 0.0, 1e-10, False),
    "rmsprop_centered_mom": lambda e: e.set_rmsprop(LR, 0.9, 0.9, 1e-6, True),
    "adagrad": lambda e: e.set_adagrad(LR, 0.1),
    "lamb": lambda e: e.set_lamb(LR, 0.9, 0.999, 1e-6, 0.01, True),
    "lars": lambda e: e.set_lars(LR, 0.9, 1e-4, 0.001, 0.0, True),
}
MODS = ("clip", "ema", "guard")


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().view(-1).numpy().tobytes()).hexdigest()


def cell(opt, mods, dtype, ds, dev):
    import torch

    from tensorflow_distributed_amd.models import mnist_cnn as M

    data, labels, perm = ds
    if "guard" in mods:  # identity perm: step s reads rows [s * B, (s + 1) * B)
        data = data.clone()
        data[POISON_STEP * B + 2, 14 * 28 + 14] = float("inf")
    e = torch.classes.tfd.MnistEngine(B, 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    OPTIMIZERS[opt](e)
    e.set_lr_schedule("piecewise", [LR], [1, 4], [LR, LR / 2, LR / 4])
    e.params().copy_(M.flat_from_dict(M.init_params(5)).to(dev) * 0.05)
    e.sync_shadow()
    if "clip" in mods:
        e.set_clip_norm(0.5)
    if "ema" in mods:
        e.set_ema(0.9, True)
    if "guard" in mods:
        e.set_skip_nonfinite(True)
    e.set_dataset(data, labels, perm)
    e.set_input_mode(1)
    for _ in range(EAGER):
        e.train_step()
    e.capture_train_steps("g", PER_GRAPH)
    e.replay("g", REPLAYS)
    torch.cuda.synchronize()
    out = ["step=%d" % int(e.step_tensor().item()), "skipped=%d" % e.skipped_steps(), "params=" + sha(e.params()),
           "adam_m=" + sha(e.adam_m()), "adam_v=" + sha(e.adam_v())]
    if opt == "rmsprop_centered_mom":
        out.append("slot3=" + sha(e.slot3()))
    if "ema" in mods:
        out.append("ema_params=" + sha(e.ema_params()))
    e.drop_graph("g")
    return " ".join(out)


def main():
    import torch

    from tensorflow_distributed_amd import _native

    _native.require()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(3)
    ds = (torch.rand(ROWS, 784, generator=gen).to(dev), torch.randint(0, 10, (ROWS,), dtype=torch.int32, generator=gen).to(dev),
          torch.arange(ROWS, dtype=torch.int32, device=dev))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    refused = 0
    for opt in OPTIMIZERS:
        for k in range(len(MODS) + 1):
            for mods in itertools.combinations(MODS, k):
                for dtype in ("bf16", "fp32"):
                    name = "%-20s %-14s %s" % (opt, "+".join(mods) or "-", dtype)
                    try:
                        with torch.cuda.stream(stream):
                            line = cell(opt, mods, dtype, ds, dev)
                    except RuntimeError as err:
                        if "HIP" in str(err) or "hip" in str(err):  # a device error is no refusal: stop here
                            raise
                        torch.cuda.synchronize()
                        refused += 1
                        line = "REFUSED " + str(err).splitlines()[0]
                    print(name, line, flush=True)
    print("cells %d refused %d" % (len(OPTIMIZERS) * 8 * 2, refused), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
