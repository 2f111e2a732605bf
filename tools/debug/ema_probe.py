"""Cost of the moving average of the weights in the one-GPU MNIST step (MnistEngine.set_ema).

Times 1000 replayed steps at B=128 of three configurations, bf16 and fp32 dtype:

  off       the default step (EMA off)
  fused     set_ema(decay, num_updates): the optimizer tail updates the shadow from p' in registers
  unfused   EMA off plus one ema_flat launch per step over the whole shadow: the separate pass

All three are captured the same way (100 steps per torch.cuda.graph, the engine launching into the
capturing stream) and timed after bench.py's warm-up protocol (--warmup steps, then untimed replays
until --min_warmup_ms have passed). Every configuration runs in a process of its own under its own
timeout, interleaved over --rounds; the first failure ends the run. `--config X --dtype D` runs one
configuration in this process (what `rocprofv3 --kernel-trace --stats -- python
tools/debug/ema_probe.py --config fused ...` wraps to get the tail kernel's own time). The shadow's
traffic is one 4-B load and one 4-B store per parameter when fused, 26.2 MB, and 12 B per parameter
as a pass of its own, 39.3 MB.

    python tools/debug/ema_probe.py > profiles/ema_step.log
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = ("off", "fused", "unfused")


def run_one(a):
    import torch

    from tensorflow_distributed_amd import _native
    from tensorflow_distributed_amd.models import mnist_cnn as M

    _native.require()
    ops = torch.ops.tfd
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    rows = 8192
    data = torch.rand(rows, 784, device=dev, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=dev, generator=g)
    perm = torch.randperm(rows, device=dev, generator=g).to(torch.int32)
    e = torch.classes.tfd.MnistEngine(a.batch_size, 0, 0.75, 1234, 0)
    e.set_dtype(a.dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    stream = torch.cuda.Stream()
    per_graph = 100
    reps = a.steps // per_graph
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev))  # the reference's N(0,1) init
        e.sync_shadow()
        e.set_dataset(data, labels, perm)
        e.set_input_mode(1)
        if a.config == "fused":
            e.set_ema(a.decay, True)
        shadow = e.params().clone()  # unfused: the caller's own shadow

        def step():
            e.train_step()
            if a.config == "unfused":
                ops.ema_flat(shadow, e.params(), a.decay, True, e.step_tensor(), 0)

        step()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(per_graph):
            step()
    with torch.cuda.stream(stream):
        for _ in range(max(1, a.warmup // per_graph)):
            graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.min_warmup_ms:  # the clock ramp (profiles/warmup_ramp.log)
        with torch.cuda.stream(stream):
            graph.replay()
        torch.cuda.synchronize()
    us = []
    for _ in range(a.repeats):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            ev0.record(stream)
            for _ in range(reps):
                graph.replay()
            ev1.record(stream)
        torch.cuda.synchronize()
        us.append(1e3 * ev0.elapsed_time(ev1) / (reps * per_graph))
    sh = e.ema_params() if a.config == "fused" else shadow
    gap = float((sh - e.params()).abs().max().item())
    loss = float(e.loss_rows().mean().item())
    print("%-8s %-5s B=%d  us/step over %d x %d steps: %s  median %.2f  (step %d, loss %.4g, max |shadow - params| "
          "%.4g)" % (a.config, a.dtype, a.batch_size, a.repeats, reps * per_graph, " ".join("%.2f" % u for u in us),
                     statistics.median(us), int(e.step_tensor().item()), loss, gap), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=CONFIGS, default=None, help="run this one configuration in this process")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--min_warmup_ms", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--rounds", type=int, default=3, help="all configurations, interleaved, this many times")
    ap.add_argument("--timeout", type=float, default=120.0, help="per configuration, seconds")
    a = ap.parse_args()
    if a.config:
        return run_one(a)
    for rnd in range(a.rounds):
        for dtype in ("bf16", "fp32"):
            for cfg in CONFIGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--dtype", dtype,
                       "--batch_size", str(a.batch_size), "--steps", str(a.steps), "--warmup", str(a.warmup),
                       "--min_warmup_ms", str(a.min_warmup_ms), "--repeats", str(a.repeats), "--decay", str(a.decay)]
                try:
                    rc = subprocess.run(cmd, timeout=a.timeout).returncode
                except subprocess.TimeoutExpired:
                    print("%s %s: timed out after %.0f s; stopping" % (cfg, dtype, a.timeout), flush=True)
                    return 124
                if rc != 0:  # nothing more is started on the GPU after a failure
                    print("%s %s: exit status %d; stopping" % (cfg, dtype, rc), flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
