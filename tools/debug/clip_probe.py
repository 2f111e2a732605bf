"""Cost of global-norm clipping in the one-GPU MNIST step (MnistEngine.set_clip_norm).

Times 1000 replayed steps at B=128 of three configurations, bf16 and fp32 dtype:

  fused     the default step (one optimizer kernel that also reduces the conv slabs)
  unfused   set_fused_tail(0): slab reduce + flat Adam -- the schedule the clipped step extends
  clipped   set_clip_norm(c): unfused + the two norm launches, Adam from the clip instantiation

after bench.py's warm-up protocol (--warmup steps, then untimed replays until --min_warmup_ms have
passed). Every configuration runs in a process of its own under its own timeout, one after the other;
the first failure ends the run. `--config X --dtype D` runs one configuration in this process (what
`rocprofv3 --kernel-trace --stats -- python tools/debug/clip_probe.py --config clipped ...` wraps to get
the two norm kernels' times). Stage 1's byte floor is the gradient buffer read once: 13.1 MB fp32.

    python tools/debug/clip_probe.py > profiles/clip_norm_step.log
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = ("fused", "unfused", "clipped")


def run_one(a):
    import torch

    from tensorflow_distributed_amd import _native
    from tensorflow_distributed_amd.models import mnist_cnn as M

    _native.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    rows = 8192
    data = torch.rand(rows, 784, device=dev, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=dev, generator=g)
    perm = torch.randperm(rows, device=dev, generator=g).to(torch.int32)
    e = torch.classes.tfd.MnistEngine(a.batch_size, 0, 0.75, 1234, 0)
    e.set_dtype(a.dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    if a.config != "fused":
        e.set_fused_tail(0)
    if a.config == "clipped":
        e.set_clip_norm(a.clip_norm)
    stream = torch.cuda.Stream()
    per_graph = 100
    reps = a.steps // per_graph
    with torch.cuda.stream(stream):
        e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev))  # the reference's N(0,1) init
        e.sync_shadow()
        e.set_dataset(data, labels, perm)
        e.set_input_mode(1)
        e.train_step()
        e.capture_train_steps("g", per_graph)
        for _ in range(max(1, a.warmup // per_graph)):
            e.replay("g", 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.min_warmup_ms:  # the clock ramp (profiles/warmup_ramp.log)
        with torch.cuda.stream(stream):
            e.replay("g", 1)
        torch.cuda.synchronize()
    us = []
    for _ in range(a.repeats):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            ev0.record(stream)
            e.replay("g", reps)
            ev1.record(stream)
        torch.cuda.synchronize()
        us.append(1e3 * ev0.elapsed_time(ev1) / (reps * per_graph))
    norm, scale = e.grad_norm().tolist()
    loss = float(e.loss_rows().mean().item())
    print("%-8s %-5s B=%d  us/step over %d x %d steps: %s  median %.2f  (step %d, loss %.4g, grad_norm %.6g, "
          "clip_scale %.6g)" % (a.config, a.dtype, a.batch_size, a.repeats, reps * per_graph,
                                " ".join("%.2f" % u for u in us), statistics.median(us),
                                int(e.step_tensor().item()), loss, norm, scale), flush=True)
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
    ap.add_argument("--clip_norm", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=2, help="all configurations, interleaved, this many times")
    ap.add_argument("--timeout", type=float, default=120.0, help="per configuration, seconds")
    a = ap.parse_args()
    if a.config:
        return run_one(a)
    for rnd in range(a.rounds):
        for dtype in ("bf16", "fp32"):
            for cfg in CONFIGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--dtype", dtype,
                       "--batch_size", str(a.batch_size), "--steps", str(a.steps), "--warmup", str(a.warmup),
                       "--min_warmup_ms", str(a.min_warmup_ms), "--repeats", str(a.repeats),
                       "--clip_norm", str(a.clip_norm)]
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
