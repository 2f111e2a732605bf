"""Cost of gradient accumulation in the one-GPU MNIST step (MnistEngine.set_grad_accum).

Times replayed optimizer steps at B=128, bf16 and fp32 dtype, of

  fused     the default step (one optimizer kernel that also reduces the conv slabs)
  unfused   set_fused_tail(0): slab reduce + flat Adam -- the kernels a micro-batch runs
  k1        set_grad_accum(1): the default step again (accumulation off)
  k2 k4 k8  set_grad_accum(K): K micro-batches of B, K - 1 of them with the grad_accum pass in place of
            the optimizer pass, the last with both

after bench.py's warm-up protocol (--warmup steps, then untimed replays until --min_warmup_ms have
passed). Every configuration runs in a process of its own under its own timeout, one after the other,
all of them --rounds times (interleaved arms); the first failure ends the run. The pass/fail line: a k4
step must cost less than 4 unfused steps of the same run (medians over the rounds).

`--config kernel` times the grad_accum kernel alone on M.TOTAL fp32 elements -- the three modes, the
blocks x loads-in-flight grid of the A/B, achieved bytes/s -- beside adam_flat on buffers of the same size.

    python tools/debug/accum_probe.py > profiles/grad_accum_step.log
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = ("fused", "unfused", "k1", "k2", "k4", "k8")


def run_step(a):
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
    K = 1
    if a.config == "unfused":
        e.set_fused_tail(0)
    elif a.config.startswith("k"):
        K = int(a.config[1:])
    stream = torch.cuda.Stream()
    per_graph = max(1, 100 // K)
    reps = max(1, a.steps // K // per_graph)
    with torch.cuda.stream(stream):
        e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev))  # the reference's N(0,1) init
        e.sync_shadow()
        e.set_dataset(data, labels, perm)
        e.set_input_mode(1)
        if a.config.startswith("k"):
            e.set_grad_accum(K)
        e.train_step()
        e.capture_train_steps("g", per_graph)
        for _ in range(max(1, a.warmup // K // per_graph)):
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
    loss = float(e.loss_rows().mean().item())
    print("%-8s %-5s B=%d K=%d  us/optimizer step over %d x %d steps: %s  median %.2f  (%.2f us per micro-batch; "
          "step %d, micro %d, loss %.4g)" % (a.config, a.dtype, a.batch_size, K, a.repeats, reps * per_graph,
                                             " ".join("%.2f" % u for u in us), statistics.median(us),
                                             statistics.median(us) / K, int(e.step_tensor().item()),
                                             int(e.micro_step_tensor().item()), loss), flush=True)
    return 0


def run_kernel(a):
    import torch

    from tensorflow_distributed_amd import _native
    from tensorflow_distributed_amd.models import mnist_cnn as M

    _native.require()
    ops = torch.ops.tfd
    dev = torch.device("cuda", 0)
    n = M.TOTAL
    gen = torch.Generator(device=dev).manual_seed(1)
    acc, g, out, p, m, v = (torch.randn(n, device=dev, generator=gen) * 0.01 for _ in range(6))
    v.abs_()
    obf = torch.empty(n, dtype=torch.bfloat16, device=dev)
    pbf = torch.empty(n, dtype=torch.bfloat16, device=dev)
    step = torch.ones(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream()
    iters = 200

    def timed(fn):
        with torch.cuda.stream(stream):
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(a.repeats):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                ev0.record(stream)
                for _ in range(iters):
                    fn()
                ev1.record(stream)
            torch.cuda.synchronize()
            best.append(1e3 * ev0.elapsed_time(ev1) / iters)
        return statistics.median(best)

    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.min_warmup_ms:
        with torch.cuda.stream(stream):
            ops.grad_accum_flat(acc, g)
        torch.cuda.synchronize()
    print("grad_accum kernel, n = %d fp32 elements; us per launch back to back in one stream (launch gaps included), "
          "median of %d x %d" % (n, a.repeats, iters))
    modes = (("store", 8, lambda b, l: ops.grad_accum_tuned(acc, g, None, True, b, l)),
             ("add", 12, lambda b, l: ops.grad_accum_tuned(acc, g, None, False, b, l)),
             ("emit fp32", 12, lambda b, l: ops.grad_accum_tuned(acc, g, out, False, b, l)),
             ("emit bf16", 10, lambda b, l: ops.grad_accum_tuned(acc, g, obf, False, b, l)))
    for name, bpe, fn in modes:
        us = timed(lambda: fn(0, 0))
        print("  %-9s default grid: %7.2f us  %6.2f TB/s (%d B/element)" % (name, us, n * bpe / us * 1e-6, bpe), flush=True)
    print("A/B of the add mode, blocks x loads in flight per lane (0 blocks = ceil(n4 / (256 * loads)), capped at 1024):")
    for loads in (1, 2, 4):
        for blocks in (0, 512, 1024, 2048, 4096):
            us = timed(lambda: ops.grad_accum_tuned(acc, g, None, False, blocks, loads))
            print("  loads %d blocks %4d: %7.2f us  %6.2f TB/s" % (loads, blocks, us, n * 12 / us * 1e-6), flush=True)
    us = timed(lambda: ops.adam_flat(p, m, v, g, pbf, 0.01, 0.9, 0.999, 1e-8, step, 1.0, 0))
    print("adam_flat on buffers of the same size (p, m, v read and written, g read, bf16 shadow written: 30 B/element): "
          "%7.2f us  %6.2f TB/s" % (us, n * 30 / us * 1e-6), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=CONFIGS + ("kernel",), default=None, help="run this one configuration in this process")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1000, help="micro-batches per timed repeat")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--min_warmup_ms", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="all configurations, interleaved, this many times")
    ap.add_argument("--timeout", type=float, default=120.0, help="per configuration, seconds")
    a = ap.parse_args()
    if a.config == "kernel":
        return run_kernel(a)
    if a.config:
        return run_step(a)
    med = {}
    jobs = [(cfg, dtype) for _ in range(a.rounds) for dtype in ("bf16", "fp32") for cfg in CONFIGS] + [("kernel", "bf16")]
    for cfg, dtype in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--dtype", dtype,
               "--batch_size", str(a.batch_size), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--min_warmup_ms", str(a.min_warmup_ms), "--repeats", str(a.repeats)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print("%s %s: timed out after %.0f s; stopping" % (cfg, dtype, a.timeout), flush=True)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:  # nothing more is started on the GPU after a failure
            print("%s %s: exit status %d; stopping" % (cfg, dtype, r.returncode), flush=True)
            return r.returncode
        mt = re.search(r"median ([0-9.]+)", r.stdout)
        if cfg != "kernel" and mt:
            med.setdefault((cfg, dtype), []).append(float(mt.group(1)))
    ok = True
    for dtype in ("bf16", "fp32"):
        k4 = statistics.median(med[("k4", dtype)])
        un = statistics.median(med[("unfused", dtype)])
        fu = statistics.median(med[("fused", dtype)])
        verdict = "PASS" if k4 < 4 * un else "FAIL"
        ok = ok and k4 < 4 * un
        print("%s %s: k4 step %.2f us < 4 unfused steps %.2f us (4 fused default steps: %.2f us, reported as it falls)"
              % (verdict, dtype, k4, 4 * un, 4 * fu), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
