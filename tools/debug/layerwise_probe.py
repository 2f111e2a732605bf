"""Cost of the layer-wise optimizers in the one-GPU MNIST step (MnistEngine.set_lamb / set_lars).

Times 1000 replayed steps at B=128 of four configurations, bf16 and fp32 dtype:

  adam      set_adam, set_fused_tail(0): the unfused Adam step (slab reduce + adam_kernel)
  momentum  set_momentum(0.9), the unfused momentum step
  lamb      set_lamb: the same serial schedule with the three layer-wise stages in place of adam_kernel
  lars      set_lars: likewise in place of sgd_kernel

All are captured the same way (100 steps per torch.cuda.graph, the engine launching into the capturing
stream) and timed after bench.py's warm-up protocol (--warmup steps, then untimed replays until
--min_warmup_ms have passed). Every configuration runs in a process of its own under its own timeout,
interleaved over --rounds; the first failure ends the run. With --baseline_lib the adam / momentum
processes load that native library (TFD_NATIVE_LIB: a build of the commit to compare against), so the
comparison is that commit's step, interleaved with this one's.

--wire bf16 (bf16 dtype only) times the data-parallel form of the same steps: the all-reduce schedule forced
over a world-1 IPC communicator with the bf16 wire, so the optimizer reads the gradient from the bf16 buffer
the all-reduce leaves (the default of every multi-GPU run); the step is captured by the engine itself
(capture_train_steps), as its DP schedule spans streams.

`--config X --dtype D` runs one configuration in this process: what `rocprofv3 --kernel-trace -- python
tools/debug/layerwise_probe.py --config lamb ...` wraps; tools/prof_summary.py then gives each stage's
time, and --stage_bytes prints the bytes each stage moves per parameter, from which the achieved
bytes per second follow:

  LAMB  stage 1 reads p, m, v, g (16 B; 14 B with a bf16 gradient) and writes m, v (8 B): 24 B
        stage 3 reads p, m', v' (12 B) and writes p (4 B) and the bf16 shadow (2 B):        18 B   total 42 B
  LARS  stage 1 reads p, g (8 B)
        stage 3 reads p, accum, g (12 B) and writes accum, p (8 B) and the shadow (2 B):    22 B   total 30 B
  Adam (adam_kernel) reads p, m, v, g (16 B), writes p, m, v (12 B) and the shadow (2 B):   30 B

    python tools/debug/layerwise_probe.py --baseline_lib <parent _C.so> > profiles/layerwise_step.log
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = ("adam", "lamb", "momentum", "lars")
NUM_PARAMS = 3274634
STAGE_BYTES = {"lamb": {"stage1": 24, "stage1 bf16 wire": 22, "stage3": 18},
               "lars": {"stage1": 8, "stage1 bf16 wire": 6, "stage3": 22, "stage3 bf16 wire": 20},
               "adam": {"adam_kernel": 30}, "momentum": {"sgd_kernel": 22}}


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
    if a.config == "adam":
        e.set_adam(0.01, 0.9, 0.999, 1e-8)
        e.set_fused_tail(0)
    elif a.config == "momentum":
        e.set_momentum(0.01, 0.9, False)
    elif a.config == "lamb":
        e.set_lamb(0.001, 0.9, 0.999, 1e-6, 0.01, True)
    else:
        e.set_lars(0.01, 0.9, 1e-4, 1e-3, 0.0, True)
    stream = torch.cuda.Stream()
    per_graph = 100
    reps = max(1, a.steps // per_graph)
    transport = None
    if a.wire == "bf16":
        from tensorflow_distributed_amd.parallel.transport import attach_engine

        transport = attach_engine(e, 0, 1, dev, mode="ipc", force_dp=True, bf16=True)
    with torch.cuda.stream(stream):
        e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev) * 0.05)
        e.sync_shadow()
        e.set_dataset(data, labels, perm)
        e.set_input_mode(1)
        e.train_step()
    torch.cuda.synchronize()
    if transport is not None:
        class _EngineGraph:  # the engine's own capture: the DP schedule spans streams
            def replay(self):
                e.replay("probe", 1)

        with torch.cuda.stream(stream):
            e.capture_train_steps("probe", per_graph)
        graph = _EngineGraph()
    else:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for _ in range(per_graph):
                e.train_step()
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
    loss = float(e.loss_rows().mean().item())
    extra = ""
    if a.config in ("lamb", "lars"):
        extra = ", trust ratios " + " ".join("%.4g" % r[2] for r in e.layer_norms().tolist())
    lib = os.environ.get("TFD_NATIVE_LIB", "")
    if transport is not None:
        transport.check()
    print("%-8s %-15s B=%d  us/step over %d x %d steps: %s  median %.2f  (step %d, loss %.4g%s)%s" % (
        a.config, a.dtype + ("/bf16-wire" if transport is not None else ""), a.batch_size, a.repeats, reps * per_graph, " ".join("%.2f" % u for u in us),
        statistics.median(us), int(e.step_tensor().item()), loss, extra, "  [baseline library]" if lib else ""), flush=True)
    if transport is not None:
        transport.close()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=CONFIGS, default=None, help="run this one configuration in this process")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--wire", choices=["none", "bf16"], default="none", help="bf16: forced DP at world 1 over IPC "
                    "with the bf16 gradient wire (bf16 dtype)")
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--min_warmup_ms", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="all configurations, interleaved, this many times")
    ap.add_argument("--timeout", type=float, default=120.0, help="per configuration, seconds")
    ap.add_argument("--baseline_lib", default="", help="native library the adam / momentum processes load")
    ap.add_argument("--stage_bytes", action="store_true", help="print the bytes per parameter of each stage and stop")
    a = ap.parse_args()
    if a.stage_bytes:
        for cfg, st in STAGE_BYTES.items():
            for k, b in st.items():
                print("%-8s %-17s %2d B/param  %.2f MB per launch over %d parameters" % (cfg, k, b, b * NUM_PARAMS / 1e6,
                                                                                     NUM_PARAMS))
        return 0
    if a.config:
        return run_one(a)
    for rnd in range(a.rounds):
        for dtype, wire in (("bf16", "none"), ("fp32", "none"), ("bf16", "bf16")):
            for cfg in CONFIGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--dtype", dtype, "--wire", wire,
                       "--batch_size", str(a.batch_size), "--steps", str(a.steps), "--warmup", str(a.warmup),
                       "--min_warmup_ms", str(a.min_warmup_ms), "--repeats", str(a.repeats)]
                env = dict(os.environ)
                if a.baseline_lib and cfg in ("adam", "momentum"):
                    env["TFD_NATIVE_LIB"] = os.path.abspath(a.baseline_lib)
                try:
                    rc = subprocess.run(cmd, timeout=a.timeout, env=env).returncode
                except subprocess.TimeoutExpired:
                    print("%s %s: timed out after %.0f s; stopping" % (cfg, dtype, a.timeout), flush=True)
                    return 124
                if rc != 0:  # nothing more is started on the GPU after a failure
                    print("%s %s: exit status %d; stopping" % (cfg, dtype, rc), flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
