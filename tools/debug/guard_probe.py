"""Cost of the non-finite guard in the one-GPU MNIST step (MnistEngine.set_skip_nonfinite).

Times replayed steps at B=128 of four configurations, bf16 and fp32 dtype, interleaved in ONE process so
that clock and neighbour drift hits them alike:

  clip        set_clip_norm(c): the whole-gradient path, two norm launches + Adam's clip instantiation
              (code unchanged by the guard: the baseline)
  guard       set_skip_nonfinite: the same launches, the finish kernel also writes ok and the counter,
              Adam's guarded instantiation (one more uniform load and branch)
  guard+clip  both
  fused       the default step (one optimizer kernel that also reduces the conv slabs)

Every engine captures one 100-step graph; a round times `--steps` replayed steps of each configuration in
turn with device events, after bench.py's warm-up protocol. The table gives every round, the median and
the spread (max - min over the rounds) per configuration. Then the norm / guard stages alone, as ops:
tfd::grad_global_norm (stage 1 + norm finish) against tfd::grad_guard (stage 1 + guard finish), 100 calls
per captured graph, at the engine's length and at n = 4, where stage 1 is one nearly empty block and the
time is the finish kernel's and the launch boundaries'.

    python tools/debug/guard_probe.py > profiles/nonfinite_guard_step.log
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = ("clip", "guard", "guard+clip", "fused")
PER_GRAPH = 100


def make_engine(cfg, dtype, a, ds, dev):
    import torch

    from tensorflow_distributed_amd.models import mnist_cnn as M

    e = torch.classes.tfd.MnistEngine(a.batch_size, 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    if "clip" in cfg:
        e.set_clip_norm(a.clip_norm)
    if "guard" in cfg:
        e.set_skip_nonfinite(True)
    e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev))  # the reference's N(0,1) init
    e.sync_shadow()
    e.set_dataset(*ds)
    e.set_input_mode(1)
    e.train_step()
    e.capture_train_steps("g", PER_GRAPH)
    for _ in range(max(1, a.warmup // PER_GRAPH)):
        e.replay("g", 1)
    return e


def timed(stream, fn):
    import torch

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        ev0.record(stream)
        fn()
        ev1.record(stream)
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1)  # us


def steps_table(dtype, a, ds, dev, stream):
    import torch

    with torch.cuda.stream(stream):
        engines = {cfg: make_engine(cfg, dtype, a, ds, dev) for cfg in CONFIGS}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.min_warmup_ms:  # the clock ramp (profiles/warmup_ramp.log)
        for e in engines.values():
            with torch.cuda.stream(stream):
                e.replay("g", 1)
        torch.cuda.synchronize()
    reps = a.steps // PER_GRAPH
    us = {cfg: [] for cfg in CONFIGS}
    for _ in range(a.rounds):
        for cfg, e in engines.items():
            us[cfg].append(timed(stream, lambda: e.replay("g", reps)) / (reps * PER_GRAPH))
    for cfg, e in engines.items():
        norm, scale = e.grad_norm().tolist()
        print("%-10s %-5s B=%d  us/step, %d rounds of %d steps: %s  median %.2f  spread %.2f  (step %d, loss %.4g, "
              "grad_norm %.6g, clip_scale %.6g, skipped_steps %d)"
              % (cfg, dtype, a.batch_size, a.rounds, reps * PER_GRAPH, " ".join("%.2f" % u for u in us[cfg]),
                 statistics.median(us[cfg]), max(us[cfg]) - min(us[cfg]), int(e.step_tensor().item()),
                 float(e.loss_rows().mean().item()), norm, scale, e.skipped_steps()), flush=True)
    med = {cfg: statistics.median(v) for cfg, v in us.items()}
    print("%s medians: guard+clip - clip %+.2f us, guard - clip %+.2f us, guard - fused %+.2f us; per-round guard+clip - "
          "clip: %s" % (dtype, med["guard+clip"] - med["clip"], med["guard"] - med["clip"], med["guard"] - med["fused"],
                        " ".join("%+.2f" % (x - y) for x, y in zip(us["guard+clip"], us["clip"]))), flush=True)


def stages_table(a, dev, stream):
    import torch

    from tensorflow_distributed_amd.models import mnist_cnn as M

    ops = torch.ops.tfd
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    for n in (M.TOTAL, 4):
        g = torch.randn(n, device=dev) * 1e-2
        calls = {"grad_global_norm": lambda: ops.grad_global_norm(g, 5.0, 1.0),
                 "grad_guard": lambda: ops.grad_guard(g, 1.0, 5.0, skipped)}
        graphs = {}
        for name, call in calls.items():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                call()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(PER_GRAPH):
                    call()
        us = {name: [] for name in calls}
        for _ in range(a.rounds + 1):  # the first round warms up
            for name, gr in graphs.items():
                us[name].append(timed(stream, lambda: [gr.replay() for _ in range(10)]) / (10 * PER_GRAPH))
        for name in calls:
            v = us[name][1:]
            print("%-17s n=%-8d us/call (two launches), %d rounds of %d calls: %s  median %.2f  spread %.2f"
                  % (name, n, a.rounds, 10 * PER_GRAPH, " ".join("%.2f" % u for u in v), statistics.median(v),
                     max(v) - min(v)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1000, help="timed steps per configuration and round")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--min_warmup_ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--clip_norm", type=float, default=5.0)
    a = ap.parse_args()

    import torch

    from tensorflow_distributed_amd import _native

    _native.require()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(3)
    rows = 8192
    ds = (torch.rand(rows, 784, device=dev, generator=gen),
          torch.randint(0, 10, (rows,), dtype=torch.int32, device=dev, generator=gen),
          torch.randperm(rows, device=dev, generator=gen).to(torch.int32))
    stream = torch.cuda.Stream()
    print("== steps: B=%d, %d-step graphs, configurations interleaved in one process" % (a.batch_size, PER_GRAPH), flush=True)
    for dtype in ("bf16", "fp32"):
        steps_table(dtype, a, ds, dev, stream)
    print("== stages alone, as ops (%d calls per captured graph)" % PER_GRAPH, flush=True)
    stages_table(a, dev, stream)
    return 0


if __name__ == "__main__":
    sys.exit(main())
