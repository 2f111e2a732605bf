"""Cost of the device step log (MnistEngine.set_step_log) and what --steps_per_call buys.

1. Step time at B=128 with the log on against off, bf16 and fp32, replayed as one-step graphs and as
   20-step graphs: two engines per case, interleaved round by round in ONE process so that clock and
   neighbour drift hits them alike (the protocol of tools/debug/guard_probe.py). Every round times
   `--steps` replayed steps of each engine in turn with device events; the table gives every round, the
   median and the spread (max - min over the rounds).
2. The loss-mode kernel alone (MnistEngine.step_log_probe): back-to-back launches on one stream, ms per
   launch from device events, at B=128 and at the largest batch.
3. mnist_single.py --training_iters 256000 (1999 steps of 128 images), wall-clock images/sec from the
   script's own "Time for Training" line, --steps_per_call 1 against 20, and -- with --baseline_tree DIR,
   a checkout of the parent commit with its extension built -- the parent's mnist_single.py. One process
   per run, the arms alternating, at the default --display_step 10 (a call ends at every display, so 20
   steps per call become 10) and at --display_step 100. The 1999 steps train for 0.2 s, of which the one-off
   captures are a visible part, so the same three arms also run `--long_iters` images (ten times as many).
4. dist_main, 1 ps + 1 worker on the GPU, --train_steps 4000 --quiet, --steps_per_call 1 against 20: steps/sec
   from the worker's "Training elapsed time". This loop returns to the host after every step (it reads
   global_step), which is what a call of 20 steps removes.

    python tools/debug/step_log_probe.py [--baseline_tree DIR --baseline_commit SHA] > profiles/step_log_step.log

None of the numbers is a pass/fail bound.
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


def make_engine(log, dtype, per_graph, a, ds, dev):
    import torch

    from tensorflow_distributed_amd.models import mnist_cnn as M

    e = torch.classes.tfd.MnistEngine(a.batch_size, 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    e.set_adam(0.01, 0.9, 0.999, 1e-8)
    if log:
        e.set_step_log(1024)
    e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev))  # the reference's N(0,1) init
    e.sync_shadow()
    e.set_dataset(*ds)
    e.set_input_mode(1)
    e.train_step()
    e.capture_train_steps("g", per_graph)
    for _ in range(max(1, a.warmup // per_graph)):
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


def steps_table(dtype, per_graph, a, ds, dev, stream):
    import torch

    with torch.cuda.stream(stream):
        engines = {name: make_engine(name == "log on", dtype, per_graph, a, ds, dev) for name in ("log off", "log on")}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.min_warmup_ms:  # the clock ramp (profiles/warmup_ramp.log)
        for e in engines.values():
            with torch.cuda.stream(stream):
                e.replay("g", max(1, 100 // per_graph))
        torch.cuda.synchronize()
    reps = a.steps // per_graph
    us = {name: [] for name in engines}
    for _ in range(a.rounds):
        for name, e in engines.items():
            us[name].append(timed(stream, lambda: e.replay("g", reps)) / (reps * per_graph))
    for name, e in engines.items():
        print("%-7s %-5s B=%d %2d-step graph  us/step, %d rounds of %d steps: %s  median %.2f  spread %.2f  (step %d, loss "
              "%.4g)" % (name, dtype, a.batch_size, per_graph, a.rounds, reps * per_graph,
                         " ".join("%.2f" % u for u in us[name]), statistics.median(us[name]),
                         max(us[name]) - min(us[name]), int(e.step_tensor().item()), float(e.loss_rows().mean().item())),
              flush=True)
    on, off = us["log on"], us["log off"]
    print("%s %d-step graph: log on - log off, medians %+.2f us/step; per round: %s" % (
        dtype, per_graph, statistics.median(on) - statistics.median(off), " ".join("%+.2f" % (x - y) for x, y in zip(on, off))),
        flush=True)
    t, rec = engines["log on"].step_log()
    last = int(engines["log on"].step_tensor().item())
    slot = (last - 1) % t.numel()
    assert int(t[slot].item()) == last, "the log on engine did not log its last step"
    return engines["log on"]


def kernel_alone(a, ds, dev, stream):
    import torch

    for batch in (a.batch_size, int(torch.ops.tfd.mnist_max_batch())):
        with torch.cuda.stream(stream):
            e = torch.classes.tfd.MnistEngine(batch, 0, 0.75, 1234, 0)
            e.set_step_log(1024)
            e.step_log_probe(200)  # warm
            ms = [e.step_log_probe(a.kernel_iters) for _ in range(a.rounds)]
        torch.cuda.synchronize()
        us = [1e3 * m for m in ms]
        print("loss-mode kernel alone B=%-5d us/launch (back-to-back launches on one stream), %d rounds of %d: %s  median "
              "%.2f  spread %.2f" % (batch, a.rounds, a.kernel_iters, " ".join("%.2f" % u for u in us),
                                     statistics.median(us), max(us) - min(us)), flush=True)


def run_single(tree, extra, a, iters):
    """One mnist_single.py process from `tree` -> (images/sec, steps, seconds) from its own training clock."""
    cmd = [sys.executable, os.path.join(tree, "mnist_single.py"), "--training_iters", str(iters),
           "--data_dir", os.path.join(a.tmp, "none"), "--eval_batches", "1"] + extra
    env = dict(os.environ, PYTHONPATH=tree)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=tree)
    if p.returncode != 0:
        raise RuntimeError("mnist_single failed: %s\n%s" % (" ".join(cmd), p.stderr[-2000:]))
    secs = float(re.search(r"--- ([0-9.eE+-]+) seconds Time for Training ---", p.stdout).group(1))
    steps = -(-iters // 128) - 1
    return steps * 128 / secs, steps, secs


def drivers_table(a):
    arms = []
    if a.baseline_tree:
        arms.append(("parent commit %s" % (a.baseline_commit or "?"), a.baseline_tree, []))
    arms += [("--steps_per_call 1", ROOT, ["--steps_per_call", "1"]), ("--steps_per_call 20", ROOT, ["--steps_per_call", "20"])]
    for display, iters in ((10, a.training_iters), (100, a.training_iters), (100, a.long_iters)):
        res = {name: [] for name, _, _ in arms}
        for _ in range(a.driver_rounds):
            for name, tree, extra in arms:
                res[name].append(run_single(tree, extra + ["--display_step", str(display)], a, iters))
        for name, _, _ in arms:
            ips = [r[0] for r in res[name]]
            print("mnist_single --training_iters %d --display_step %-3d %-28s images/sec over %d steps (training wall "
                  "clock, one process per run): %s  median %.0f  (%.3f s)" % (
                      iters, display, name, res[name][0][1], " ".join("%.0f" % v for v in ips),
                      statistics.median(ips), statistics.median(r[2] for r in res[name])), flush=True)


def dist_main_table(a):
    from tensorflow_distributed_amd import launch

    res = {1: [], 20: []}
    for _ in range(a.driver_rounds):
        for n in res:
            logdir = os.path.join(a.tmp, "step_log_probe_%d_%d" % (os.getpid(), len(res[1]) + len(res[20])))
            args = ["--num_gpus=1", "--train_steps=%d" % a.dist_steps, "--logdir=" + logdir, "--synthetic_data",
                    "--eval_batches=1", "--data_dir=/nonexistent", "--quiet", "--steps_per_call=%d" % n]
            r = launch.launch(1, 1, args, echo=False, timeout_s=300)
            out = "".join(v for k, v in r["outputs"].items() if k.startswith("worker:0#"))
            if not r["ok"]:
                raise RuntimeError("dist_main failed:\n" + out[-2000:])
            res[n].append(a.dist_steps / float(re.search(r"Training elapsed time: ([0-9.eE+-]+) s", out).group(1)))
    for n, v in res.items():
        print("dist_main 1 worker --train_steps %d --steps_per_call %-2d steps/sec (training wall clock, one cluster per "
              "run): %s  median %.0f  (%.1f us/step)" % (a.dist_steps, n, " ".join("%.0f" % x for x in v),
                                                         statistics.median(v), 1e6 / statistics.median(v)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=2000, help="timed steps per engine and round")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--min_warmup_ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel_iters", type=int, default=2000)
    ap.add_argument("--training_iters", type=int, default=256000)
    ap.add_argument("--long_iters", type=int, default=2560000)
    ap.add_argument("--driver_rounds", type=int, default=3)
    ap.add_argument("--baseline_tree", default="", help="a checkout of the parent commit, its extension built")
    ap.add_argument("--baseline_commit", default="", help="its commit id, for the log")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--dist_steps", type=int, default=4000)
    ap.add_argument("--skip_drivers", action="store_true")
    ap.add_argument("--only_dist_main", action="store_true")
    a = ap.parse_args()

    if a.only_dist_main:
        print("== dist_main, steps per host round trip", flush=True)
        dist_main_table(a)
        return 0

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
    print("== step time, log on against log off: B=%d, two engines interleaved in one process" % a.batch_size, flush=True)
    for dtype in ("bf16", "fp32"):
        for per_graph in (1, 20):
            steps_table(dtype, per_graph, a, ds, dev, stream)
    print("== the loss-mode kernel alone", flush=True)
    kernel_alone(a, ds, dev, stream)
    del ds
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if not a.skip_drivers:
        print("== mnist_single.py, steps per host round trip%s" % (
            "; baseline: the parent commit %s" % a.baseline_commit if a.baseline_tree else " (no baseline tree given)"),
            flush=True)
        drivers_table(a)
        print("== dist_main, steps per host round trip", flush=True)
        dist_main_table(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
