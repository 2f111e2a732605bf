"""Cost of RMSProp and Adagrad in the one-GPU MNIST step (MnistEngine.set_rmsprop / set_adagrad), and of
their flat kernels alone.

Part 1 times 1000 replayed steps at B=128 of six configurations, bf16 and fp32 dtype, all on the unfused step
(slab reduce + ONE optimizer launch):

  rmsprop        set_rmsprop(momentum 0):            rmsprop_kernel<false, false>
  rmsprop_mom    set_rmsprop(momentum 0.9):          rmsprop_kernel<false, true>
  rmsprop_cen    set_rmsprop(momentum 0.9, centered) rmsprop_kernel<true, true>
  adagrad        set_adagrad:                        adagrad_kernel
  momentum       set_momentum(0.9):                  sgd_kernel
  adam           set_adam, set_fused_tail(0):        adam_kernel

Every configuration is captured the same way (100 steps per torch.cuda.graph, the engine launching into the
capturing stream); the engines live in ONE process and their timed replays are interleaved over --rounds, after
bench.py's warm-up protocol (--warmup steps each, then untimed replays until --min_warmup_ms have passed).

Part 2 times each flat op alone over M.TOTAL elements (fp32 gradient, bf16 shadow written), 100 launches per
graph, interleaved over the same rounds, with the bytes each moves per parameter and the achieved TB/s:

  adagrad_flat                reads p, accum, g (12 B), writes p, accum (8 B) and the shadow (2 B):   22 B
  rmsprop_flat  momentum 0    reads p, ms, g (12 B), writes p, ms, mom (12 B) and the shadow:         26 B
  rmsprop_flat  momentum      also reads mom:                                                         30 B
  rmsprop_flat  centered      momentum 0: reads / writes mg too (34 B); with momentum:                38 B
  adam_flat                   reads p, m, v, g (16 B), writes p, m, v (12 B) and the shadow:          30 B
  momentum_flat               reads p, mom, g (12 B), writes p, mom (8 B) and the shadow:             22 B

The expectation it checks: Adagrad and RMSProp without momentum move 22/30 and 26/30 of Adam's bytes, so neither
may be slower than adam_flat by more than adam_flat's own round-to-round spread here; the last lines say so.

    python tools/debug/rules_probe.py > profiles/rules_step.log
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = ("rmsprop", "rmsprop_mom", "rmsprop_cen", "adagrad", "momentum", "adam")
FLAT_BYTES = {"adagrad_flat": 22, "rmsprop_flat": 26, "rmsprop_flat mom": 30, "rmsprop_flat centered": 34,
              "rmsprop_flat centered mom": 38, "adam_flat": 30, "momentum_flat": 22}
PER_GRAPH = 100


def make_engine(torch, M, cfg, dtype, batch, dev, ds):
    e = torch.classes.tfd.MnistEngine(batch, 0, 0.75, 1234, 0)
    e.set_dtype(dtype)
    if cfg == "adam":
        e.set_adam(0.01, 0.9, 0.999, 1e-8)
        e.set_fused_tail(0)
    elif cfg == "momentum":
        e.set_momentum(0.01, 0.9, False)
    elif cfg == "adagrad":
        e.set_adagrad(0.01, 0.1)
    else:
        e.set_rmsprop(0.001, 0.9, 0.0 if cfg == "rmsprop" else 0.9, 1e-10, cfg == "rmsprop_cen")
    e.params().copy_(M.flat_from_dict(M.init_params(0)).to(dev) * 0.05)
    e.sync_shadow()
    e.set_dataset(*ds)
    e.set_input_mode(1)
    e.train_step()
    return e


def capture(torch, stream, fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for _ in range(PER_GRAPH):
            fn()
    return graph


def timed(torch, stream, graph, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        ev0.record(stream)
        for _ in range(reps):
            graph.replay()
        ev1.record(stream)
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / (reps * PER_GRAPH)


def warm(torch, stream, graphs, a):
    for g in graphs:
        with torch.cuda.stream(stream):
            for _ in range(max(1, a.warmup // PER_GRAPH)):
                g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < a.min_warmup_ms:  # the clock ramp
        with torch.cuda.stream(stream):
            for g in graphs:
                g.replay()
        torch.cuda.synchronize()


def flat_ops(torch, M, dev):
    """name -> a closure launching the op once over M.TOTAL elements."""
    ops, n = torch.ops.tfd, M.TOTAL
    gen = torch.Generator(device=dev).manual_seed(5)
    buf = lambda v=None: torch.full((n,), v, device=dev) if v is not None else torch.randn(n, device=dev, generator=gen) * 0.01  # noqa: E731
    g, pbf = buf(), torch.zeros(n, device=dev, dtype=torch.bfloat16)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    out = {}

    def rms(momentum, centered):
        p, ms, mom, mg = buf(), buf(1.0), buf(0.0), (buf(0.0) if centered else None)
        return lambda: ops.rmsprop_flat(p, ms, mom, g, pbf, 0.001, 0.9, momentum, 1e-10, mg)

    out["rmsprop_flat"] = rms(0.0, False)
    out["rmsprop_flat mom"] = rms(0.9, False)
    out["rmsprop_flat centered"] = rms(0.0, True)
    out["rmsprop_flat centered mom"] = rms(0.9, True)
    p1, acc = buf(), buf(0.1)
    out["adagrad_flat"] = lambda: ops.adagrad_flat(p1, acc, g, pbf, 0.01)
    p2, m, v = buf(), buf(0.0), buf(0.0)
    out["adam_flat"] = lambda: ops.adam_flat(p2, m, v, g, pbf, 0.001, 0.9, 0.999, 1e-8, step)
    p3, mo = buf(), buf(0.0)
    out["momentum_flat"] = lambda: ops.momentum_flat(p3, mo, g, pbf, 0.01, 0.9, 0.0, False)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch_size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--min_warmup_ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5, help="every configuration, interleaved, this many times")
    ap.add_argument("--flat_launches", type=int, default=1000, help="launches per timed sample of a flat op")
    a = ap.parse_args()

    import torch

    from tensorflow_distributed_amd import _native
    from tensorflow_distributed_amd.models import mnist_cnn as M

    _native.require()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(3)
    rows = 8192
    ds = (torch.rand(rows, 784, device=dev, generator=gen),
          torch.randint(0, 10, (rows,), dtype=torch.int32, device=dev, generator=gen),
          torch.randperm(rows, device=dev, generator=gen).to(torch.int32))
    stream = torch.cuda.Stream()
    reps = max(1, a.steps // PER_GRAPH)
    print("rules_probe: B=%d, %d steps per sample (%d per graph), %d rounds, one process" % (
        a.batch_size, reps * PER_GRAPH, PER_GRAPH, a.rounds), flush=True)
    for dtype in ("bf16", "fp32"):
        with torch.cuda.stream(stream):
            engines = {c: make_engine(torch, M, c, dtype, a.batch_size, dev, ds) for c in CONFIGS}
        torch.cuda.synchronize()
        graphs = {c: capture(torch, stream, e.train_step) for c, e in engines.items()}
        warm(torch, stream, list(graphs.values()), a)
        us = {c: [] for c in CONFIGS}
        for _ in range(a.rounds):
            for c in CONFIGS:
                us[c].append(timed(torch, stream, graphs[c], reps))
        for c in CONFIGS:
            e = engines[c]
            print("step  %-12s %-5s us/step by round: %s  median %.2f  (step %d, loss %.4g)" % (
                c, dtype, " ".join("%.2f" % u for u in us[c]), statistics.median(us[c]), int(e.step_tensor().item()),
                float(e.loss_rows().mean().item())), flush=True)
        del graphs, engines
    # ---- the flat ops alone
    with torch.cuda.stream(stream):
        fns = flat_ops(torch, M, dev)
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    graphs = {k: capture(torch, stream, fn) for k, fn in fns.items()}
    warm(torch, stream, list(graphs.values()), a)
    freps = max(1, a.flat_launches // PER_GRAPH)
    us = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k in graphs:
            us[k].append(timed(torch, stream, graphs[k], freps))
    med = {k: statistics.median(v) for k, v in us.items()}
    for k in graphs:
        mb = FLAT_BYTES[k] * M.TOTAL / 1e6
        print("flat  %-26s %2d B/param %6.2f MB  us/launch by round: %s  median %.2f  %.2f TB/s" % (
            k, FLAT_BYTES[k], mb, " ".join("%.2f" % u for u in us[k]), med[k], mb / med[k]), flush=True)
    spread = max(us["adam_flat"]) - min(us["adam_flat"])
    print("adam_flat: median %.2f us, round-to-round spread (max - min) %.2f us" % (med["adam_flat"], spread))
    rc = 0
    for k in ("adagrad_flat", "rmsprop_flat"):
        slower = med[k] - med["adam_flat"]
        verdict = "not slower than adam_flat" if slower <= 0 else (
            "slower than adam_flat by %.2f us, within its spread" % slower if slower <= spread else
            "SLOWER than adam_flat by %.2f us, beyond its spread of %.2f us" % (slower, spread))
        print("%-13s %2d/30 of adam_flat's bytes, %.2f us against %.2f us: %s" % (
            k, FLAT_BYTES[k], med[k], med["adam_flat"], verdict))
        rc = rc or (1 if slower > spread else 0)
    return rc


if __name__ == "__main__":
    sys.exit(main())
