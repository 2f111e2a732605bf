"""What does a kernel's first kernel-argument fetch cost on this box? (docs/DESIGN.md section 8c)

Every kernel of the MNIST step took its pointers from a 320-byte by-value struct: each wave starts
with scalar loads of the argument segment and waits for them before its first vector address exists.
This probe measures that wait in isolation. It captures a chain of LINKS dependent kernels, one
64-lane block per CU, each issuing ONE vector load whose address comes from an argument
(csrc/kernels/kernarg_probe.hip), in two forms:

  struct   the pointers inside a 320-byte by-value struct (scalar load + wait, then the vector load);
  preload  the pointers as leading kernel parameters, preloaded into SGPRs at wave launch.

Both run twice: back to back (the argument segment's lines may still sit in a cache), and with a
90 MB streaming kernel (tfd::roofline_stream: the optimizer tail's traffic) between the links, which
is what the step's kernels see in front of them. The per-link difference struct - preload is the
cost of the fetch; with the stream between the links it is the difference of two long chains, so the
stream-only chain is printed too. Medians over TRIALS replays; one JSON line per configuration.

    python tools/debug/kernarg_probe.py [--links 300] [--trials 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tensorflow_distributed_amd import _native  # noqa: E402
from tensorflow_distributed_amd.models import mnist_cnn as M  # noqa: E402


def chain_us(link, links, trials):
    """median and min microseconds per link of a captured graph of `links` calls of link()"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            link()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(links):
            link()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(trials):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / links)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=300)
    ap.add_argument("--trials", type=int, default=9)
    a = ap.parse_args(argv)
    _native.require()
    dev = torch.device("cuda", 0)
    blocks = torch.cuda.get_device_properties(0).multi_processor_count  # one block per CU
    x = torch.zeros(blocks * 64, device=dev)
    y = torch.zeros(blocks * 64, device=dev)
    n = M.TOTAL // 4 * 4  # the optimizer tail's buffers: 28 B per parameter, ~90 MB
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.ones(n, device=dev)
    g = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    pbf = torch.empty(n, dtype=torch.bfloat16, device=dev)

    def stream():
        torch.ops.tfd.roofline_stream(p, m, v, g, pbf, None, 1024, 1)

    def probe(preload):
        torch.ops.tfd.kernarg_probe(x, y, blocks, preload)

    res = {}
    for streamed in (False, True):
        arms = [("struct", lambda: probe(False)), ("preload", lambda: probe(True))]
        if streamed:
            arms = [("stream only", stream)] + [(k, (lambda f=f: (stream(), f()))) for k, f in arms]
        for rnd in range(2):  # the arms interleaved twice: a drift of the box shows as a disagreement
            for name, fn in arms:
                med, lo, hi = chain_us(fn, a.links, a.trials)
                res[(streamed, name, rnd)] = med
                print(json.dumps({"probe": name, "stream_between_links": streamed, "round": rnd, "links": a.links,
                                  "blocks": blocks, "us_per_link_median": round(med, 3), "us_per_link_min": round(lo, 3),
                                  "us_per_link_max": round(hi, 3)}), flush=True)
    for streamed in (False, True):
        d = [res[(streamed, "struct", r)] - res[(streamed, "preload", r)] for r in range(2)]
        print(json.dumps({"result": "struct - preload, us per link", "stream_between_links": streamed,
                          "rounds": [round(v_, 3) for v_ in d]}), flush=True)


if __name__ == "__main__":
    main()
