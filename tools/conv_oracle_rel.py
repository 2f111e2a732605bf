#!/usr/bin/env python
"""Run every case of tests/test_conv_oracle_gpu.py's tables on the GPU and print, per op and shape,
the exact family's mismatch count and the random family's worst |got - ref| / bound against the fp64
oracle (tests/conv_oracle.py), in each GEMM core mode (128-row core / 256-row core / halo tiles) and
both statistics-partials modes (row mode / 4 slots) where partials are involved.

The bounds are derived (conv_oracle's docstrings), so a ratio <= 1 is a pass and the ratio shows how
much of the bound a kernel uses; a count > 0 or a ratio > 1 is what the tests would fail on.

    python tools/conv_oracle_rel.py > profiles/conv_oracle_r8.txt
"""
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

CORES = [("core128", 0, 0), ("core256", 2, 0), ("halo", 1, 2)]
SLOTS = [("row", 0), ("slots4", 4)]


def measure(check):
    what, got, ref, bound, _ = check
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    if not torch.is_tensor(bound) and float(bound) == 0.0:
        return what, "exact", int((err > 0).sum()), err.numel()
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                      torch.zeros_like(err)))
    return what, "bound", float(ratio.max()) if ratio.numel() else 0.0, err.numel()


def main():
    from tensorflow_distributed_amd import _native
    _native.require()
    import conv_oracle as O
    ops = torch.ops.tfd
    dev = torch.device("cuda", 0)
    DG = [(s, a) for s in O.DGRAD_SHAPES for a in O.dgrad_adds(s)]
    DGBN = [(s, m, a) for s in O.DGRAD_BN_SHAPES for m in (0, 2, 3) for a in O.dgrad_adds(s)
            if a in (None, "plain") or s[0] * s[1] * s[2] < 4096]
    plain = [lambda s=s: O.run_fwd_exact(ops, dev, s) for s in O.FWD_SHAPES]
    plain += [lambda s=s, a=a: O.run_dgrad_exact(ops, dev, s, a) for s, a in DG]
    plain += [lambda s=s, z=z: O.run_wgrad_exact(ops, dev, s, z) for s in O.WGRAD for z in (False, True)]
    plain += [lambda s=s: O.run_linear_exact(ops, dev, s) for s in O.LINEAR]
    plain += [lambda s=s: O.run_gemm_nt_exact(ops, dev, s) for s in O.GEMM_NT]
    plain += [lambda s=s: O.run_maxpool_exact(ops, dev, s) for s in O.POOLS]
    plain += [lambda s=s, op=op: O.run_conv_random(ops, dev, s, op) for s, op in O.RANDOM_CASES]
    stats = [lambda s=s: O.run_fwd_stats_exact(ops, dev, s) for s in O.FWD_SHAPES]
    stats += [lambda s=s, m=m, a=a: O.run_dgrad_bn_exact(ops, dev, s, m, a) for s, m, a in DGBN]
    stats += [lambda s=s: O.run_fold_exact(ops, dev, s) for s in O.FOLD]
    stats += [lambda s=s: O.run_stem_exact(ops, dev, s) for s in O.STEM]
    once = [lambda M=M, C=C, c=c: O.run_bn_random(ops, dev, M, C, *c) for M, C in O.BN_SHAPES for c in O.bn_combos()]
    once += [lambda M=M, C=C, r=r: O.run_bn_infer_random(ops, dev, M, C, r) for M, C in O.BN_SHAPES for r in (False, True)]
    once += [lambda n=n: O.run_xent(ops, dev, n) for n in O.xent_cases()]

    rows = OrderedDict()  # what -> (kind, {mode: value}, elements)

    def record(mode, checks):
        for c in checks:
            what, kind, v, n = measure(c)
            rows.setdefault(what, (kind, OrderedDict(), n))[1][mode] = v

    old = ops.conv_gemm_core(-1), ops.conv_halo_mode(-1), ops.bn_part_slots()
    try:
        for cname, core, halo in CORES:
            ops.conv_gemm_core(core)
            ops.conv_halo_mode(halo)
            for run in plain:
                record(cname, run())
            for sname, slots in SLOTS:
                ops.set_bn_part_slots(slots)
                for run in stats:
                    record(f"{cname}/{sname}", run())
            ops.set_bn_part_slots(old[2])
        ops.conv_gemm_core(old[0])
        ops.conv_halo_mode(old[1])
        for run in once:  # no GEMM and no producer partials: the modes do not reach these kernels
            record("-", run())
    finally:
        ops.conv_gemm_core(old[0])
        ops.conv_halo_mode(old[1])
        ops.set_bn_part_slots(old[2])
    torch.cuda.synchronize()

    print(f"# conv / BN oracle run: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    print("# exact family: mismatching elements (of n) per mode; random family: worst |got - ref| / derived bound per mode")
    print("# every bound is derived (tests/conv_oracle.py); the one assumption that is not a derivation: __expf's exp2 and")
    print("# __logf are taken as accurate to 2 ulp (the toolchain ships no figure) -- the softmax_xent ratios below are against that")
    print("# modes: " + ", ".join(n for n, _, _ in CORES) + " x " + ", ".join(n for n, _ in SLOTS) + " where partials are involved")
    bad = 0
    worst = {}
    for what, (kind, vals, n) in rows.items():
        if kind == "exact":
            bad += sum(1 for v in vals.values() if v)
            body = " ".join(f"{m}={v}" for m, v in vals.items()) if any(vals.values()) else f"0 in all {len(vals)} modes"
            print(f"exact  n={n:<9d} {what}: {body}")
        else:
            mx = max(vals.values())
            bad += mx > 1.0
            op = " ".join(what.split()[:2]) if what.startswith("softmax") else what.split(" (")[0].split(" M=")[0]
            worst[op] = max(worst.get(op, 0.0), mx)
            print(f"bound  n={n:<9d} {what}: worst ratio {mx:.3f}" + ("" if len(vals) == 1 else
                                                                      " (" + " ".join(f"{m}={v:.3f}" for m, v in vals.items()) + ")"))
    print("# worst ratio per op (random family):")
    for op, v in worst.items():
        print(f"#   {op}: {v:.3f}")
    print(f"# {len(rows)} checks, {bad} beyond their bound")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
