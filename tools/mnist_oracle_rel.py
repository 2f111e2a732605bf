"""Errors of the native MNIST step against its oracles: the calibration behind the test bounds.

Default: per-tensor relative L2 error of the fused bf16 step against the fp32 oracle that rounds to
bf16 where the kernels do (models.mnist_cnn.conv_net(emulate_bf16=True)): the bounds of
tests/test_mnist_engine_gpu.py::test_step_grads_match_oracle (about 3x the measured errors, like
profiles/resnet_oracle_rel_r5.txt for ResNet).

--slices: per-slice errors (tests/mnist_oracle.py: per tap, channel, tile, image, element ...) of both
precisions against the fp64 oracle, over the three standard configurations, the edge batches and the
B = 37 dropout case at three seeds each, then the special-input cases of
tests/test_mnist_kernel_edges_gpu.py (reported, not part of the bounds). The last section is the
BOUNDS table of tests/mnist_oracle.py: 3x the worst of each class.

--fused: the fused one-GPU Adam step (train_step() with set_fused_tail(1)) over the cases of
tests/test_mnist_fused_step_gpu.py: the gradient the tail consumed, read back out of Adam's m, per
slice against the fp64 oracle -- per dtype, setting and class the measured error and the bound used
(BOUNDS plus the derived allowances of tests/mnist_oracle.py::fused_allowance) -- and the worst ratios
error / tolerance of v and p' against fp64 ApplyAdam from that gradient. Its output is
profiles/mnist_fused_step_slices.txt.

    python tools/mnist_oracle_rel.py [--seeds 0,1,2] [--slices | --fused]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensorflow_distributed_amd import _native  # noqa: E402
from tensorflow_distributed_amd.models import mnist_cnn as M  # noqa: E402

CONFIGS = [(0.05, 128), (1.0, 128), (0.05, 40)]


def rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def measure(scale, B, seed, dev):
    torch.manual_seed(seed)
    params = {k: v * scale for k, v in M.init_params(7 + seed).items()}
    x = torch.rand(B, 784)
    y = torch.randint(0, 10, (B,), dtype=torch.int32)
    eng = torch.classes.tfd.MnistEngine(B, dev.index or 0, 1.0, 1234, 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.params().copy_(M.flat_from_dict(params).to(dev))
        eng.sync_shadow()
        eng.feed_x().copy_(x.to(dev))
        eng.feed_y().copy_(y.to(dev))
        eng.forward(True)
        eng.backward_a()
        eng.backward_b()
    torch.cuda.synchronize()
    p = {k: v.clone().float().requires_grad_(True) for k, v in params.items()}
    logits = M.conv_net(x, p, 1.0, emulate_bf16=True)
    loss_rows = torch.nn.functional.cross_entropy(logits, y.long(), reduction="none")
    loss_rows.mean().backward()
    g = M.dict_from_flat(eng.grads().cpu())
    out = {"loss": rel(eng.loss_rows().cpu(), loss_rows.detach())}
    out.update({k: rel(g[k].float(), p[k].grad) for k in p})
    return out


def _fmt(m):
    by = {}
    for (t, s), (e, i) in m.items():
        by.setdefault(t, []).append(f"{s}={e:.2e}@{i}")
    return by


def slices(seeds, dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mnist_oracle as O

    worst = {}

    def run(name, dtype, params, x, y, keep=1.0, count=True, follow=True):
        mask = M.native_dropout_mask(x.shape[0], 0, 0, 1234, keep) if keep < 1.0 else None
        got = O.run_engine(dev, dtype, params, x, y, keep)
        ref = O.oracle_step(params, x, y, dtype, keep, mask, follow=got if follow else None)
        m = O.measure(got, ref)
        for t, parts in _fmt(m).items():
            print(f"{dtype} {name} {t}: " + " ".join(parts), flush=True)
        if count:
            for k, (e, _) in m.items():
                if e > worst.get((dtype, k), (-1.0, ""))[0]:
                    worst[(dtype, k)] = (e, name)

    print("# calibration set: (scale, B) x seeds, keep 1 unless stated")
    for dtype in ("bf16", "fp32"):
        cases = [(s, B, 1.0) for s, B in O.STANDARD] + [(0.05, B, 1.0) for B in O.EDGE_BATCHES] + [(0.05, 37, 0.75)]
        for scale, B, keep in cases:
            for seed in seeds:
                params, x, y = O.random_case(B, scale, seed)
                run(f"scale={scale} B={B} keep={keep} seed={seed}", dtype, params, x, y, keep)
    print("# special inputs (reported; not part of the bounds)")
    for dtype in ("bf16", "fp32"):
        for B in (5, 37):
            run(f"integer B={B}", dtype, *O.integer_case(B), count=False, follow=False)
        for B in (9, 37):
            run(f"impulse B={B}", dtype, *O.impulse_case(B), count=False)
        for B in (6, 3):
            for rev in (False, True):
                run(f"neighbours B={B} reverse={rev}", dtype, *O.neighbours_case(B, rev), count=False)
        for lab in ("zeros", "nines", "argmin"):
            run(f"saturated B=37 labels={lab}", dtype, *O.saturated_case(37, lab), count=False)
    print("# bounds: 3x the worst of each class over the calibration set (dtype tensor slicing worst where bound)")
    for (dtype, (t, s)), (e, name) in sorted(worst.items()):
        print(f"bound {dtype} {t} {s} {e:.3e} [{name}] {3 * e:.3e}")


def fused(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mnist_oracle as O

    worst = {}
    ratios = {}

    def run(name, dtype, B, keep=1.0, local_bf16=False, step0=0, update=False, **kw):
        res = O.run_fused_step(dev, dtype, *O.random_case(B), keep=keep, local_bf16=local_bf16, step0=step0, **kw)
        ref = O.fused_oracle(res, dtype, keep, step0)
        bf = local_bf16 and dtype == "bf16"
        table = O.measure_fused(res, ref, dtype, bf, only=O.GRADS)
        by = {}
        for (t, s), (e, b, i) in sorted(table.items()):
            by.setdefault(t, []).append(f"{s}={e:.2e}/{b:.2e}@{i}{'' if e <= b else ' ABOVE'}")
            w = worst.get((dtype, bf, (t, s)), (-1.0, 0.0, ""))
            if e / b > w[0]:
                worst[(dtype, bf, (t, s))] = (e / b, e, f"{name} B={B}")
        for t, parts in by.items():
            print(f"{dtype} {name} B={B} {t}: " + " ".join(parts), flush=True)
        if update:
            r = O.update_ratios(res)
            print(f"{dtype} {name} B={B} update t={res['t']}: v ratio {r['v'][0]:.3f}@{r['v'][1]} "
                  f"p ratio {r['p'][0]:.3f}@{r['p'][1]}", flush=True)
            for k in ("v", "p"):
                ratios[(dtype, k)] = max(ratios.get((dtype, k), 0.0), r[k][0])

    print("# fused one-GPU Adam step: class=error/bound@worst index; bound = BOUNDS + fused_allowance")
    print("# consumed gradient: feed mode, keep 1, fp32 fc gradients")
    for dtype in ("bf16", "fp32"):
        for B in O.FUSED_BATCHES[dtype]:
            run("edge", dtype, B)
    print("# the benchmark's settings: bf16, bf16 fc gradients, dataset mode, keep 0.75")
    for B in (5, 37, 130):
        run("bench", "bf16", B, keep=0.75, local_bf16=True, dataset=True)
    print("# later steps: global step 2, dataset mode, keep 0.75")
    for dtype in ("bf16", "fp32"):
        run("step2", dtype, 37, keep=0.75, dataset=True, step0=2)
    print("# tail instantiations at global step 1: lr 1e-4, schedule lr 1e-4 * 0.5^s, EMA 0.99 with num_updates")
    for variant in ("sched", "ema", "sched+ema"):
        for dtype in ("bf16", "fp32"):
            for B in (3, 130):
                run(variant, dtype, B, step0=1, update=True, lr=O.FUSED_LR, schedule=O.FUSED_SCHEDULE if "sched" in variant else None,
                    ema=O.FUSED_EMA if "ema" in variant else None)
    print("# update from the consumed gradient: B = 37, dataset mode, keep 0.75; ratios are error / tolerance")
    for step0 in (0, 2):
        for dtype in ("bf16", "fp32"):
            for lb in (False, True):
                run(f"update step0={step0} local_bf16={int(lb)}", dtype, 37, keep=0.75, local_bf16=lb, dataset=True,
                    step0=step0, update=True)
    print("# not part of the tests: the fp32 B = 3 case at global step 1 after one step at lr 0.01 (logits +-45), the fused")
    print("# step and the unfused kernels at the same parameters (see FUSED_LR in tests/mnist_oracle.py)")
    res = O.run_fused_step(dev, "fp32", *O.random_case(3), step0=1)
    ref = O.fused_oracle(res, "fp32", 1.0, 1)
    pd = {k: v.clone() for k, v in M.dict_from_flat(res["p_before"]).items()}
    got = O.run_engine(dev, "fp32", pd, res["x"], res["y"])
    m_un = O.measure(got, O.oracle_step(pd, res["x"], res["y"], "fp32", follow=got))
    gu = O.fused_got(res)["grads"]
    print(f"max |logit| {ref['logits'].abs().max().item():.1f}")
    for (t, s), (e, b, i) in sorted(O.measure_fused(res, ref, "fp32", False, only=O.GRADS).items()):
        print(f"fp32 lr=0.01 B=3 {t} {s}: fused {e:.2e} unfused {m_un[(t, s)][0]:.2e} bound {b:.2e}")
    for t in O.GRADS:
        print(f"fp32 lr=0.01 B=3 {t}: |fused - unfused| / |unfused| = "
              f"{((gu[t] - got['grads'][t]).norm() / got['grads'][t].norm()).item():.2e}")
    print("# worst error / bound of each class (dtype, bf16 fc gradients, tensor, slicing, ratio, error, where)")
    for (dtype, bf, (t, s)), (r, e, name) in sorted(worst.items()):
        print(f"worst {dtype} local_bf16={int(bf)} {t} {s} {r:.3f} {e:.3e} [{name}]")
    print("# worst update ratios (v: 2^-22 relative; p: 2^-24 |p_ref| + 2^-18 |dp_ref|)")
    for (dtype, k), r in sorted(ratios.items()):
        print(f"worst {dtype} {k} ratio {r:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--slices", action="store_true", help="per-slice errors against the fp64 oracle")
    ap.add_argument("--fused", action="store_true", help="the fused one-GPU Adam step's consumed gradient and update")
    a = ap.parse_args()
    _native.require()
    dev = torch.device("cuda", 0)
    seeds = [int(s) for s in a.seeds.split(",")]
    if a.slices:
        slices(seeds, dev)
        return
    if a.fused:
        fused(dev)
        return
    worst = {}
    for scale, B in CONFIGS:
        for seed in seeds:
            r = measure(scale, B, seed, dev)
            print(f"scale={scale} B={B} seed={seed} " + " ".join(f"{k}={v:.2e}" for k, v in r.items()), flush=True)
            for k, v in r.items():
                worst[(scale, B, k)] = max(worst.get((scale, B, k), 0.0), v)
    print("# worst per (scale, B, tensor):")
    for (scale, B, k), v in sorted(worst.items()):
        print(f"  {scale} {B} {k}: {v:.3e}")


if __name__ == "__main__":
    main()
