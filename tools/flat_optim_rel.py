"""The flat Adam / Momentum / SGD kernels against their fp64 oracle: the figures behind tests/flat_optim_oracle.py.

1. The device's bias-corrected rate lr_t, read bit for bit through the probe of the GPU test (p = 0, m = v = g = 1,
   eps = 0: p' = -lr_t), against the fp64 lr_t at every t of LR_T_PROBE_T, constant and scheduled, beta2 = 0.999 and
   0.99: the relative error in units of U = 2^-24, E_lr at K_pow = 2 and their ratio; then the smallest integer
   K_pow >= 2 at which error / E_lr <= 0.5 at every t -- the K_POW of the oracle. Above 8 it is a finding about
   powf, not a tolerance.
2. Whether powf(x, 1) == x held (the exact Adam case: p' = 0.75 bit for bit).
3. One update through every variant, gradient dtype and size of the GPU test: the worst error / bound of each
   quantity (tests/test_flat_optim_oracle_gpu.py's inputs and helpers).

    python tools/flat_optim_rel.py > profiles/flat_optim_rel.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tensorflow_distributed_amd import _native  # noqa: E402


def lr_t_table(dev, FO, T):
    rows, worst = [], {}
    print("# 1. lr_t: instantiation beta2 t device_lr_t fp64_lr_t rel_err/U E_lr(K_pow=2)/U err/E_lr(K_pow=2)")
    for sched, label in ((None, "const"), (T.PROBE_SCHED, "sched")):
        for beta2 in (0.999, 0.99):
            for t in FO.LR_T_PROBE_T:
                got, err, _ = FO.probe_lr_t(dev, t, T.LR, T.B1, beta2, sched)
                want = FO.lr_t_ref(T._rate(sched, T.LR, t), T.B1, beta2, t)
                e2 = FO.e_lr(T.B1, beta2, t, k_pow=2)
                rows.append((beta2, t, err))
                print("%s %.3f %7d %.9e %.9e %8.3f %9.3f %.4f" % (label, beta2, t, got, want, err / FO.U, e2 / FO.U, err / e2))
    k_pow = None
    for k in range(2, 9):
        worst[k] = max(err / FO.e_lr(T.B1, b2, t, k_pow=k) for b2, t, err in rows)
        if k_pow is None and worst[k] <= 0.5:
            k_pow = k
    print("worst err / E_lr by K_pow: " + ", ".join("%d: %.4f" % kv for kv in worst.items()))
    if k_pow is None:
        print("K_pow would have to exceed 8: a finding about the device powf, not a tolerance")
    else:
        print("K_pow = %d (the smallest integer >= 2 with err / E_lr <= 0.5 at every t); tests/flat_optim_oracle.py holds K_POW = %d"
              % (k_pow, FO.K_POW))
    return k_pow


def powf_of_one(dev, T):
    n = 4099
    full = lambda x: torch.full((n,), x, device=dev)  # noqa: E731
    p, m, v = full(1.0), full(0.0), full(0.0)
    T._adam(p, m, v, full(1.0), None, lr=0.25, b1=0.5, b2=0.75, eps=0.0, step=None, t_offset=1)
    exact = bool((p == 0.75).all().item()) and bool((m == 0.5).all().item()) and bool((v == 0.25).all().item())
    print("# 2. exact Adam case at t = 1: p' = %r, m' = %r, v' = %r: powf(x, 1) == x %s"
          % (p[0].item(), m[0].item(), v[0].item(), "held" if exact else "did NOT hold"))


def per_size(dev, FO, T):
    print("# 3. one update, worst error / bound: op variant instantiation g_dtype n quantity...")
    step = torch.full((1,), 2, dtype=torch.int64, device=dev)
    for variant in T.VARIANTS:
        for sched, label in ((None, "const"), (T.SCHED, "sched")):
            for gdt in (torch.float32, torch.bfloat16):
                gen = torch.Generator(device=dev).manual_seed(3)
                for n in T.ADAM_SIZES:
                    b = {k: x[1] for k, x in T._adam_state(n, gen, dev, gdt).items()}
                    p0, m0, v0 = b["p"].clone(), b["m"].clone(), b["v"].clone()
                    T._adam(b["p"], b["m"], b["v"], b["g"], b["pbf"], step=step, grad_scale=0.5, sched=sched,
                            **T._mods(variant, dev, b["ema"]))
                    ref, tol = FO.adam_ref(p0, m0, v0, b["g"], 3, T._rate(sched, T.LR, 3), T.B1, T.B2, T.EPS, 0.5)
                    keys = {}
                    ok, _ = FO.check(b, ref, tol, by_key=keys)
                    print("adam %-9s %s %s %8d %s%s" % (variant, label, str(gdt).split(".")[-1], n,
                                                        " ".join("%s %.4f" % kv for kv in keys.items()), "" if ok else "  OUTSIDE"))
                for nesterov, slot, name in ((False, True, "momentum"), (True, True, "nesterov"), (False, False, "sgd")):
                    for n in T.SGD_SIZES:
                        b = {k: x[1] for k, x in T._adam_state(n, gen, dev, gdt).items()}
                        mom = b["m"] if slot else None
                        p0, mom0 = b["p"].clone(), mom.clone() if slot else None
                        mods = T._mods(variant, dev, b["ema"])
                        mods.pop("ema_decay", None)
                        T._sgd(b["p"], mom, b["g"], b["pbf"], nesterov=nesterov, step=step, grad_scale=0.5, sched=sched, **mods)
                        ref, tol = FO.sgd_ref(p0, mom0, b["g"], T._rate(sched, 0.01, 3), T.MOM, T.WD, nesterov, 0.5)
                        keys = {}
                        ok, _ = FO.check({"p": b["p"], "mom": mom}, ref, tol, by_key=keys)
                        print("%-8s %-9s %s %s %8d %s%s" % (name, variant, label, str(gdt).split(".")[-1], n,
                                                            " ".join("%s %.4f" % kv for kv in keys.items()), "" if ok else "  OUTSIDE"))


def main():
    _native.require()
    import flat_optim_oracle as FO
    import test_flat_optim_oracle_gpu as T

    dev = torch.device("cuda", 0)
    print("# %s; flat optimizer kernels against the fp64 oracle of tests/flat_optim_oracle.py, U = 2^-24" % torch.cuda.get_device_name(0))
    k_pow = lr_t_table(dev, FO, T)
    powf_of_one(dev, T)
    per_size(dev, FO, T)
    return 0 if k_pow is not None else 1


if __name__ == "__main__":
    sys.exit(main())
