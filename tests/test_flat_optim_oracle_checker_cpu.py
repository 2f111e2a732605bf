"""The criterion of tests/flat_optim_oracle.py, checked on the host: a numpy fp32 model of the flat kernels
(csrc/optim_kernels.h: adam_apply4 and the scalar tails -- one expression --, sgd_kernel; every operation rounded
separately, powf modelled as correctly rounded) stays within the derived bounds over magnitudes spread across six
to twelve decades, and each planted error is refused. Then the old criterion (rtol=1e-5, atol=1e-6 on p, the one
the flat kernels had before) on the same inputs, and a host model of adam_ranges_kernel's index map against a
plain enumeration of the ranges.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flat_optim_oracle as FO  # noqa: E402

F = np.float32
N = 200_000
T_LIST = (1, 2, 3, 10, 100, 1000, 20000)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
GS, GC = 0.5, 0.75  # grad_scale and *gscale
ADAM_MUTATIONS = ("c2_from_beta1", "no_bias_correction", "t_minus_1", "gg_unscaled", "eps_in_root", "old_m")
SGD_MUTATIONS = ("nesterov_old_accum", "wd_after_mult", "no_grad_scale")


# ---------------------------------------------------------------- the fp32 model
def model_adam(p, m, v, gw, t, lr, beta1, beta2, eps, grad_scale=1.0, gscale=1.0, mut=None):
    lr, b1, b2, eps = F(lr), F(beta1), F(beta2), F(eps)
    mult = F(grad_scale) * F(gscale)
    g = gw.astype(F) * mult
    c1 = F(1) - b1
    c2 = F(1) - (b1 if mut == "c2_from_beta1" else b2)
    tt = t - 1 if mut == "t_minus_1" else t
    b1p, b2p = F(float(b1) ** tt), F(float(b2) ** tt)
    with np.errstate(divide="ignore", invalid="ignore"):
        lr_t = lr if mut == "no_bias_correction" else lr * np.sqrt(F(1) - b2p) / (F(1) - b1p)
        m2 = m + (g - m) * c1
        gg = gw.astype(F) * gw.astype(F) if mut == "gg_unscaled" else g * g
        v2 = v + (gg - v) * c2
        den = np.sqrt(v2 + eps) if mut == "eps_in_root" else np.sqrt(v2) + eps
        p2 = p - lr_t * (m if mut == "old_m" else m2) / den
    assert p2.dtype == m2.dtype == v2.dtype == F
    return {"p": p2, "m": m2, "v": v2}


def model_sgd(p, mom, gw, lr, momentum, weight_decay, nesterov, grad_scale=1.0, gscale=1.0, mut=None):
    lr, mu, wd = F(lr), F(momentum), F(weight_decay)
    mult = F(gscale) if mut == "no_grad_scale" else F(grad_scale) * F(gscale)
    if mut == "wd_after_mult":
        g = (gw.astype(F) + wd * p) * mult
    else:
        g = gw.astype(F) * mult + wd * p
    if mom is None:
        return {"p": p - lr * g}
    acc = mom * mu + g
    if nesterov:
        p2 = p - lr * (g + mu * (mom if mut == "nesterov_old_accum" else acc))
    else:
        p2 = p - lr * acc
    assert p2.dtype == acc.dtype == F
    return {"p": p2, "mom": acc}


# ---------------------------------------------------------------- inputs
def _decades(rng, n, lo, hi, signed=True):
    x = 10.0 ** rng.uniform(lo, hi, n)
    return (x * (rng.choice([-1.0, 1.0], n) if signed else 1.0)).astype(F)


def _as_dtype(g, gdt):
    return torch.from_numpy(g).to(gdt).float().numpy()


def spread_inputs(seed, gdt):
    """g over six decades (|g| >= 1e-6), m over six, v over twelve."""
    rng = np.random.default_rng(seed)
    g = _as_dtype(_decades(rng, N, -6, 0), gdt)
    return dict(p=(rng.standard_normal(N) * 0.05).astype(F), m=_decades(rng, N, -7, -1),
                v=_decades(rng, N, -12, 0, signed=False), gw=g)


def usual_inputs(seed, gdt):
    """What the earlier tests of the flat ops fed them: |p| ~ 0.05, g ~ 0.01, slots as after some updates."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(N) * 0.01
    g = np.where(np.abs(g) < 1e-6, 1e-6, g).astype(F)
    return dict(p=(rng.standard_normal(N) * 0.05).astype(F), m=(rng.standard_normal(N) * 1e-3).astype(F),
                v=(rng.uniform(1e-4, 1.1e-3, N)).astype(F), gw=_as_dtype(g, gdt))


def _t(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def _adam_check(x, t, mut=None):
    dev = model_adam(x["p"], x["m"], x["v"], x["gw"], t, grad_scale=GS, gscale=GC, mut=mut, **HYPER)
    ref, tol = FO.adam_ref(*(torch.from_numpy(x[k]) for k in ("p", "m", "v", "gw")), t, HYPER["lr"], HYPER["beta1"],
                           HYPER["beta2"], HYPER["eps"], GS, GC)
    keys = {}
    ok, worst = FO.check(_t(dev), ref, tol, by_key=keys)
    return ok, worst, keys, FO.outside(_t(dev), ref, tol), dev, ref


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_fp32_model_of_adam_stays_within_the_bounds_and_mutations_do_not(gdt):
    for i, t in enumerate(T_LIST):
        x = spread_inputs(100 + i, gdt)
        ok, worst, keys, _, _, _ = _adam_check(x, t)
        print(f"adam model t={t} {str(gdt).split('.')[-1]}: worst err / bound " + ", ".join(f"{k} {w:.3f}" for k, w in keys.items()))
        assert ok and 0 < worst <= 1, (t, keys)
        for mut in ADAM_MUTATIONS:
            bad_ok, _, _, frac, _, _ = _adam_check(x, t, mut)
            if mut in ("no_bias_correction", "t_minus_1") and t == 20000:
                continue  # the correction is 1 in fp32 there, at t - 1 too: why small t are in every test set
            assert not bad_ok, (mut, t)
            print(f"  {mut}: {100 * frac:.1f} % of p' outside")


def test_k_pow_is_felt_only_where_the_power_is():
    """E_lr at t = 1 is dominated by the power's term (b2 / (1 - b2) = 999 at the defaults) and falls to a few U
    once b^t is small: the bound is not a blanket tolerance."""
    e = [FO.e_lr(0.9, 0.999, t) for t in FO.LR_T_PROBE_T]
    assert e[0] > 500 * FO.U * FO.K_POW and all(a > b for a, b in zip(e, e[1:-1])) and e[-1] < 9 * FO.U
    assert FO.e_lr(0.9, 0.999, 1, k_pow=4) > FO.e_lr(0.9, 0.999, 1, k_pow=2)
    assert 2 <= FO.K_POW <= 8 and int(FO.K_POW) == FO.K_POW


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_fp32_model_of_sgd_stays_within_the_bounds_and_mutations_do_not(gdt):
    cases = [dict(momentum=0.9, weight_decay=1e-4, nesterov=False), dict(momentum=0.9, weight_decay=1e-4, nesterov=True),
             dict(momentum=0.9, weight_decay=0.0, nesterov=True), dict(momentum=None, weight_decay=1e-4, nesterov=False)]
    for i, c in enumerate(cases):
        x = spread_inputs(200 + i, gdt)
        mom = x["m"] if c["momentum"] is not None else None
        mu = c["momentum"] or 0.0

        def run(mut=None):
            dev = model_sgd(x["p"], mom, x["gw"], 0.01, mu, c["weight_decay"], c["nesterov"], GS, GC, mut)
            ref, tol = FO.sgd_ref(torch.from_numpy(x["p"]), None if mom is None else torch.from_numpy(mom),
                                  torch.from_numpy(x["gw"]), 0.01, mu, c["weight_decay"], c["nesterov"], GS, GC)
            keys = {}
            ok, worst = FO.check(_t(dev), ref, tol, by_key=keys)
            return ok, worst, keys

        ok, worst, keys = run()
        print(f"sgd model {c} {str(gdt).split('.')[-1]}: worst err / bound " + ", ".join(f"{k} {w:.3f}" for k, w in keys.items()))
        assert ok and 0 < worst <= 1, (c, keys)
        assert not run("no_grad_scale")[0], c
        if c["weight_decay"]:
            assert not run("wd_after_mult")[0], c
        if c["nesterov"] and mom is not None:
            assert not run("nesterov_old_accum")[0], c


def test_old_criterion_accepts_what_the_oracle_refuses():
    """On inputs like those the flat ops' earlier tests used, at t = 100 and 1000: the oracle refuses every planted
    error (fraction of p' outside its bound: 1.00 for the missing bias correction and the old m, 0.997 for c2 from
    beta1, 0.81-0.97 for t - 1, 0.22-0.35 for g^2 from the unscaled gradient, 0.05-0.12 for eps inside the root,
    whose effect at sqrt(v) ~ 0.02 is a few 1e-5 of the update). np.allclose(rtol=1e-5, atol=1e-6) on p -- all the
    flat kernels were held to -- ACCEPTED three of the six at both t: t - 1 for t, g^2 from the unscaled gradient
    and eps inside the root."""
    accepted, fracs = {}, {}
    for t in (100, 1000):
        x = usual_inputs(7 + t, torch.float32)
        assert _adam_check(x, t)[0]
        for mut in ADAM_MUTATIONS:
            bad_ok, _, _, frac, dev, ref = _adam_check(x, t, mut)
            assert not bad_ok, (mut, t, frac)
            fracs[(mut, t)] = round(frac, 3)
            if np.allclose(dev["p"], ref["p"].numpy(), rtol=1e-5, atol=1e-6):
                accepted.setdefault(t, []).append(mut)
    print("old criterion accepted:", accepted, "; fraction of p' outside the oracle's bound:", fracs)
    for t in (100, 1000):
        assert "eps_in_root" in accepted[t] and "t_minus_1" in accepted[t], accepted


# ---------------------------------------------------------------- the ranges index map
def model_ranges(table):
    """make_adam_ranges and adam_ranges_kernel's phys(), in float4 units: (physical float4 index of every
    logical one, the tail's elements). Raises where the launcher does."""
    nr = len(table)
    if not 1 <= nr <= 3:
        raise ValueError("1..3 ranges")
    beg4, pre4 = [], [0]
    for k, (beg, n) in enumerate(table):
        if beg % 4 or (k < nr - 1 and n % 4):
            raise ValueError("unaligned range")
        beg4.append(beg // 4)
        pre4.append(pre4[-1] + n // 4)
    lbeg, ln = table[-1]
    tail = list(range(lbeg + ln // 4 * 4, lbeg + ln))

    def phys(i):
        k = 0 if i < pre4[1] else (2 if nr > 2 and i >= pre4[2] else 1)
        return beg4[k] + (i - pre4[k])

    return [phys(i) for i in range(pre4[nr])], tail


@pytest.mark.parametrize("name", [k for k, v in FO.range_tables().items() if FO.table_extent(v) <= 8192])
def test_ranges_index_map_is_the_plain_enumeration(name):
    table = FO.range_tables()[name]
    f4, tail = model_ranges(table)
    got = sorted([4 * q + j for q in f4 for j in range(4)] + tail)
    want = [e for beg, n in table for e in range(beg, beg + n)]
    assert got == want and len(set(got)) == len(got), name
    assert len(tail) == table[-1][1] % 4 < 4


def test_ranges_index_map_large_tables_and_refusals():
    """The large tables (past the grid, MNIST's ZeRO-1 shards) through a vectorised copy of the same map."""
    for name, table in FO.range_tables().items():
        if FO.table_extent(table) <= 8192:
            continue
        nr = len(table)
        beg4 = np.array([b // 4 for b, _ in table])
        pre4 = np.cumsum([0] + [n // 4 for _, n in table])
        assert all(b % 4 == 0 for b, _ in table) and all(n % 4 == 0 for _, n in table[:-1])
        i = np.arange(pre4[nr])
        k = np.where(i < pre4[1], 0, np.where((nr > 2) & (i >= pre4[min(2, nr)]), 2, 1))
        k = np.minimum(k, nr - 1)
        phys = beg4[k] + (i - pre4[k])
        mask = np.zeros(FO.table_extent(table), dtype=np.int32)
        np.add.at(mask, (4 * phys[:, None] + np.arange(4)[None, :]).ravel(), 1)
        lbeg, ln = table[-1]
        mask[lbeg + ln // 4 * 4:lbeg + ln] += 1
        assert np.array_equal(mask, FO.range_mask(table, mask.size).numpy().astype(np.int32)), name
    # the second pass of three_past_the_grid starts inside the second range and ends in the third
    t = FO.range_tables()["three_past_the_grid"]
    pre = np.cumsum([0] + [n // 4 for _, n in t])
    assert pre[1] < FO.GRID4 // 4 < pre[2] < pre[3]
    for bad in ([(2, 8)], [(0, 6), (8, 4)], [(0, 4), (8, 4), (16, 4), (24, 4)], []):
        with pytest.raises(ValueError):
            model_ranges(bad)
