"""The fp64 oracle of the flat Adam / Momentum / SGD kernels (csrc/optim_kernels.h: adam_kernel, its scalar tail,
adam_ranges_kernel, sgd_kernel) with per-element bounds derived from the kernels' own roundings. Importable
without a GPU: tests/test_flat_optim_oracle_gpu.py holds the device to it, tests/test_flat_optim_oracle_checker_cpu.py
holds a numpy fp32 model of the kernels and planted errors to it, tools/flat_optim_rel.py records the figures.

The reference. training/optimizers.py's adam_update / momentum_update in fp64, from the fp32 state the kernel
read and from the fp32 values the kernel received for every scalar: lr, beta1, beta2, eps, grad_scale, *gscale,
momentum, weight_decay are each float(np.float32(x)) (f32 below). 1 - fp32(0.999) differs from 0.001 by 1.3e-5
relative; that is TF's behaviour too and no error of the kernel.

The bounds. Per element, to first order, U = 2^-24 (half an ulp relative: one fp32 rounding). Each line counts
the un-contracted form; -ffp-contract=fast, the only fast-math flag of the build, only removes roundings (a
product that is contracted into the sum behind it is not rounded). sqrtf and the division are the correctly
rounded ones (hipcc's default); the lines count them at 2 U and U.

Adam (adam_apply4 and the scalar tails, the same expression):

    g   = gw * mult                  |dg|  <= 2U|g|         mult = grad_scale * *gscale rounds once, the product once
    c   = 1 - beta                   E_c   =  U             relative; exact for beta >= 0.5
    a   = g - m                      |da|  <= |dg| + U|a|
    m'  = m + a c1                   |dm'| <= c1(|da| + |a|(E_c + U)) + U|m'|
    gg  = g g                        |dgg| <= 5U gg         g twice at 2U, the product
    a2  = gg - v                     |da2| <= |dgg| + U|a2|
    v'  = v + a2 c2                  |dv'| <= c2(|da2| + |a2|(E_c + U)) + U|v'|
    s   = sqrtf(v')                  |ds|  <= |dv'| / (2 s) + 2U s       (v' = 0: sqrt(|dv'|))
    den = s + eps                    |dden| <= |ds| + U den
    lr_t = lr sqrtf(1 - b2^t) / (1 - b1^t), relative:
          E_lr = E_base + (E_pow b2^t/(1 - b2^t) + U)/2 + 2U + (E_pow b1^t/(1 - b1^t) + U) + 4U
          -- the power's error E_pow = 2 K_pow U relative to b^t is E_pow b^t / (1 - b^t) relative to 1 - b^t, the
          subtraction rounds once; the root halves its operand's error and rounds (2U); the quotient's operand
          likewise without the halving; 4U for lr's product, the quotient and (float)t's neighbours. E_base is
          the error of the schedule's rate: 0 for a constant and for a piecewise schedule of powers of two.
    upd = lr_t m' / den              |dupd| <= |upd|(E_lr + 3U + |dden|/den) + lr_t |dm'| / den
    p'  = p - upd                    |dp'| <= |dupd| + U|p'|

Momentum / SGD (sgd_kernel):

    g = gw*mult + wd*p               |dg|   <= 2U|gw mult| + U|wd p| + U|g|
    acc = mom*mu + g                 |dacc| <= U|mom mu| + |dg| + U|acc|
    p' = p - lr*acc                  |dp'|  <= lr(|dacc| + U|acc|) + U|p'|
    nesterov: inner = g + mu*acc     |di|   <= |dg| + mu|dacc| + U|mu acc| + U|inner|
              p' = p - lr*inner      |dp'|  <= lr(|di| + U|inner|) + U|p'|
    no mom slot: p' = p - lr*g       |dp'|  <= lr(|dg| + U|g|) + U|p'|

2^-126 is added to every bound: an underflowing result carries no relative precision. Test gradients stay at
|g| >= 1e-6 so that g g (>= 1e-12) and the slots built from it are normal numbers.

The worst error / bound of p' and v' sits just under 1 wherever the result lies right above a power of two:
there the final rounding U|x'| is all but the whole bound and half an ulp is all but U|x'| (tests/test_rules_gpu.py
notes the same). m's ratio, and the planted errors of the checker test, speak about the arithmetic.

K_POW is the one constant that is measured, not derived: the accuracy of the device powf in ulps, read through
the lr_t probe of the GPU test (p = 0, m = v = g = 1, eps = 0 leave p' = -lr_t bit for bit). It is the smallest
integer >= 2 at which the probe's observed error is at most half of E_lr at every t of LR_T_PROBE_T, for
beta2 = 0.999 and 0.99: profiles/flat_optim_rel.txt holds the table (tools/flat_optim_rel.py writes it).
"""
import math

import numpy as np
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O

U = 2.0 ** -24      # fp32 unit roundoff
TINY = 2.0 ** -126  # the smallest normal fp32
# ulps of the device powf. Measured on an MI355X (profiles/flat_optim_rel.txt, the lr_t table): at K_pow = 2, the floor,
# the worst error / E_lr over the 36 probes is 0.11 (t = 1000, beta2 = 0.99; 0.06-0.10 at t = 2, 3 where the power's
# term is nearly all of E_lr), below the 0.5 asked for; powf(x, 1) == x held.
K_POW = 2
LR_T_PROBE_T = (1, 2, 3, 10, 100, 1000, 6931, 20000, 10 ** 6)
GRID4 = 2048 * 256 * 4  # adam_kernel's largest grid x 256 lanes x 4: above it a second grid-stride pass
GRID1 = 2048 * 256      # sgd_kernel's


def f32(x):
    """The value the kernel received for the host double x."""
    return float(np.float32(x))


def f64(x):
    return torch.as_tensor(x).detach().to(torch.float64)


def lr_t_ref(lr, beta1, beta2, t):
    """lr sqrt(1 - b2^t) / (1 - b1^t) in fp64 from the fp32 scalars (lr: the rate of this update)."""
    b1, b2 = f32(beta1), f32(beta2)
    return f32(lr) * math.sqrt(1.0 - b2 ** int(t)) / (1.0 - b1 ** int(t))


def e_lr(beta1, beta2, t, k_pow=None, e_base=0.0):
    """E_lr: the relative bound of the device's lr_t."""
    k = K_POW if k_pow is None else k_pow
    e_pow = 2.0 * k * U
    b1p, b2p = f32(beta1) ** int(t), f32(beta2) ** int(t)
    return e_base + (e_pow * b2p / (1.0 - b2p) + U) / 2 + 2 * U + (e_pow * b1p / (1.0 - b1p) + U) + 4 * U


def adam_ref(p, m, v, gw, t, lr, beta1, beta2, eps, grad_scale=1.0, gscale=1.0, k_pow=None, e_base=0.0):
    """(reference, bounds) of one Adam update: dicts over "p", "m", "v" of fp64 tensors. p, m, v: the fp32 state
    before the update; gw: the gradient as the kernel read it (fp32, or bf16: exact in fp32); t: Adam's t; lr: the
    rate of this update (the schedule's value at t - 1)."""
    p, m, v = f64(p), f64(m), f64(v)
    b1, b2, ep = f32(beta1), f32(beta2), f32(eps)
    g = f64(gw) * (f32(grad_scale) * f32(gscale))
    p2, m2, v2 = O.adam_update(p, m, v, g, t, f32(lr), b1, b2, ep)
    c1, c2 = 1.0 - b1, 1.0 - b2
    dg = 2 * U * g.abs()
    a = (g - m).abs()
    dm = c1 * (dg + U * a + a * 2 * U) + U * m2.abs()
    gg = g * g
    a2 = (gg - v).abs()
    dv = c2 * (5 * U * gg + U * a2 + a2 * 2 * U) + U * v2.abs()
    s = v2.sqrt()
    ds = torch.where(s > 0, dv / (2 * s).clamp_min(TINY) + 2 * U * s, dv.sqrt())
    den = s + ep
    dden = ds + U * den
    lr_t = lr_t_ref(lr, beta1, beta2, t)
    upd = lr_t * m2 / den
    dupd = upd.abs() * (e_lr(beta1, beta2, t, k_pow, e_base) + 3 * U + dden / den) + abs(lr_t) * dm / den
    dp = dupd + U * p2.abs()
    return {"p": p2, "m": m2, "v": v2}, {"p": dp + TINY, "m": dm + TINY, "v": dv + TINY}


def sgd_ref(p, mom, gw, lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0, gscale=1.0):
    """(reference, bounds) of one Momentum / GradientDescent update: dicts over "p" and, with a slot, "mom"."""
    p = f64(p)
    lr32, mu, wd = f32(lr), f32(momentum), f32(weight_decay)
    gs = f64(gw) * (f32(grad_scale) * f32(gscale))
    p2, a2 = O.momentum_update(p, mom, gs, lr32, mu, wd, nesterov)
    g = gs + wd * p
    dg = 2 * U * gs.abs() + U * (wd * p).abs() + U * g.abs()
    if mom is None:
        return {"p": p2}, {"p": abs(lr32) * (dg + U * g.abs()) + U * p2.abs() + TINY}
    dacc = U * (f64(mom) * mu).abs() + dg + U * a2.abs()
    if nesterov:
        inner = g + mu * a2
        di = dg + mu * dacc + U * (mu * a2).abs() + U * inner.abs()
        dp = abs(lr32) * (di + U * inner.abs()) + U * p2.abs()
    else:
        dp = abs(lr32) * (dacc + U * a2.abs()) + U * p2.abs()
    return {"p": p2, "mom": a2}, {"p": dp + TINY, "mom": dacc + TINY}


def check(dev, ref, tol, by_key=None, where=None):
    """(ok, worst error / bound) of the results dev against the reference, element by element; by_key: a dict
    that collects the worst ratio of each quantity; where: a boolean mask of the elements to look at."""
    worst, ok = 0.0, True
    for k in ref:
        err = (f64(dev[k]) - ref[k]).abs()
        bound = tol[k]
        if where is not None:
            err, bound = err[where], bound[where]
        if err.numel() == 0:
            continue
        ok = ok and bool((err <= bound).all().item())
        w = float((err / bound).max().item())
        worst = max(worst, w)
        if by_key is not None:
            by_key[k] = max(by_key.get(k, 0.0), w)
    return ok, worst


def outside(dev, ref, tol, key="p"):
    """The fraction of elements of `key` outside their bound."""
    return float(((f64(dev[key]) - ref[key]).abs() > tol[key]).double().mean().item())


def probe_lr_t(device, t, lr, beta1, beta2, sched=None, n=1031):
    """The device's bias-corrected rate at Adam's t, read bit for bit: p = 0, m = v = g = 1, eps = 0 and a
    multiplier of 1 leave m' = v' = 1 and p' = -lr_t. -> (device lr_t, its relative error against the fp64 one,
    E_lr). Every element of the launch (float4 items of two blocks and a scalar tail) must carry the same bits.
    sched: a piecewise schedule of powers of two (E_base = 0), read at s = t - 1."""
    p = torch.zeros(n, device=device)
    m, v, g = (torch.ones(n, device=device) for _ in range(3))
    step = torch.full((1,), t - 1, dtype=torch.int64, device=device)
    kind, params, bnd, vals = ("constant", [], [], []) if sched is None else O.schedule_args(sched)
    torch.ops.tfd.adam_flat(p, m, v, g, None, lr if sched is None else params[0], beta1, beta2, 0.0, step, 1.0, 1, kind,
                            params, bnd, vals)
    assert bool((m == 1).all().item()) and bool((v == 1).all().item()), "the probe's slots moved"
    assert bool((p.view(torch.int32) == p.view(torch.int32)[0]).all().item()), "lr_t differs between lanes"
    got = -float(p[0].item())
    want = lr_t_ref(lr if sched is None else O.lr_at(sched, t - 1), beta1, beta2, t)
    return got, abs(got - want) / want, e_lr(beta1, beta2, t)


# ---------------------------------------------------------------- the ranges form
def zero_table(world, rank):
    """MNIST's ZeRO-1 ranges of one rank, as csrc/runtime/mnist_engine.cpp builds them: the conv bucket, this
    rank's shard of the fc1 weight, and everything behind it."""
    wd1, bd1 = M.OFFSETS["wd1"], M.OFFSETS["bd1"]
    shard = (bd1 - wd1) // world
    assert (bd1 - wd1) % (world * 64) == 0
    return [(0, M.BUCKET_SPLIT), (wd1 + rank * shard, shard), (bd1, M.TOTAL - bd1)]


def range_tables():
    """{name: [(beg, n), ...]}: the tables of the ranges tests. A block of adam_ranges_kernel is 256 lanes of one
    float4: 1024 logical elements."""
    big = GRID4 // 2
    t = {
        "one_8": [(0, 8)],
        "one_4_offset": [(4, 4)],
        "one_ragged": [(8, 1027)],
        "one_tail_only": [(4, 2)],                              # block 0's tail and no float4 at all
        "two_4_8": [(0, 4), (8, 8)],
        "two_inside_a_block": [(0, 512), (600, 515)],           # the boundary at logical 512, inside block 0
        "two_on_a_block_edge": [(0, 1024), (2048, 1026)],
        "two_tail_only_last": [(0, 8), (16, 3)],
        "three": [(0, 1024), (1032, 1024), (4096, 7)],
        "three_inside_blocks": [(0, 300), (304, 1500), (2000, 1029)],
        "three_empty_middle": [(0, 8), (16, 0), (32, 9)],
        "three_empty_first": [(0, 0), (8, 12), (64, 6)],
        "three_last_is_one": [(0, 4), (8, 4), (12, 1)],
        "two_last_mod_1": [(0, 8), (16, 9)],
        "two_last_mod_2": [(0, 8), (16, 10)],
        "two_last_mod_3": [(0, 8), (16, 11)],
        # 524800 float4 in front of the last boundary, 525824 in all: the second grid-stride pass (logical float4
        # 524288 on) crosses from the second range into the third
        "three_past_the_grid": [(0, big), (big + 64, big + 2048), (2 * big + 4096, 4099)],
    }
    for world, rank in ((4, 0), (4, 3), (8, 5)):
        z = zero_table(world, rank)
        t[f"zero_w{world}_r{rank}"] = z
        t[f"zero_w{world}_r{rank}_fc"] = z[1:]   # the split schedule's two launches
    t["zero_conv"] = zero_table(4, 0)[:1]
    return t


def range_mask(table, numel, device=None):
    """A boolean mask of the elements inside the ranges, by plain enumeration."""
    mask = torch.zeros(numel, dtype=torch.bool, device=device)
    for beg, n in table:
        mask[beg:beg + n] = True
    return mask


def table_extent(table):
    return max(beg + n for beg, n in table)
