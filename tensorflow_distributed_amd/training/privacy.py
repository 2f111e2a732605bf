"""A small privacy accountant for DP-SGD: Renyi differential privacy of the sampled Gaussian mechanism.

One step with sampling rate ``q`` and noise multiplier ``sigma`` has, at an integer order ``alpha >= 2``,

    RDP(alpha) = log( sum_{k=0}^{alpha} C(alpha, k) (1 - q)^(alpha - k) q^k exp((k^2 - k) / (2 sigma^2)) ) / (alpha - 1)

(Mironov, Talwar, Zhang 2019, the closed binomial form). RDP adds over steps, and
``epsilon = min_alpha steps * RDP(alpha) + log(1 / delta) / (alpha - 1)``.

The bound ASSUMES POISSON SAMPLING: every example enters each batch independently with probability ``q``. The
training loops here walk a per-epoch shuffle in fixed batches of ``batch`` rows with ``q = batch / n_train``, which
does not meet it, so the reported epsilon is the customary approximation and not a guarantee -- TF Privacy's own
caveat for its MNIST tutorial.
"""
from __future__ import annotations

import math

ORDERS = tuple(range(2, 257))


def rdp_sampled_gaussian(q: float, sigma: float, alpha: int) -> float:
    """RDP of one step at integer order ``alpha >= 2``"""
    assert 0.0 <= q <= 1.0 and int(alpha) == alpha and alpha >= 2
    if q == 0.0:
        return 0.0
    if sigma == 0.0:
        return math.inf
    if q == 1.0:
        return alpha / (2.0 * sigma ** 2)
    terms = [math.lgamma(alpha + 1) - math.lgamma(k + 1) - math.lgamma(alpha - k + 1) + (alpha - k) * math.log1p(-q) +
             k * math.log(q) + (k * k - k) / (2.0 * sigma ** 2) for k in range(alpha + 1)]
    top = max(terms)
    return (top + math.log(sum(math.exp(t - top) for t in terms))) / (alpha - 1)


def rdp_per_step(q: float, sigma: float, orders=ORDERS) -> list:
    """one step's RDP at every order: computed once per run, so that a per-step epsilon costs one pass over the orders"""
    return [rdp_sampled_gaussian(q, sigma, a) for a in orders]


def epsilon_from_rdp(rdp, steps: int, delta: float, orders=ORDERS) -> float:
    """``epsilon`` after ``steps`` steps of a mechanism whose one step has ``rdp[i]`` at ``orders[i]``"""
    if steps <= 0 or not any(rdp):
        return 0.0
    return min(steps * r + math.log(1.0 / delta) / (a - 1) for r, a in zip(rdp, orders))


def epsilon(q: float, sigma: float, steps: int, delta: float, orders=ORDERS) -> float:
    """``epsilon`` of ``steps`` steps at ``(q, sigma)`` for the given ``delta`` (Poisson sampling assumed: see above)"""
    if steps <= 0 or q == 0.0:
        return 0.0
    if sigma <= 0.0:
        return math.inf
    return epsilon_from_rdp(rdp_per_step(q, sigma, orders), steps, delta, orders)
