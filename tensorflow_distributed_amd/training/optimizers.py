"""Optimizers with TF1 ``tf.train`` semantics (reference: ``AdamOptimizer(lr)`` at
``/root/reference/mnist_single.py:95`` and ``mnist_python_m.py:208``; ``SyncReplicasOptimizer`` at
``mnist_python_m.py:210-233``).

Two layers:

* Plain config objects (``AdamOptimizer``, ``GradientDescentOptimizer``, ``MomentumOptimizer``)
  that model runners hand to their device implementation: the native GPU engine applies them with
  one fused flat HIP kernel (``csrc/kernels/optim.hip``); :class:`FlatApplier` below is the torch
  implementation used on CPU workers and by the parameter-server role (same update equations).
* :class:`SyncReplicasOptimizer` -- the distributed aggregation policy: average exactly
  ``replicas_to_aggregate`` gradients per global step out of ``total_num_replicas`` workers
  (``replicas_to_aggregate < total`` = backup workers). Executed by
  :mod:`tensorflow_distributed_amd.parallel.sync_replicas`.

TF ApplyAdam: ``lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)``; ``m = m + (g - m)(1 - b1)``;
``v = v + (g^2 - v)(1 - b2)``; ``p -= lr_t * m / (sqrt(v) + eps)``, ``t`` = update count (the
``beta1_power``/``beta2_power`` accumulators are ``b^t``). :func:`adam_update` and
:func:`momentum_update` are the fp64 definitions of ApplyAdam and ApplyMomentum / GradientDescent that the
flat kernels (``csrc/optim_kernels.h``) are held to element by element (``tests/flat_optim_oracle.py``).

Learning-rate schedules (``tf.train.exponential_decay`` / ``piecewise_constant`` /
``polynomial_decay`` / ``cosine_decay``, each with an optional linear warm-up): the ``learning_rate``
of every optimizer config is a float or one of the schedule dataclasses below. A schedule is a
function of ``global_step`` *before* the update (Adam's ``t - 1``), which is what TF's graph reads.
:func:`lr_at` is the fp64 definition; the GPU kernels evaluate the same formulas in fp32 from the
device step counter (``csrc/lr_schedule.h``), so a captured step graph follows the schedule.

Global-norm gradient clipping (``tf.clip_by_global_norm`` between ``compute_gradients`` and
``apply_gradients``): ``clip_norm`` on every optimizer config. :func:`clip_by_global_norm` is the fp64
definition; the GPU engine takes the norm and the factor on the device inside the step graph
(``csrc/kernels/grad_norm.hip``, ``optim_clip.hip``).

Moving average of the weights (``tf.train.ExponentialMovingAverage``, the ``variable_averages`` of
``SyncReplicasOptimizer``): ``ema_decay`` / ``ema_num_updates`` on every optimizer config. After each
update ``e' = e - (1 - d_t)(e - p')`` with ``d_t = decay`` or, with ``num_updates``,
``min(decay, (1 + t)/(10 + t))``, ``t`` = ``global_step`` after the update; no zero-debias, the shadow
starts as a copy of the parameters. :func:`ema_decay_at` / :func:`ema_update` are the fp64 definition;
the GPU optimizer kernels update the shadow themselves from ``p'`` in registers (``csrc/ema.h``,
``optim_ema.hip``, ``mnist_tail_ema.hip``).

Layer-wise optimizers (``tf.contrib.opt.LARSOptimizer``; LAMB, You et al. / tensorflow_addons):
:class:`LAMBOptimizer` and :class:`LARSOptimizer` scale every variable's update by a trust ratio formed
from two L2 norms over that variable, and carry a weight decay. A variable has two flags, ``LW_DECAY``
(the decay applies) and ``LW_ADAPT`` (the ratio applies); without them it uses ``lambda = 0`` and
``r = 1``. :func:`trust_ratio`, :func:`lamb_update` and :func:`lars_update` are the fp64 definitions;
the GPU forms the norms and the ratios on the device inside the step (``csrc/layerwise.h``,
``csrc/kernels/optim_layerwise.hip``). ``t`` is ``global_step`` after the update; no beta powers exist.

RMSProp and Adagrad (``tf.train.RMSPropOptimizer``, ``tf.train.AdagradOptimizer``): :class:`RMSPropOptimizer`
(plain or centered, with or without momentum) and :class:`AdagradOptimizer`. :func:`rmsprop_update` and
:func:`adagrad_update` are the fp64 definitions; slots start at TF's initial values (``ms = 1``,
``mom = mg = 0``, ``accum = initial_accumulator_value``). The GPU applies them with one flat kernel each
(``csrc/optim_rules.h``, ``csrc/kernels/optim_rules.hip``) inside the step, under the same schedules, clip,
moving average, accumulation and guard as every other rule.

Non-finite guard (the ``is_finite`` gate of TF's ``LossScaleOptimizer`` around ``apply_gradients``, the
``if not np.isfinite(loss): skip`` idiom): ``skip_nonfinite`` on every optimizer config, off by default.
A step whose aggregated gradient is not finite is an identity update -- parameters, slots and the EMA
shadow keep their bits -- that still consumes its batch and its ``t``. :func:`nonfinite_guard` is the
fp64 definition; the GPU engine decides on the device inside the step graph and counts the skipped steps
there (``csrc/kernels/grad_guard.hip``, ``optim_guard.hip``). The count is a statistic: nothing depends
on it and it is not checkpointed.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple, Union

import torch

MAX_BOUNDARIES = 4  # csrc/lr_schedule.h: kLrMaxBoundaries


def _check_common(decay_steps, warmup_steps) -> None:
    if int(decay_steps) != decay_steps or decay_steps < 1:
        raise ValueError(f"decay_steps must be an integer >= 1, got {decay_steps!r}")
    if int(warmup_steps) != warmup_steps or warmup_steps < 0:
        raise ValueError(f"warmup_steps must be an integer >= 0, got {warmup_steps!r}")


@dataclass(frozen=True)
class ExponentialDecay:
    """``lr * rate ** (s / decay_steps)``; ``staircase``: the integer quotient ``s // decay_steps``."""
    learning_rate: float
    decay_steps: int
    decay_rate: float
    staircase: bool = False
    warmup_steps: int = 0
    kind = "exponential"

    def __post_init__(self):
        _check_common(self.decay_steps, self.warmup_steps)


@dataclass(frozen=True)
class PiecewiseConstant:
    """``values[i]`` for the first ``i`` with ``s <= boundaries[i]``, else ``values[-1]`` (TF's
    inclusive convention). At most 4 boundaries; values are absolute rates."""
    boundaries: Tuple[int, ...]
    values: Tuple[float, ...]
    warmup_steps: int = 0
    kind = "piecewise"

    def __post_init__(self):
        b = tuple(self.boundaries)
        v = tuple(float(x) for x in self.values)
        if any(int(x) != x for x in b):
            raise ValueError(f"boundaries must be integer steps, got {b!r}")
        b = tuple(int(x) for x in b)
        if len(b) > MAX_BOUNDARIES:
            raise ValueError(f"at most {MAX_BOUNDARIES} boundaries, got {len(b)}")
        if len(v) != len(b) + 1:
            raise ValueError(f"len(values) must be len(boundaries) + 1, got {len(v)} values for {len(b)} boundaries")
        if any(b[i] <= b[i - 1] for i in range(1, len(b))):
            raise ValueError(f"boundaries must be strictly increasing, got {b!r}")
        _check_common(1, self.warmup_steps)
        object.__setattr__(self, "boundaries", b)
        object.__setattr__(self, "values", v)

    @property
    def learning_rate(self) -> float:
        return self.values[0]


@dataclass(frozen=True)
class PolynomialDecay:
    """``(lr - end) * (1 - min(s, decay_steps) / decay_steps) ** power + end``."""
    learning_rate: float
    decay_steps: int
    end_learning_rate: float = 0.0001
    power: float = 1.0
    warmup_steps: int = 0
    kind = "polynomial"

    def __post_init__(self):
        _check_common(self.decay_steps, self.warmup_steps)


@dataclass(frozen=True)
class CosineDecay:
    """``lr * ((1 - alpha) * 0.5 * (1 + cos(pi * min(s, decay_steps) / decay_steps)) + alpha)``."""
    learning_rate: float
    decay_steps: int
    alpha: float = 0.0
    warmup_steps: int = 0
    kind = "cosine"

    def __post_init__(self):
        _check_common(self.decay_steps, self.warmup_steps)


@dataclass(frozen=True)
class ConstantWarmup:
    """A constant rate behind a linear warm-up (``--lr_schedule=constant --lr_warmup_steps=w``)."""
    learning_rate: float
    warmup_steps: int
    kind = "constant"

    def __post_init__(self):
        _check_common(1, self.warmup_steps)


SCHEDULES = (ExponentialDecay, PiecewiseConstant, PolynomialDecay, CosineDecay, ConstantWarmup)
LearningRate = Union[float, ExponentialDecay, PiecewiseConstant, PolynomialDecay, CosineDecay, ConstantWarmup]


def is_schedule(lr) -> bool:
    return isinstance(lr, SCHEDULES)


def lr_at(lr: LearningRate, step: int) -> float:
    """The learning rate of the update that starts from ``global_step == step`` (fp64)."""
    if not is_schedule(lr):
        return float(lr)
    s = int(step)
    if isinstance(lr, PiecewiseConstant):
        out = lr.values[-1]
        for b, v in zip(lr.boundaries, lr.values):
            if s <= b:
                out = v
                break
    elif isinstance(lr, ExponentialDecay):
        e = (s // lr.decay_steps) if lr.staircase else s / lr.decay_steps
        out = lr.learning_rate * lr.decay_rate ** e
    elif isinstance(lr, PolynomialDecay):
        f = min(s, lr.decay_steps) / lr.decay_steps
        out = (lr.learning_rate - lr.end_learning_rate) * (1.0 - f) ** lr.power + lr.end_learning_rate
    elif isinstance(lr, CosineDecay):
        f = min(s, lr.decay_steps) / lr.decay_steps
        out = lr.learning_rate * ((1.0 - lr.alpha) * 0.5 * (1.0 + math.cos(math.pi * f)) + lr.alpha)
    else:
        out = lr.learning_rate
    if s < lr.warmup_steps:
        out *= (s + 1) / lr.warmup_steps
    return float(out)


def schedule_args(lr: LearningRate):
    """``(kind, params, boundaries, values)`` as the native ``set_lr_schedule`` / flat ops take them:
    params = [lr, decay_steps, rate, end, power, alpha, warmup_steps, staircase]."""
    if not is_schedule(lr):
        return "constant", [float(lr)], [], []
    p = [float(lr.learning_rate), float(getattr(lr, "decay_steps", 1)), float(getattr(lr, "decay_rate", 1.0)),
         float(getattr(lr, "end_learning_rate", 0.0)), float(getattr(lr, "power", 1.0)), float(getattr(lr, "alpha", 0.0)),
         float(lr.warmup_steps), float(bool(getattr(lr, "staircase", False)))]
    if isinstance(lr, PiecewiseConstant):
        return lr.kind, p, list(lr.boundaries), list(lr.values)
    return lr.kind, p, [], []


def _check_ema(decay) -> None:
    if decay is not None and not 0.0 < float(decay) < 1.0:
        raise ValueError(f"ema decay must be in (0, 1), got {decay!r}")


def ema_decay_at(decay: float, t: int, num_updates: bool = False) -> float:
    """``d_t`` of the update that ends at ``global_step == t`` (Adam's ``t``), fp64: ``decay``, or with
    ``num_updates`` (TF's ``num_updates=global_step``) ``min(decay, (1 + t) / (10 + t))``."""
    d = float(decay)
    if not 0.0 < d < 1.0:
        raise ValueError(f"ema decay must be in (0, 1), got {decay!r}")
    if not num_updates:
        return d
    return min(d, (1.0 + int(t)) / (10.0 + int(t)))


def ema_update(e: torch.Tensor, p: torch.Tensor, decay: float, t: int, num_updates: bool = False) -> torch.Tensor:
    """The shadow after the update that produced ``p`` and ended at ``global_step == t``, in fp64:
    ``e - (1 - d_t) * (e - p)``."""
    e64 = e.detach().to(torch.float64)
    return e64 - (1.0 - ema_decay_at(decay, t, num_updates)) * (e64 - p.detach().to(torch.float64))


@dataclass(frozen=True)
class ExponentialMovingAverage:
    """``tf.train.ExponentialMovingAverage(decay, num_updates=global_step)`` as a value: what
    ``SyncReplicasOptimizer(variable_averages=...)`` takes. ``num_updates``: whether the decay follows
    ``global_step`` (``min(decay, (1 + t)/(10 + t))``)."""
    decay: float
    num_updates: bool = False

    def __post_init__(self):
        if not 0.0 < float(self.decay) < 1.0:
            raise ValueError(f"ema decay must be in (0, 1), got {self.decay!r}")


@dataclass
class AdamOptimizer:
    learning_rate: LearningRate = 0.001
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: float = 1e-8
    name: str = "Adam"
    kind: str = field(default="adam", init=False)
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)


@dataclass
class GradientDescentOptimizer:
    learning_rate: LearningRate = 0.01
    name: str = "GradientDescent"
    kind: str = field(default="sgd", init=False)
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)


@dataclass
class MomentumOptimizer:
    learning_rate: LearningRate = 0.01
    momentum: float = 0.9
    use_nesterov: bool = False
    name: str = "Momentum"
    kind: str = field(default="momentum", init=False)
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)


@dataclass
class RMSPropOptimizer:
    """``ms' = ms + (g g - ms)(1 - decay)``; centered: ``mg' = mg + (g - mg)(1 - decay)``;
    ``mom' = momentum mom + lr g / sqrt(ms' [- mg' mg'] + epsilon)``; ``p' = p - mom'`` (TF1 ApplyRMSProp /
    ApplyCenteredRMSProp). Slots start as ``ms = 1``, ``mom = 0``, ``mg = 0``. The denominator is not
    clamped: a centered ``ms' - mg'^2`` that rounding drives below ``-epsilon`` gives NaN, exactly as in TF."""
    learning_rate: LearningRate = 0.001
    decay: float = 0.9
    momentum: float = 0.0
    epsilon: float = 1e-10
    centered: bool = False
    name: str = "RMSProp"
    kind: str = field(default="rmsprop", init=False)
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)
        if not 0.0 <= self.decay < 1.0 or self.momentum < 0 or self.epsilon < 0:
            raise ValueError("RMSProp: decay in [0, 1), momentum >= 0, epsilon >= 0")


@dataclass
class AdagradOptimizer:
    """``accum' = accum + g g``; ``p' = p - lr g / sqrt(accum')`` (TF1 ApplyAdagrad). The slot starts at
    ``initial_accumulator_value`` (> 0); there is no epsilon."""
    learning_rate: LearningRate = 0.01
    initial_accumulator_value: float = 0.1
    name: str = "Adagrad"
    kind: str = field(default="adagrad", init=False)
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)
        if not self.initial_accumulator_value > 0:
            raise ValueError(f"initial_accumulator_value must be > 0, got {self.initial_accumulator_value!r}")


def rmsprop_update(p, ms, mom, g, lr: float, decay: float, momentum: float, epsilon: float, mg=None):
    """One RMSProp update in fp64: ``(p', ms', mom')``, or ``(p', ms', mom', mg')`` when ``mg`` is given (the
    centered rule). ``g`` is the gradient the optimizer consumes (scale and clip factor applied), ``lr`` the
    rate of this update. No clamp on the denominator (see :class:`RMSPropOptimizer`)."""
    f = lambda x: torch.as_tensor(x).detach().to(torch.float64)  # noqa: E731
    p, ms, mom, g = f(p), f(ms), f(mom), f(g)
    ms2 = ms + (g * g - ms) * (1.0 - decay)
    if mg is None:
        d = ms2 + epsilon
    else:
        mg2 = f(mg) + (g - f(mg)) * (1.0 - decay)
        d = ms2 - mg2 * mg2 + epsilon
    mom2 = momentum * mom + lr * g / d.sqrt()
    if mg is None:
        return p - mom2, ms2, mom2
    return p - mom2, ms2, mom2, mg2


def adagrad_update(p, accum, g, lr: float):
    """One Adagrad update in fp64: ``(p', accum')``."""
    f = lambda x: torch.as_tensor(x).detach().to(torch.float64)  # noqa: E731
    p, accum, g = f(p), f(accum), f(g)
    a2 = accum + g * g
    return p - lr * g / a2.sqrt(), a2


def adam_update(p, m, v, g, t: int, lr: float, beta1: float, beta2: float, epsilon: float):
    """One Adam update in fp64 (TF1 ApplyAdam, as ``csrc/kernels/optim.hip`` states it): ``(p', m', v')``.
    ``g`` is the gradient the optimizer consumes (scale and clip factor applied), ``t`` the update's count
    (``global_step`` after it), ``lr`` the rate of this update; epsilon is outside the root."""
    f = lambda x: torch.as_tensor(x).detach().to(torch.float64)  # noqa: E731
    p, m, v, g = f(p), f(m), f(v), f(g)
    m2 = m + (g - m) * (1.0 - beta1)
    v2 = v + (g * g - v) * (1.0 - beta2)
    lr_t = lr * math.sqrt(1.0 - beta2 ** int(t)) / (1.0 - beta1 ** int(t))
    return p - lr_t * m2 / (v2.sqrt() + epsilon), m2, v2


def momentum_update(p, accum, g, lr: float, momentum: float, weight_decay: float = 0.0, nesterov: bool = False):
    """One Momentum update in fp64 (TF1 ApplyMomentum): ``(p', accum')`` with ``accum' = momentum accum + g`` and
    ``p' = p - lr accum'``, Nesterov ``p' = p - lr (g + momentum accum')``. ``accum=None`` is plain gradient
    descent, ``(p - lr g, None)``. The L2 weight decay is folded into the gradient: ``g + weight_decay p``."""
    f = lambda x: torch.as_tensor(x).detach().to(torch.float64)  # noqa: E731
    p, g = f(p), f(g)
    g = g + weight_decay * p
    if accum is None:
        return p - lr * g, None
    a2 = momentum * f(accum) + g
    return p - lr * ((g + momentum * a2) if nesterov else a2), a2


LW_DECAY, LW_ADAPT = 1, 2  # csrc/layerwise.h: LwFlags


@dataclass
class LAMBOptimizer:
    """``u = c_t m' / (sqrt(v') + eps) + lambda p``; ``p' = p - lr r u``, ``r = |p| / |u|`` per variable.
    With ``weight_decay`` and no variable adapted this is AdamW."""
    learning_rate: LearningRate = 0.001
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: float = 1e-6
    weight_decay: float = 0.0
    skip_bias: bool = True
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped
    name: str = "LAMB"
    kind: str = field(default="lamb", init=False)

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)
        if self.weight_decay < 0:
            raise ValueError(f"weight_decay must be >= 0, got {self.weight_decay!r}")


@dataclass
class LARSOptimizer:
    """``accum' = mu accum + lr r (g + lambda p)``; ``p' = p - accum'``,
    ``r = eeta |p| / (|g| + lambda |p| + eps)`` per variable (TF1 contrib: the rate is folded into the
    accumulator). No Nesterov form."""
    learning_rate: LearningRate = 0.01
    momentum: float = 0.9
    weight_decay: float = 1e-4
    eeta: float = 1e-3
    epsilon: float = 0.0
    skip_bias: bool = True
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_num_updates: bool = False
    accum_steps: int = 1  # micro-batches summed per update (gradient accumulation); 1 = off
    skip_nonfinite: bool = False  # non-finite guard: a step whose aggregated gradient is not finite is skipped
    name: str = "LARS"
    kind: str = field(default="lars", init=False)

    def __post_init__(self):
        _check_ema(self.ema_decay)
        _check_accum(self.accum_steps)
        if self.weight_decay < 0 or not self.eeta > 0 or self.epsilon < 0:
            raise ValueError("LARS: weight_decay >= 0, eeta > 0, epsilon >= 0")


LAYERWISE_KINDS = ("lamb", "lars")


def is_layerwise(opt) -> bool:
    return getattr(base_optimizer(opt), "kind", None) in LAYERWISE_KINDS


def trust_ratio(p_norm: float, x_norm: float, adapt: bool = True, eeta: Optional[float] = None,
                weight_decay: float = 0.0, epsilon: float = 0.0) -> float:
    """The trust ratio of one variable, fp64. LAMB (``eeta`` None): ``|p| / |u|`` with ``x_norm = |u|``.
    LARS: ``eeta |p| / (|g| + lambda |p| + eps)`` with ``x_norm = |g|`` and ``weight_decay`` the
    variable's effective ``lambda``. 1 for a variable that is not adapted or when either norm is 0."""
    pn, xn = float(p_norm), float(x_norm)
    if not (adapt and pn > 0.0 and xn > 0.0):
        return 1.0
    if eeta is None:
        return pn / xn
    return float(eeta) * pn / (xn + float(weight_decay) * pn + float(epsilon))


def _norm64(x: torch.Tensor) -> float:
    return math.sqrt(float(x.pow(2).sum().item()))


def lamb_update(p, m, v, g, t: int, lr: float, beta1: float, beta2: float, epsilon: float, weight_decay: float = 0.0,
                decay: bool = True, adapt: bool = True):
    """One LAMB update of ONE variable in fp64: ``(p', m', v', (|p|, |u|, r))``. ``g`` is the gradient
    the optimizer consumes (scale and clip factor applied), ``t`` the update's count (``global_step``
    after it), ``lr`` the rate of this update."""
    f = lambda x: x.detach().to(torch.float64)  # noqa: E731
    p, m, v, g = f(p), f(m), f(v), f(g)
    m2 = m + (g - m) * (1.0 - beta1)
    v2 = v + (g * g - v) * (1.0 - beta2)
    ct = math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    u = ct * m2 / (v2.sqrt() + epsilon) + (float(weight_decay) if decay else 0.0) * p
    pn, un = _norm64(p), _norm64(u)
    r = trust_ratio(pn, un, adapt)
    return p - lr * r * u, m2, v2, (pn, un, r)


def lars_update(p, accum, g, lr: float, momentum: float, weight_decay: float, eeta: float, epsilon: float = 0.0,
                decay: bool = True, adapt: bool = True):
    """One LARS update of ONE variable in fp64: ``(p', accum', (|p|, |g|, r))``."""
    f = lambda x: x.detach().to(torch.float64)  # noqa: E731
    p, accum, g = f(p), f(accum), f(g)
    lam = float(weight_decay) if decay else 0.0
    pn, gn = _norm64(p), _norm64(g)
    r = trust_ratio(pn, gn, adapt, eeta, lam, epsilon)
    a2 = momentum * accum + lr * r * (g + lam * p)
    return p - a2, a2, (pn, gn, r)


@dataclass
class SyncReplicasOptimizer:
    """``tf.train.SyncReplicasOptimizer(opt, replicas_to_aggregate, total_num_replicas)``."""
    opt: object
    replicas_to_aggregate: Optional[int] = None
    total_num_replicas: Optional[int] = None
    name: str = "sync_replicas"
    # TF's variable_averages (variables_to_average: every trainable variable): forwarded to the base
    # optimizer's ema_decay / ema_num_updates, so the shadow is updated after every aggregated update
    variable_averages: Optional[ExponentialMovingAverage] = None
    # the non-finite guard of the aggregated update: forwarded to the base optimizer's skip_nonfinite
    # (None: whatever the base optimizer says)
    skip_nonfinite: Optional[bool] = None

    def __post_init__(self):
        import dataclasses

        va = self.variable_averages
        if va is not None:
            self.opt = dataclasses.replace(self.opt, ema_decay=float(va.decay), ema_num_updates=bool(va.num_updates))
        if self.skip_nonfinite is not None:
            self.opt = dataclasses.replace(self.opt, skip_nonfinite=bool(self.skip_nonfinite))

    def resolve(self, num_workers: int) -> "SyncReplicasOptimizer":
        r = self.replicas_to_aggregate if self.replicas_to_aggregate is not None else num_workers
        t = self.total_num_replicas if self.total_num_replicas is not None else num_workers
        if not 1 <= r <= t:
            raise ValueError(f"replicas_to_aggregate={r} must be in [1, total_num_replicas={t}]")
        return SyncReplicasOptimizer(self.opt, r, t, self.name, self.variable_averages, self.skip_nonfinite)

    @property
    def has_backup_workers(self) -> bool:
        return self.replicas_to_aggregate is not None and self.total_num_replicas is not None and \
            self.replicas_to_aggregate < self.total_num_replicas


def _check_accum(k) -> None:
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"accum_steps must be an integer >= 1, got {k!r}")


def accumulate_gradients(grads: Sequence[torch.Tensor]) -> torch.Tensor:
    """Gradient accumulation's definition in fp64: the micro-batch gradients summed one after another in
    the order given, unscaled (the optimizer takes the sum at scale ``1 / (K * world)``). The device does
    the same sum in fp32 (``csrc/kernels/grad_accum.hip``)."""
    if len(grads) < 1:
        raise ValueError("accumulate_gradients: at least one gradient")
    acc = grads[0].detach().to(torch.float64).clone()
    for g in grads[1:]:
        if g.shape != acc.shape:
            raise ValueError("accumulate_gradients: gradients of one shape")
        acc += g.detach().to(torch.float64)
    return acc


def clip_by_global_norm(g: torch.Tensor, clip_norm: float, scale: float = 1.0) -> Tuple[float, float]:
    """``(factor, norm)`` of ``tf.clip_by_global_norm`` over the flat gradient ``g``, in fp64.

    ``norm = scale * sqrt(sum g_i^2)`` is the norm of the gradient the optimizer consumes (``scale`` is
    the 1/N of a sum-all-reduce); the optimizer's gradient is ``g * factor`` with
    ``factor = scale * clip_norm / max(norm, clip_norm)``. The clip part is *exactly* 1.0 whenever
    ``norm <= clip_norm`` (TF's ``clip_norm * min(1/norm, 1/clip_norm)`` equals it up to rounding), so
    an inactive clip changes no bit. Non-finite norms get no special handling: an ``inf`` norm gives
    factor 0; a NaN norm fails the comparison, leaves the clip part at 1, and the NaN gradient
    elements propagate as they do without clipping. The device kernels do the same in fp32.
    """
    c = float(clip_norm)
    if not c > 0:
        raise ValueError(f"clip_norm must be > 0, got {clip_norm!r}")
    norm = float(scale) * math.sqrt(float(g.detach().to(torch.float64).pow(2).sum().item()))
    return float(scale) * (c / (norm if norm > c else c)), norm


FLT_MAX = 3.4028234663852886e38  # the largest finite fp32


def nonfinite_guard(g: torch.Tensor, scale: float = 1.0) -> Tuple[float, bool]:
    """``(norm, ok)`` of the non-finite guard over the flat gradient ``g``, in fp64.

    ``norm = scale * sqrt(sum g_i^2)`` as :func:`clip_by_global_norm` takes it. ``ok`` is False when the
    step is to be skipped: the sum of squares or the scaled norm is ``inf``, NaN or beyond the fp32 range.
    That covers every ``inf`` / NaN element, and also finite gradients whose norm overflows fp32 -- the
    device sums the squares in fp32 (``grad_sumsq``), so for it such a norm *is* ``inf``, and those
    steps are skipped as well: a gradient whose norm fp32 cannot hold has no usable clip factor or
    trust ratio either.
    """
    sumsq = float(g.detach().to(torch.float64).pow(2).sum().item())
    norm = float(scale) * math.sqrt(sumsq) if sumsq >= 0.0 else float("nan")  # NaN fails the compare
    ok = math.isfinite(sumsq) and sumsq <= FLT_MAX and math.isfinite(norm) and norm <= FLT_MAX
    return norm, ok


def check_segments(segments, numel: int):
    """The variable table as ``[(begin, length, flags)]`` of ints, checked as ``csrc/layerwise.h`` checks
    it: sorted, disjoint, every begin a multiple of 4, any length >= 1, inside ``numel``; gaps allowed."""
    out, end = [], 0
    for i, (beg, n, flags) in enumerate(segments):
        beg, n, flags = int(beg), int(n), int(flags)
        if n < 1:
            raise ValueError(f"segment {i} is empty (length >= 1)")
        if beg < 0 or beg % 4:
            raise ValueError(f"segment {i} does not begin on a multiple of 4")
        if beg < end:
            raise ValueError(f"segment {i} overlaps or precedes its predecessor (sorted, disjoint)")
        if beg + n > numel:
            raise ValueError(f"segment {i} ends outside the buffer")
        if flags & ~(LW_DECAY | LW_ADAPT):
            raise ValueError(f"segment {i} has unknown flags")
        end = beg + n
        out.append((beg, n, flags))
    if not out:
        raise ValueError("at least one segment")
    return out


def base_optimizer(opt):
    return opt.opt if isinstance(opt, SyncReplicasOptimizer) else opt


class FlatApplier:
    """Applies an optimizer config to a flat fp32 parameter tensor (any device) with TF semantics.

    Slot tensors (``m``/``v`` for Adam, ``accum`` for momentum) are flat buffers of the same size;
    ``t`` counts applied updates (for the parameter server it is the number of updates applied to
    this shard, exactly like TF's per-PS ``beta1_power``).
    """

    def __init__(self, opt, numel: int, device=None, segments=None):
        self.opt = base_optimizer(opt)
        self.device = device
        self.t = 0
        k = self.opt.kind
        z = lambda: torch.zeros(numel, dtype=torch.float32, device=device)  # noqa: E731
        self.m = z() if k in ("adam", "momentum", "lamb", "lars") else None
        self.v = z() if k in ("adam", "lamb") else None
        # RMSProp: ms, mom and (centered) mg; Adagrad: accum -- at TF's initial values (reset_slots)
        self.ms = z() if k == "rmsprop" else None
        self.mom = z() if k == "rmsprop" else None
        self.mg = z() if k == "rmsprop" and self.opt.centered else None
        self.accum = z() if k == "adagrad" else None
        self.reset_slots()
        # layer-wise optimizers: the variable table [(begin, length, flags)] (models.mnist_cnn.segments)
        # and, after every apply(), [(|p|, |u| or |g|, r)] per variable
        self.segments = None
        self.last_layer_norms = None
        if k in LAYERWISE_KINDS:
            if segments is None:
                raise ValueError(f"{self.opt.name}: a layer-wise optimizer needs the variable table (segments=...)")
            self.segments = check_segments(segments, numel)
        self.last_grad_norm: Optional[float] = None  # norm / clip part of the last clipped apply()
        self.last_clip_scale: Optional[float] = None
        # moving average of the weights (ema_decay on the config): starts as a copy of the parameters at
        # the first apply(), or where reset_ema() / load_ema() put it
        self.ema: Optional[torch.Tensor] = None
        # non-finite guard (skip_nonfinite on the config): applies skipped so far (a statistic, not
        # checkpointed) and whether the last apply() was applied
        self.skipped_steps = 0
        self.last_step_ok = True

    @torch.no_grad()
    def apply(self, p: torch.Tensor, g: torch.Tensor, scale: float = 1.0) -> None:
        o = self.opt
        if getattr(o, "skip_nonfinite", False):
            self.last_grad_norm, self.last_step_ok = nonfinite_guard(g, scale)
            if not self.last_step_ok:
                # an identity update that consumes its t: p, the slots and the shadow keep their bits
                if getattr(o, "ema_decay", None) and self.ema is None:
                    self.reset_ema(p)
                self.last_clip_scale = 0.0
                self.skipped_steps += 1
                self.t += 1
                return
        if getattr(o, "clip_norm", None):
            factor, self.last_grad_norm = clip_by_global_norm(g, o.clip_norm, scale)
            self.last_clip_scale = factor / scale
            scale = factor
        g = g if scale == 1.0 else g * scale
        if getattr(o, "ema_decay", None) and self.ema is None:
            self.reset_ema(p)
        lr = lr_at(o.learning_rate, self.t)  # global_step before this update
        self.t += 1
        if o.kind == "adam":
            b1, b2 = o.beta1, o.beta2
            lr_t = lr * (1 - b2 ** self.t) ** 0.5 / (1 - b1 ** self.t)
            self.m.add_(g - self.m, alpha=1 - b1)
            self.v.add_(g * g - self.v, alpha=1 - b2)
            p.sub_(lr_t * self.m / (self.v.sqrt() + o.epsilon))
        elif o.kind in LAYERWISE_KINDS:
            self._apply_layerwise(p, g, lr)
        elif o.kind == "rmsprop":
            # the fp64 definition; parameters and slots are stored in fp32
            out = rmsprop_update(p, self.ms, self.mom, g, lr, o.decay, o.momentum, o.epsilon, self.mg)
            p.copy_(out[0].to(torch.float32))
            self.ms.copy_(out[1].to(torch.float32))
            self.mom.copy_(out[2].to(torch.float32))
            if self.mg is not None:
                self.mg.copy_(out[3].to(torch.float32))
        elif o.kind == "adagrad":
            p2, a2 = adagrad_update(p, self.accum, g, lr)
            p.copy_(p2.to(torch.float32))
            self.accum.copy_(a2.to(torch.float32))
        elif o.kind == "momentum":
            self.m.mul_(o.momentum).add_(g)
            if o.use_nesterov:
                p.sub_(lr * (g + o.momentum * self.m))
            else:
                p.sub_(lr * self.m)
        else:
            p.sub_(lr * g)
        if getattr(o, "ema_decay", None):
            # the update itself ran with EMA off or on alike; the shadow follows p' in fp32
            omd = 1.0 - ema_decay_at(o.ema_decay, self.t, o.ema_num_updates)
            self.ema.add_(p - self.ema, alpha=omd)

    def _apply_layerwise(self, p: torch.Tensor, g: torch.Tensor, lr: float) -> None:
        """Per variable, the fp64 definition; parameters and slots are stored in fp32. Elements that
        belong to no variable are untouched."""
        o = self.opt
        norms = []
        for beg, n, flags in self.segments:
            sl = slice(beg, beg + n)
            decay, adapt = bool(flags & LW_DECAY), bool(flags & LW_ADAPT)
            if o.kind == "lamb":
                p2, m2, v2, nr = lamb_update(p[sl], self.m[sl], self.v[sl], g[sl], self.t, lr, o.beta1, o.beta2, o.epsilon,
                                             o.weight_decay, decay, adapt)
                self.v[sl] = v2.to(torch.float32)
            else:
                p2, m2, nr = lars_update(p[sl], self.m[sl], g[sl], lr, o.momentum, o.weight_decay, o.eeta, o.epsilon,
                                         decay, adapt)
            self.m[sl] = m2.to(torch.float32)
            p[sl] = p2.to(torch.float32)
            norms.append(nr)
        self.last_layer_norms = norms

    def reset_ema(self, p: torch.Tensor) -> None:
        """(Re)start the average as a copy of ``p`` (no zero-debias)."""
        if getattr(self.opt, "ema_decay", None):
            self.ema = p.detach().clone()

    def load_ema(self, e: torch.Tensor) -> None:
        if getattr(self.opt, "ema_decay", None):
            self.ema = e.detach().to(torch.float32).clone()

    def reset_slots(self) -> None:
        """Every slot at its initial value: 0, but TF's ``ms = 1`` for RMSProp and
        ``initial_accumulator_value`` for Adagrad."""
        for name, s in self.slots().items():
            s.fill_(1.0 if name == "ms" else self.opt.initial_accumulator_value if name == "accum" else 0.0)

    def slots(self) -> "OrderedDict[str, torch.Tensor]":
        """In a fixed order: ``m``, ``v``; RMSProp ``ms``, ``mg`` (centered), ``mom``; Adagrad ``accum``."""
        out = OrderedDict()
        for name in ("m", "v", "ms", "mg", "mom", "accum"):
            if getattr(self, name) is not None:
                out[name] = getattr(self, name)
        return out

    def powers(self):
        o = self.opt
        if o.kind != "adam":
            return {}
        return {"beta1_power": o.beta1 ** self.t, "beta2_power": o.beta2 ** self.t}
