"""Learning-rate schedules, host side: the fp64 ``lr_at`` against literal values, construction-time
validation, ``FlatApplier`` under a schedule, checkpoint resume, the ``--lr_*`` flags and the
Supervisor's ``learning_rate`` scalar. (The device evaluation: tests/test_lr_schedule_gpu.py.)"""
import math

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import lr_at


# ---------------------------------------------------------------- lr_at against literal values
def test_exponential_values():
    sc = O.ExponentialDecay(0.1, 100, 0.96)
    assert lr_at(sc, 0) == pytest.approx(0.1, rel=1e-15)
    assert lr_at(sc, 250) == pytest.approx(0.1 * 0.96 ** 2.5, rel=1e-15)
    st = O.ExponentialDecay(0.1, 100, 0.96, staircase=True)
    assert lr_at(st, 250) == pytest.approx(0.09216, rel=1e-12)
    assert lr_at(st, 200) == lr_at(st, 299) and lr_at(st, 299) != lr_at(st, 300)


def test_piecewise_values_inclusive_boundaries():
    sc = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])
    assert [lr_at(sc, s) for s in (0, 2, 3, 5, 6)] == [1e-2, 1e-2, 1e-3, 1e-3, 1e-4]
    assert lr_at(O.PiecewiseConstant([], [0.5]), 10 ** 6) == 0.5


def test_polynomial_values():
    d = 200
    sc = O.PolynomialDecay(0.1, d, end_learning_rate=0.001, power=2.0)
    assert lr_at(sc, 0) == pytest.approx(0.1, rel=1e-15)
    assert lr_at(sc, d // 2) == pytest.approx((0.1 - 0.001) * 0.25 + 0.001, rel=1e-15)
    assert lr_at(sc, d) == pytest.approx(0.001, rel=1e-15)
    assert lr_at(sc, d + 7) == lr_at(sc, d)


def test_cosine_values():
    d = 200
    sc = O.CosineDecay(0.1, d, alpha=0.01)
    assert lr_at(sc, 0) == pytest.approx(0.1, rel=1e-15)
    assert lr_at(sc, d // 2) == pytest.approx(0.1 * (0.99 * 0.5 + 0.01), rel=1e-14)
    assert lr_at(sc, d) == pytest.approx(0.1 * 0.01, rel=1e-12)
    assert lr_at(sc, d + 7) == lr_at(sc, d)


def test_warmup_values():
    for sc, base in ((O.ExponentialDecay(0.1, 100, 0.96, warmup_steps=4), lambda s: 0.1 * 0.96 ** (s / 100)),
                     (O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4], warmup_steps=4),
                      lambda s: 1e-2 if s <= 2 else 1e-3),
                     (O.ConstantWarmup(0.3, 4), lambda s: 0.3)):
        assert lr_at(sc, 0) == pytest.approx(base(0) * 1 / 4, rel=1e-15)
        assert lr_at(sc, 3) == pytest.approx(base(3) * 4 / 4, rel=1e-15)
        assert lr_at(sc, 4) == pytest.approx(base(4), rel=1e-15)


def test_float_is_its_own_schedule():
    assert lr_at(0.01, 0) == 0.01 and lr_at(0.01, 10 ** 9) == 0.01
    assert O.schedule_args(0.01) == ("constant", [0.01], [], [])


# ---------------------------------------------------------------- validation at construction
@pytest.mark.parametrize("bounds,values", [
    ([5, 2], [1.0, 0.1, 0.01]),          # not increasing
    ([2, 2], [1.0, 0.1, 0.01]),          # not strictly increasing
    ([2, 5], [1.0, 0.1]),                # too few values
    ([2, 5], [1.0, 0.1, 0.01, 0.001]),   # too many values
    ([1, 2, 3, 4, 5], [1.0] * 6),        # more than 4 boundaries
    ([1.5], [1.0, 0.1]),                 # a boundary that is no step
])
def test_piecewise_validation(bounds, values):
    with pytest.raises(ValueError):
        O.PiecewiseConstant(bounds, values)


@pytest.mark.parametrize("make", [
    lambda: O.ExponentialDecay(0.1, 0, 0.96),
    lambda: O.PolynomialDecay(0.1, 0),
    lambda: O.CosineDecay(0.1, -3),
    lambda: O.CosineDecay(0.1, 10, warmup_steps=-1),
])
def test_decay_steps_validation(make):
    with pytest.raises(ValueError):
        make()


# ---------------------------------------------------------------- FlatApplier
@pytest.mark.parametrize("kind", ["adam", "momentum"])
def test_flat_applier_follows_schedule(kind):
    """6 steps under a piecewise schedule == a manual loop that swaps in a constant-lr optimizer with
    lr_at(s) before every step (bitwise)."""
    sc = O.PiecewiseConstant([2, 4], [1e-1, 1e-2, 1e-3])
    mk = (lambda lr: O.AdamOptimizer(lr)) if kind == "adam" else (lambda lr: O.MomentumOptimizer(lr, 0.9))
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(16, generator=g)
    grads = [torch.randn(16, generator=g) for _ in range(6)]
    pa, pb = p0.clone(), p0.clone()
    a = O.FlatApplier(mk(sc), 16)
    b = O.FlatApplier(mk(lr_at(sc, 0)), 16)
    seen = []
    for s, gr in enumerate(grads):
        a.apply(pa, gr)
        b.opt = mk(lr_at(sc, s))
        seen.append(b.opt.learning_rate)
        b.apply(pb, gr)
    assert seen == [1e-1, 1e-1, 1e-1, 1e-2, 1e-2, 1e-3]
    assert torch.equal(pa, pb) and torch.equal(a.m, b.m)
    if kind == "adam":
        assert torch.equal(a.v, b.v)
    c = O.FlatApplier(mk(1e-1), 16)
    pc = p0.clone()
    for gr in grads:
        c.apply(pc, gr)
    assert not torch.equal(pa, pc)


# ---------------------------------------------------------------- resume
def _run(runner, batches):
    for x, y in batches:
        runner.train_step(x, y)


def test_resume_continues_the_schedule():
    """3 steps, checkpoint, 2 more in a fresh runner == 5 uninterrupted steps (bitwise): the schedule
    is a function of the saved global_step, no extra checkpoint state."""
    from tensorflow_distributed_amd.models import mnist_cnn as M
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    sc = O.PiecewiseConstant([1, 3], [1e-2, 1e-3, 1e-4])
    g = torch.Generator().manual_seed(5)
    batches = [(torch.rand(8, 784, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(5)]
    init = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(0).items()})

    def fresh(lr):
        r = TorchMnistRunner(8, O.AdamOptimizer(lr), keep_prob=1.0)
        r.set_params(init)
        return r

    whole = fresh(sc)
    _run(whole, batches)
    first = fresh(sc)
    _run(first, batches[:3])
    ckpt = first.state_dict_tf()
    second = fresh(sc)
    second.load_state_dict_tf(ckpt)
    assert second.global_step() == 3 and second.current_lr() == 1e-3
    _run(second, batches[3:])
    assert second.global_step() == 5
    assert torch.equal(second.params(), whole.params())
    assert torch.equal(second.applier.m, whole.applier.m) and torch.equal(second.applier.v, whole.applier.v)
    const = fresh(1e-2)
    _run(const, batches)
    assert not torch.equal(const.params(), whole.params())


# ---------------------------------------------------------------- flags
def _optimizer_from(argv):
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog"] + argv)
        return dist_main._make_optimizer()
    finally:
        F.FLAGS.reset()


def test_flags_build_the_schedule():
    opt = _optimizer_from(["--lr_schedule=piecewise", "--lr_boundaries=2,5", "--lr_values=0.01,0.001,0.0001"])
    assert isinstance(opt, O.AdamOptimizer)
    assert opt.learning_rate == O.PiecewiseConstant((2, 5), (0.01, 0.001, 0.0001))
    opt = _optimizer_from(["--optimizer=momentum", "--learning_rate=0.1", "--lr_schedule=exponential",
                           "--lr_decay_steps=100", "--lr_decay_rate=0.96", "--lr_staircase", "--lr_warmup_steps=5"])
    assert opt == O.MomentumOptimizer(O.ExponentialDecay(0.1, 100, 0.96, True, 5), 0.9)
    opt = _optimizer_from(["--optimizer=sgd", "--lr_schedule=cosine", "--lr_decay_steps=50", "--lr_alpha=0.01"])
    assert opt == O.GradientDescentOptimizer(O.CosineDecay(0.01, 50, 0.01))
    opt = _optimizer_from(["--lr_schedule=polynomial", "--lr_decay_steps=50", "--lr_end=0.001", "--lr_power=2"])
    assert opt == O.AdamOptimizer(O.PolynomialDecay(0.01, 50, 0.001, 2.0))
    with pytest.raises(ValueError):
        _optimizer_from(["--lr_schedule=piecewise", "--lr_boundaries=5,2", "--lr_values=0.01,0.001,0.0001"])


def test_default_flags_give_todays_optimizer():
    opt = _optimizer_from([])
    assert opt == O.AdamOptimizer(0.01) and type(opt.learning_rate) is float
    assert _optimizer_from(["--optimizer=momentum"]) == O.MomentumOptimizer(0.01, 0.9)
    assert _optimizer_from(["--optimizer=sgd", "--learning_rate=0.5"]) == O.GradientDescentOptimizer(0.5)


# ---------------------------------------------------------------- reporting
def test_supervisor_writes_learning_rate(tmp_path):
    from tensorflow_distributed_amd.training import summary as S
    from tensorflow_distributed_amd.training.supervisor import Supervisor

    class Runner:
        opt = O.AdamOptimizer(O.ExponentialDecay(0.1, 100, 0.96))

        def global_step(self):
            return 0

    sv = Supervisor(True, str(tmp_path), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(250)
    sv.writer.close()
    got = {tag: v for step, tag, v in S.read_scalars(sv.writer.path) if step == 250}
    assert got["learning_rate"] == pytest.approx(0.1 * 0.96 ** 2.5, rel=1e-6)  # the event file stores fp32
    assert math.isfinite(got["global_step/sec"])


def test_native_arguments_of_a_schedule():
    kind, params, bounds, values = O.schedule_args(O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4], warmup_steps=3))
    assert kind == "piecewise" and bounds == [2, 5] and values == [1e-2, 1e-3, 1e-4] and params[6] == 3.0
    kind, params, bounds, values = O.schedule_args(O.ExponentialDecay(0.1, 100, 0.96, staircase=True))
    assert (kind, bounds, values) == ("exponential", [], [])
    assert params == [0.1, 100.0, 0.96, 0.0, 1.0, 0.0, 0.0, 1.0]
    assert np.isclose(params[0], 0.1)


# ---------------------------------------------------------------- ResNet
def test_resnet_runner_evaluates_the_schedule_at_the_step_before_the_update():
    from tensorflow_distributed_amd.models.resnet import ResNet, ResNetRunner

    sc = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])
    calls = []

    class Model:
        def train_step(self, x, labels, lr, global_step=0, **kw):
            calls.append(ResNet.lr_op_args(lr, 0.9, 1e-4, 1.0, global_step)[0])
            return 0.0

    r = ResNetRunner(Model())
    r.set_global_step(1)
    for _ in range(6):
        r.train_step(None, None, lr=sc)
    assert r.global_step() == 7
    assert calls == [lr_at(sc, s) for s in range(1, 7)] == [1e-2, 1e-2, 1e-3, 1e-3, 1e-3, 1e-4]
    assert ResNet.lr_op_args(0.1, 0.9, 1e-4, 0.5, 123) == (0.1, 0.9, 1e-4, False, 0.5)
    step = torch.zeros(1, dtype=torch.int64)  # the captured-graph form: the kernel reads the tensor
    got = ResNet.lr_op_args(sc, 0.9, 1e-4, 0.5, 123, step)
    assert got[0] == 1e-2 and got[5] is step and got[6] == 1 and got[7:] == O.schedule_args(sc)
    assert ResNet.lr_op_args(0.1, 0.9, 1e-4, 0.5, 123, step) == (0.1, 0.9, 1e-4, False, 0.5)
