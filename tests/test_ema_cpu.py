"""Exponential moving average of the weights (training/optimizers.py: ema_decay_at, ema_update,
ExponentialMovingAverage; FlatApplier / TorchMnistRunner keep the shadow in torch): the definition, the
torch runners against it, the checkpoint's <var>/ExponentialMovingAverage tensors and the flags."""
import dataclasses

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.models.mnist_runner import EMA_SUFFIX, TorchMnistRunner
from tensorflow_distributed_amd.training import optimizers as O

B = 4


# ---------------------------------------------------------------- the definition
def test_ema_decay_at():
    for t in (0, 1, 7, 10 ** 6):
        assert O.ema_decay_at(0.99, t) == 0.99  # constant mode
        assert O.ema_decay_at(0.99, t, False) == 0.99
    for t in range(1, 13):  # num_updates: (1 + t) / (10 + t) until it reaches the decay, at t = 8
        want = (1.0 + t) / (10.0 + t) if t < 8 else 0.5
        assert O.ema_decay_at(0.5, t, True) == want, t
    assert (1.0 + 8) / (10.0 + 8) == 0.5
    assert O.ema_decay_at(0.5, 7, True) < 0.5 == O.ema_decay_at(0.5, 8, True)
    assert O.ema_decay_at(0.9999, 10 ** 9, True) == 0.9999


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_bad_decays_raise(bad):
    with pytest.raises(ValueError, match="decay"):
        O.ema_decay_at(bad, 1)
    with pytest.raises(ValueError, match="decay"):
        O.ExponentialMovingAverage(bad)
    for cfg in (O.AdamOptimizer, O.MomentumOptimizer, O.GradientDescentOptimizer):
        with pytest.raises(ValueError, match="decay"):
            cfg(0.01, ema_decay=bad)
    assert O.AdamOptimizer(0.01).ema_decay is None and O.AdamOptimizer(0.01).ema_num_updates is False


def test_ema_update_by_hand():
    e, p = torch.tensor([8.0]), torch.tensor([0.0])
    for want in (4.0, 2.0, 1.0, 0.5):
        e = O.ema_update(e, p, 0.5, 1)
        assert e.dtype == torch.float64 and e.item() == want
    # num_updates: t = 1 gives d = 2 / 11
    assert O.ema_update(torch.tensor([1.0]), torch.tensor([0.0]), 0.5, 1, True).item() == pytest.approx(2.0 / 11.0, abs=1e-16)
    # e - (1 - d)(e - p): p = e stays put
    assert O.ema_update(torch.tensor([3.0]), torch.tensor([3.0]), 0.9, 5).item() == 3.0


# ---------------------------------------------------------------- FlatApplier
N = 1000


@pytest.mark.parametrize("opt", [O.AdamOptimizer(1e-2), O.MomentumOptimizer(0.1, 0.9), O.GradientDescentOptimizer(0.1)],
                         ids=["adam", "momentum", "sgd"])
@pytest.mark.parametrize("nu", [False, True])
def test_flat_applier_shadow_follows_ema_update(opt, nu):
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(N, generator=g)
    grads = [torch.randn(N, generator=g) for _ in range(6)]
    off, p_off = O.FlatApplier(opt, N), p0.clone()
    on, p_on = O.FlatApplier(dataclasses.replace(opt, ema_decay=0.9, ema_num_updates=nu), N), p0.clone()
    assert off.ema is None and on.ema is None
    ref = p0.double()
    for t, gr in enumerate(grads, 1):
        off.apply(p_off, gr)
        on.apply(p_on, gr)
        assert torch.equal(p_on, p_off)  # the update itself is untouched, bit for bit
        ref = O.ema_update(ref, p_on, 0.9, t, nu)
        # fp32 shadow against the fp64 recurrence: a few roundings per step, none amplified
        assert (on.ema.double() - ref).abs().max() <= 6 * 5 * 2.0 ** -24 * max(ref.abs().max(), p_on.abs().max())
    assert off.ema is None
    for a, b in zip(on.slots().values(), off.slots().values()):
        assert torch.equal(a, b)
    assert not torch.equal(on.ema, p_on)
    on.reset_ema(p_on)
    assert torch.equal(on.ema, p_on) and on.ema.data_ptr() != p_on.data_ptr()


# ---------------------------------------------------------------- TorchMnistRunner
def _batches(n, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, B, 784, generator=g), torch.randint(0, 10, (n, B), generator=g, dtype=torch.int32)


def _init():
    return M.flat_from_dict(M.init_params(13)) * 0.05


def _runner(opt):
    r = TorchMnistRunner(B, opt, keep_prob=1.0)
    r.load_flat(_init(), {}, 0)
    return r


@pytest.mark.parametrize("base", [O.AdamOptimizer(1e-2), O.MomentumOptimizer(0.05, 0.9)], ids=["adam", "momentum"])
def test_torch_runner_shadow_params_and_evaluate(base):
    x, y = _batches(6)
    off = _runner(base)
    on = _runner(dataclasses.replace(base, ema_decay=0.9, ema_num_updates=True))
    assert on.ema_on and not off.ema_on
    assert torch.equal(on.ema_params(), on.params())
    ref = on.params().double()
    for t in range(6):
        off.train_step(x[t], y[t])
        on.train_step(x[t], y[t])
        assert torch.equal(on.params(), off.params())
        ref = O.ema_update(ref, on.params(), 0.9, t + 1, True)
        assert (on.ema_params().double() - ref).abs().max() <= 6 * 5 * 2.0 ** -24 * max(ref.abs().max(), on.params().abs().max())
        assert on.current_ema_decay() == O.ema_decay_at(0.9, t + 1, True)
    assert on.global_step() == 6
    # evaluation from the averages = evaluating a runner whose parameters are the averages
    twin = _runner(base)
    twin.set_params(on.ema_params())
    assert on.evaluate(x[0], y[0], use_ema=True) == twin.evaluate(x[0], y[0])
    assert on.evaluate(x[0], y[0]) == on.evaluate(x[0], y[0], use_ema=False) == off.evaluate(x[0], y[0])
    assert on.evaluate(x[0], y[0], use_ema=True) != on.evaluate(x[0], y[0])
    # set_params starts the average again
    on.set_params(_init())
    assert torch.equal(on.ema_params(), on.params())


# ---------------------------------------------------------------- checkpoint
def test_checkpoint_carries_the_averages(tmp_path):
    from tensorflow_distributed_amd.training import checkpoint

    x, y = _batches(5)
    opt = O.AdamOptimizer(1e-2, ema_decay=0.9, ema_num_updates=True)
    a = _runner(opt)
    for t in range(3):
        a.train_step(x[t], y[t])
    sd = a.state_dict_tf()
    keys = [tf + EMA_SUFFIX for _, tf, _ in M.PARAM_SPECS]
    assert EMA_SUFFIX == "/ExponentialMovingAverage" and len(keys) == 8
    for (key, tf, _), k in zip(M.PARAM_SPECS, keys):
        assert k in sd and sd[k].shape == sd[tf].shape
        assert np.array_equal(sd[k], M.dict_from_flat(a.ema_params())[key].numpy())
    # through the bundle files and back, exactly
    saver = checkpoint.Saver()
    got = saver.restore(saver.save(str(tmp_path), sd, global_step=3))
    for k in keys:
        assert np.array_equal(got[k], sd[k])
    b = _runner(opt)
    b.load_state_dict_tf(got)
    assert torch.equal(b.ema_params(), a.ema_params()) and torch.equal(b.params(), a.params())
    for t in range(3, 5):
        a.train_step(x[t], y[t])
        b.train_step(x[t], y[t])
    assert torch.equal(b.ema_params(), a.ema_params()) and torch.equal(b.params(), a.params())
    # a checkpoint without them: the shadow starts from the restored values
    c = _runner(opt)
    c.load_state_dict_tf({k: v for k, v in sd.items() if not k.endswith(EMA_SUFFIX)})
    assert torch.equal(c.ema_params(), c.params()) and torch.equal(c.params(), M.flat_from_dict(
        {key: torch.from_numpy(sd[tf]) for key, tf, _ in M.PARAM_SPECS}))
    # EMA off: the averages in the checkpoint are ignored, and none is written
    d = _runner(O.AdamOptimizer(1e-2))
    d.load_state_dict_tf(sd)
    assert d.applier.ema is None and not any(k.endswith(EMA_SUFFIX) for k in d.state_dict_tf())
    assert torch.equal(d.params(), c.params())


# ---------------------------------------------------------------- flags
def _with_flags(argv, fn):
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog"] + argv)
        return fn(dist_main)
    finally:
        F.FLAGS.reset()


def test_ema_flags_reach_every_optimizer():
    assert _with_flags([], lambda d: d._make_optimizer()) == O.AdamOptimizer(0.01)
    assert _with_flags(["--ema_decay=0.99"], lambda d: d._make_optimizer()) == \
        O.AdamOptimizer(0.01, ema_decay=0.99, ema_num_updates=True)
    assert _with_flags(["--ema_decay=0.99", "--ema_num_updates=False", "--optimizer=momentum"],
                       lambda d: d._make_optimizer()) == O.MomentumOptimizer(0.01, 0.9, ema_decay=0.99)
    assert _with_flags(["--ema_decay=0.5", "--optimizer=sgd"], lambda d: d._make_optimizer()).ema_decay == 0.5
    _with_flags(["--ema_decay=0.99"], lambda d: d.check_ema_flags(2))  # the supported combination passes
    _with_flags(["--ema_decay=0.99", "--dp_schedule=sfb"], lambda d: d.check_ema_flags(2))
    _with_flags(["--sync_replicas=False"], lambda d: d.check_ema_flags(2))  # and no EMA, no complaint
    assert _with_flags([], lambda d: (d.FLAGS.ema_decay, d.FLAGS.ema_num_updates, d.FLAGS.ema_eval)) == (0.0, True, True)


@pytest.mark.parametrize("argv,word", [
    (["--ema_decay=0.99", "--sync_replicas=False"], "sync_replicas"),
    (["--ema_decay=0.99", "--replicas_to_aggregate=1"], "backup workers"),
    (["--ema_decay=0.99", "--model=resnet18"], "resnet18"),
    (["--ema_decay=0.99", "--model=resnet50"], "resnet50"),
    (["--ema_decay=0.99", "--dp_schedule=sfb+zero"], "ZeRO"),
    (["--ema_decay=0.99", "--dp_schedule=sfb+zero+mr"], "ZeRO"),
    (["--ema_decay=-0.5"], "ema_decay"),
    (["--ema_decay=1"], "ema_decay"),
])
def test_unsupported_ema_combinations_are_flag_errors(argv, word):
    with pytest.raises(ValueError, match=word):
        _with_flags(argv, lambda d: d.check_ema_flags(2))


def test_ema_drops_the_zero_schedules_from_auto():
    from tensorflow_distributed_amd.parallel import schedule as SCH

    assert _with_flags([], lambda d: d.dp_candidates("cuda", "bf16")) == list(SCH.MNIST_SCHEDULES)
    got = _with_flags(["--ema_decay=0.99"], lambda d: d.dp_candidates("cuda", "bf16"))
    assert got == [k for k in SCH.MNIST_SCHEDULES if "zero" not in k] and "sfb" in got and "allreduce" in got
    assert _with_flags(["--ema_decay=0.99"], lambda d: d.dp_candidates("cuda", "fp32")) == ["allreduce"]
    assert _with_flags(["--ema_decay=0.99"], lambda d: d.dp_candidates("cpu", "bf16")) == list(SCH.CPU_SCHEDULES)
    with pytest.raises(ValueError, match="sfb\\+zero"):
        _with_flags(["--ema_decay=0.99", "--dp_schedule=sfb+zero"],
                    lambda d: d.choose_dp_schedule(lambda n: 1.0, 0, 2, "cuda"))


def test_flag_errors_come_before_any_process_group(monkeypatch):
    from tensorflow_distributed_amd.parallel import cluster
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    def no_server(*a, **k):
        raise AssertionError("a Server was built before the flag check")

    monkeypatch.setattr(cluster, "Server", no_server)
    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog", "--ema_decay=0.99", "--sync_replicas=False", "--synthetic_data", "--data_dir=/nonexistent",
                       "--job_name=worker", "--task_index=0"])
        with pytest.raises(ValueError, match="sync_replicas"):
            dist_main.main()
    finally:
        F.FLAGS.reset()


def test_sync_replicas_variable_averages_reach_the_base_optimizer():
    va = O.ExponentialMovingAverage(0.999, num_updates=True)
    sro = O.SyncReplicasOptimizer(O.AdamOptimizer(0.01), 2, 2, variable_averages=va)
    assert O.base_optimizer(sro) == O.AdamOptimizer(0.01, ema_decay=0.999, ema_num_updates=True)
    assert sro.resolve(2).opt == sro.opt and sro.resolve(2).variable_averages == va
    assert O.base_optimizer(O.SyncReplicasOptimizer(O.AdamOptimizer(0.01), 2, 2)) == O.AdamOptimizer(0.01)
    r = TorchMnistRunner(B, sro, keep_prob=1.0)
    assert r.ema_on and r.opt.ema_decay == 0.999
    ap = O.FlatApplier(O.SyncReplicasOptimizer(O.MomentumOptimizer(0.1), variable_averages=O.ExponentialMovingAverage(0.5)), 4)
    p = torch.zeros(4)
    ap.load_ema(torch.full((4,), 8.0))
    for want in (4.0, 2.0, 1.0):
        ap.apply(p, torch.zeros(4))
        assert torch.equal(ap.ema, torch.full((4,), want))


@pytest.mark.slow
def test_mnist_single_trains_from_the_averages_and_restores(tmp_path):
    import subprocess
    import sys
    import os

    from tensorflow_distributed_amd.training import checkpoint

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "mnist_single.py"), "--cpu", "--ema_decay=0.99", "--training_iters=64",
           "--batch_size=16", "--eval_batches=1", f"--logdir={tmp_path}", f"--data_dir={tmp_path}/data"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Accuracy from the moving averages" in out.stdout and "Mean Accuracy" in out.stdout
    names = [n for n, _ in checkpoint.list_variables(checkpoint.latest_checkpoint(str(tmp_path)))]
    assert sum(n.endswith(EMA_SUFFIX) for n in names) == 8
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "Restored" in out.stdout, out.stderr
