"""RMSProp and Adagrad off the GPU: the fp64 definitions and FlatApplier on exact cases, TF's initial slot
values, the composition with the guard / clip / schedules / EMA, config validation, the flags of dist_main and
mnist_single, the TF checkpoint names through a save / restore round trip, and one Gloo parameter-server run."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O

from dist_util import run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- exact cases
def _t(*v):
    return torch.tensor(v, dtype=torch.float32)


def test_fp64_definitions_on_exact_cases():
    """Every quantity is a short binary fraction: fp64 (and an fp32 emulation of it) is exact."""
    p, ms, mom = O.rmsprop_update(_t(1.0), _t(0.25), _t(0.0), _t(0.5), 0.25, 0.5, 0.5, 0.0)
    assert (p.item(), ms.item(), mom.item()) == (0.75, 0.25, 0.25) and p.dtype == torch.float64
    p, ms, mom = O.rmsprop_update(p, ms, mom, _t(0.5), 0.25, 0.5, 0.5, 0.0)
    assert (p.item(), ms.item(), mom.item()) == (0.375, 0.25, 0.375)
    p, ms, mom, mg = O.rmsprop_update(_t(1.0), _t(1.5), _t(0.0), _t(1.0), 0.25, 0.5, 0.0, 0.0, mg=_t(0.0))
    assert (p.item(), ms.item(), mom.item(), mg.item()) == (0.75, 1.25, 0.25, 0.5)
    p, acc = O.adagrad_update(_t(1.0), _t(0.1875), _t(0.25), 0.5)
    assert (p.item(), acc.item()) == (0.75, 0.25)


def test_flat_applier_on_exact_cases_and_slot_order():
    a = O.FlatApplier(O.RMSPropOptimizer(0.25, 0.5, 0.5, 0.0), 3)
    assert list(a.slots()) == ["ms", "mom"]
    a.ms.fill_(0.25)
    p = torch.ones(3)
    for want in ((0.75, 0.25, 0.25), (0.375, 0.25, 0.375)):
        a.apply(p, torch.full((3,), 0.5))
        assert (p[1].item(), a.ms[1].item(), a.mom[1].item()) == want
    assert a.t == 2 and p.dtype == torch.float32
    a = O.FlatApplier(O.RMSPropOptimizer(0.25, 0.5, 0.0, 0.0, centered=True), 3)
    assert list(a.slots()) == ["ms", "mg", "mom"]
    a.ms.fill_(1.5)
    p = torch.ones(3)
    a.apply(p, torch.ones(3))
    assert [x[2].item() for x in (p, a.ms, a.mg, a.mom)] == [0.75, 1.25, 0.5, 0.25]
    a = O.FlatApplier(O.AdagradOptimizer(0.5, 0.1875), 3)
    assert list(a.slots()) == ["accum"]
    p = torch.ones(3)
    a.apply(p, torch.full((3,), 0.25))
    assert (p[0].item(), a.accum[0].item()) == (0.75, 0.25)
    assert a.powers() == {}


def test_slots_start_at_tfs_initial_values():
    a = O.FlatApplier(O.RMSPropOptimizer(centered=True), 5)
    assert (a.ms == 1).all() and (a.mom == 0).all() and (a.mg == 0).all()
    a = O.FlatApplier(O.AdagradOptimizer(), 5)
    assert (a.accum == np.float32(0.1)).all()
    a = O.FlatApplier(O.AdagradOptimizer(initial_accumulator_value=2.0), 5)
    a.accum.fill_(9.0)
    a.reset_slots()
    assert (a.accum == 2.0).all()
    assert all((s == 0).all() for s in O.FlatApplier(O.AdamOptimizer(), 5).slots().values())
    # defaults of the configs
    r, g = O.RMSPropOptimizer(), O.AdagradOptimizer()
    assert (r.learning_rate, r.decay, r.momentum, r.epsilon, r.centered, r.name, r.kind) == \
        (0.001, 0.9, 0.0, 1e-10, False, "RMSProp", "rmsprop")
    assert (g.learning_rate, g.initial_accumulator_value, g.name, g.kind) == (0.01, 0.1, "Adagrad", "adagrad")


def test_centered_denominator_is_not_clamped():
    """ms' - mg'^2 + eps < 0 gives NaN, as TF's kernel does."""
    p, ms, mom, mg = O.rmsprop_update(_t(1.0), _t(0.0), _t(0.0), _t(0.0), 0.1, 0.5, 0.0, 0.0, mg=_t(1.0))
    assert math.isnan(p.item()) and ms.item() == 0.0 and mg.item() == 0.5


# ---------------------------------------------------------------- composition around the update
CONFIGS = [lambda **kw: O.RMSPropOptimizer(0.25, 0.5, 0.5, 2.0 ** -10, **kw),
           lambda **kw: O.RMSPropOptimizer(0.25, 0.5, 0.5, 2.0 ** -10, centered=True, **kw),
           lambda **kw: O.AdagradOptimizer(0.25, 0.5, **kw)]


@pytest.mark.parametrize("mk", CONFIGS, ids=["rmsprop", "centered", "adagrad"])
def test_skipped_step_keeps_every_slot_and_advances_t(mk):
    a = O.FlatApplier(mk(skip_nonfinite=True, ema_decay=0.5), 4)
    p = _t(1.0, -2.0, 0.5, 0.25)
    a.apply(p, _t(0.5, 0.25, -1.0, 2.0))
    before = [p.clone(), a.ema.clone()] + [s.clone() for s in a.slots().values()]
    a.apply(p, _t(0.5, float("inf"), -1.0, 2.0))
    after = [p, a.ema] + list(a.slots().values())
    assert all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in zip(before, after))
    assert a.t == 2 and a.skipped_steps == 1 and not a.last_step_ok
    a.apply(p, _t(0.5, 0.25, -1.0, 2.0))
    assert a.t == 3 and a.last_step_ok and not torch.equal(p, before[0]) and torch.isfinite(p).all()


@pytest.mark.parametrize("mk", CONFIGS, ids=["rmsprop", "centered", "adagrad"])
def test_clip_scale_schedule_and_ema_compose(mk):
    g = _t(3.0, -4.0, 0.0, 0.0)  # norm 5
    # scale 0.5 brings the norm to the clip_norm of 2.5: the clip part is exactly 1, the plain update with g * 0.5
    a, b = O.FlatApplier(mk(clip_norm=2.5), 4), O.FlatApplier(mk(), 4)
    pa, pb = torch.ones(4), torch.ones(4)
    a.apply(pa, g, 0.5)
    b.apply(pb, g * 0.5)
    assert torch.equal(pa, pb) and all(torch.equal(x, y) for x, y in zip(a.slots().values(), b.slots().values()))
    assert a.last_grad_norm == 2.5 and a.last_clip_scale == 1.0
    a.apply(pa, g)  # norm 5 > 2.5: the clip factor 0.5 multiplies g
    b.apply(pb, g * 0.5)
    assert torch.equal(pa, pb) and a.last_clip_scale == 0.5
    # schedules are read at t - 1: the second update uses values[1]
    sched = O.PiecewiseConstant([0], [0.25, 0.125])
    a = O.FlatApplier(mk(), 4)
    a.opt.learning_rate = sched
    c = O.FlatApplier(mk(), 4)
    pa, pc = torch.ones(4), torch.ones(4)
    for lr in (0.25, 0.125):
        c.opt.learning_rate = lr
        a.apply(pa, g)
        c.apply(pc, g)
        assert torch.equal(pa, pc)
    # EMA follows p'
    a = O.FlatApplier(mk(ema_decay=0.75), 4)
    pa = torch.ones(4)
    a.apply(pa, g)
    assert torch.equal(a.ema, torch.ones(4) + 0.25 * (pa - torch.ones(4)))


def test_config_validation_and_sync_replicas_forwarding():
    for bad in (dict(decay=1.0), dict(decay=-0.1), dict(momentum=-0.5), dict(epsilon=-1e-3), dict(ema_decay=1.0),
                dict(accum_steps=0)):
        with pytest.raises(ValueError):
            O.RMSPropOptimizer(**bad)
    for bad in (dict(initial_accumulator_value=0.0), dict(initial_accumulator_value=-1.0), dict(ema_decay=0.0 - 1),
                dict(accum_steps=1.5)):
        with pytest.raises(ValueError):
            O.AdagradOptimizer(**bad)
    for base in (O.RMSPropOptimizer(centered=True), O.AdagradOptimizer()):
        s = O.SyncReplicasOptimizer(base, variable_averages=O.ExponentialMovingAverage(0.9, True), skip_nonfinite=True)
        assert s.opt.ema_decay == 0.9 and s.opt.ema_num_updates and s.opt.skip_nonfinite and s.opt.kind == base.kind
        assert O.base_optimizer(s) is s.opt and not O.is_layerwise(s)


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


def test_optimizer_flags_build_the_configs():
    mk = lambda d: d._make_optimizer()  # noqa: E731
    assert _with_flags(["--optimizer=rmsprop"], mk) == O.RMSPropOptimizer(0.01)
    # --momentum is momentum's / lars's: its default of 0.9, or a given value, does not reach RMSProp
    assert _with_flags(["--optimizer=rmsprop", "--momentum=0.8"], mk).momentum == 0.0
    assert _with_flags(["--optimizer=rmsprop", "--rmsprop_decay=0.95", "--rmsprop_momentum=0.5", "--rmsprop_epsilon=1e-6",
                        "--rmsprop_centered", "--clip_norm=5", "--ema_decay=0.9", "--skip_nonfinite",
                        "--grad_accum_steps=2"], mk) == \
        O.RMSPropOptimizer(0.01, 0.95, 0.5, 1e-6, True, clip_norm=5.0, ema_decay=0.9, ema_num_updates=True,
                           accum_steps=2, skip_nonfinite=True)
    assert _with_flags(["--optimizer=adagrad"], mk) == O.AdagradOptimizer(0.01)
    assert _with_flags(["--optimizer=adagrad", "--adagrad_init_accum=0.5", "--learning_rate=0.1"], mk) == \
        O.AdagradOptimizer(0.1, 0.5)
    for argv in (["--optimizer=rmsprop"], ["--optimizer=adagrad", "--dp_schedule=sfb+zero"], ["--model=resnet18"],
                 ["--optimizer=rmsprop", "--sync_replicas=False", "--ps_on_gpu=False", "--num_gpus=1"],
                 ["--optimizer=adagrad", "--sync_replicas=False"]):  # --num_gpus=0: the host parameter server
        _with_flags(argv, lambda d: d.check_rules_flags(2))


@pytest.mark.parametrize("opt", ["rmsprop", "adagrad"])
@pytest.mark.parametrize("argv,word", [
    (["--model=resnet18"], "resnet18"),
    (["--model=resnet50"], "resnet50"),
    (["--sync_replicas=False", "--num_gpus=1"], "--ps_on_gpu=False"),
    (["--replicas_to_aggregate=1", "--num_gpus=2"], "--ps_on_gpu=False"),
])
def test_unsupported_combinations_are_flag_errors(opt, argv, word):
    with pytest.raises(ValueError, match=word) as e:
        _with_flags(["--optimizer=" + opt] + argv, lambda d: d.check_rules_flags(2))
    assert "--optimizer=" + opt in str(e.value)


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
        F.FLAGS.parse(["prog", "--optimizer=rmsprop", "--model=resnet18", "--synthetic_data", "--data_dir=/nonexistent",
                       "--job_name=worker", "--task_index=0"])
        with pytest.raises(ValueError, match="resnet18"):
            dist_main.main()
    finally:
        F.FLAGS.reset()


@pytest.mark.parametrize("opt", ["rmsprop", "adagrad"])
def test_mnist_single_trains_on_the_cpu(opt, tmp_path):
    """A few iterations of the single-process trainer: the minibatch loss goes down."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "mnist_single.py"), "--cpu", "--optimizer", opt,
                          "--learning_rate", "0.001" if opt == "rmsprop" else "0.01", "--training_iters", "1100",
                          "--batch_size", "32", "--display_step", "8", "--eval_batches", "1", "--data_dir",
                          str(tmp_path / "no_data")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    losses = [float(line.rsplit("=", 1)[1]) for line in out.stdout.splitlines() if "Minibatch Loss" in line]
    print(opt, losses)
    assert len(losses) >= 3 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# ---------------------------------------------------------------- checkpoint names
def _batches(k, rows=4, seed=2):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(rows, 784, generator=g), torch.randint(0, 10, (rows,), generator=g)) for _ in range(k)]


@pytest.mark.parametrize("kind", ["rmsprop", "centered", "adagrad"])
def test_checkpoint_names_and_bit_identical_resume(kind, tmp_path):
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner, _slot_suffixes
    from tensorflow_distributed_amd.training import checkpoint

    cfg = {"rmsprop": O.RMSPropOptimizer(0.001, momentum=0.9), "centered": O.RMSPropOptimizer(0.001, centered=True),
           "adagrad": O.AdagradOptimizer(0.01)}[kind]
    want = {"rmsprop": [("/RMSProp", "ms"), ("/RMSProp_1", "mom")],
            "centered": [("/RMSProp", "ms"), ("/RMSProp_1", "mg"), ("/RMSProp_2", "mom")],
            "adagrad": [("/Adagrad", "accum")]}[kind]
    assert _slot_suffixes(cfg) == want
    import dataclasses
    assert _slot_suffixes(dataclasses.replace(cfg, name="opt2"))[0][0] == "/opt2"
    init = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(4).items()})
    b = _batches(3)

    def make():
        r = TorchMnistRunner(4, cfg, keep_prob=1.0)
        r.load_flat(init, {}, 0)
        return r

    a = make()
    for xy in b[:2]:
        a.train_step(*xy)
    saver = checkpoint.Saver()
    path = saver.save(str(tmp_path), a.state_dict_tf(), global_step=a.global_step())
    sd = saver.restore(path)
    for key, tf_name, shape in M.PARAM_SPECS:
        for suffix, slot in want:
            got = np.asarray(sd[tf_name + suffix])
            assert got.shape == tuple(shape)
            assert np.array_equal(got, M.dict_from_flat(a.slot_tensors()[slot])[key].numpy()), (tf_name, suffix)
        assert not any(n.startswith(tf_name + "/Adam") or n.startswith(tf_name + "/Momentum") for n in sd)
    assert len([n for n in sd if "/" in n]) == len(want) * len(M.PARAM_SPECS)
    r = make()
    r.load_state_dict_tf(sd)
    assert r.global_step() == 2 and r.applier.t == 2
    for run in (a, r):
        run.train_step(*b[2])
    n = M.NUM_PARAMS  # the padding behind the variables is in no checkpoint
    assert torch.equal(r.params()[:n], a.params()[:n]) and torch.isfinite(r.params()).all()
    for k in a.slot_tensors():
        assert torch.equal(r.slot_tensors()[k][:n], a.slot_tensors()[k][:n]), k
    assert not torch.equal(a.params(), init)


# ---------------------------------------------------------------- the Gloo parameter server
def _ps_role(rank, world):
    """1 PS + 2 workers, sync with R = 2: one averaged RMSProp update on the PS, whose slots come back."""
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
    from tensorflow_distributed_amd.parallel import async_ps

    opt = O.RMSPropOptimizer(0.001, momentum=0.9, centered=True)
    layout = async_ps.mnist_layout(1)
    if rank == 0:
        svc = async_ps.ParameterServerService(0, 1, 2, layout, opt, sync=True, replicas_to_aggregate=2)
        svc.serve()
        return ("ps", svc.updates, svc.global_step)
    wk = rank - 1
    names = list(O.FlatApplier(opt, 0).slots())
    client = async_ps.AsyncPSClient(wk, layout, slot_names=names)
    flat = torch.zeros(M.TOTAL)
    p0 = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(5).items()})
    if wk == 0:
        client.init(p0.clone())
    client.pull(flat)
    g = torch.randn(M.TOTAL, generator=torch.Generator().manual_seed(100 + wk)) * 1e-2
    step = client.push_pull(flat, g, local_step=0)
    out = {"step": step, "flat": flat.clone(), "names": names}
    if wk == 0:  # the chief's checkpoint reads what the PS holds
        r = TorchMnistRunner(4, opt, keep_prob=1.0)
        r.ps_client = client
        out["ckpt"] = r.state_dict_tf()
    client.stop()
    return ("worker", out)


@pytest.mark.slow
def test_gloo_parameter_server_applies_rmsprop_and_returns_its_slots():
    outs = run_ranks(_ps_role, 3)
    assert outs[0][1] == 1 and outs[0][2] == 1, outs[0]
    w0, w1 = outs[1][1], outs[2][1]
    assert w0["names"] == ["ms", "mg", "mom"] and w0["step"] == w1["step"] == 1
    opt = O.RMSPropOptimizer(0.001, momentum=0.9, centered=True)
    p = M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(5).items()})
    gs = [torch.randn(M.TOTAL, generator=torch.Generator().manual_seed(100 + w)) * 1e-2 for w in (0, 1)]
    ap = O.FlatApplier(opt, M.TOTAL)
    ap.apply(p, gs[0] + gs[1], 0.5)
    real = lambda t: torch.cat([v.reshape(-1) for v in M.dict_from_flat(t).values()])  # noqa: E731 (no padding)
    torch.testing.assert_close(real(w0["flat"]), real(p), rtol=1e-6, atol=1e-7)
    assert torch.equal(w0["flat"], w1["flat"])
    ck = w0["ckpt"]
    assert int(ck["global_step"]) == 1
    for key, tf_name, _ in M.PARAM_SPECS:
        for suffix, slot in (("/RMSProp", ap.ms), ("/RMSProp_1", ap.mg), ("/RMSProp_2", ap.mom)):
            want = M.dict_from_flat(slot)[key].numpy()
            np.testing.assert_allclose(ck[tf_name + suffix], want, rtol=1e-6, atol=1e-9)
        assert (ck[tf_name + "/RMSProp"] != 1.0).any()  # ms moved away from its initial 1 ...
    assert float(np.abs(ck["Variable_2/RMSProp"] - 1.0).max()) < 0.11  # ... by (g^2 - 1) * 0.1
