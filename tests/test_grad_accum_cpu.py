"""Gradient accumulation without a GPU: the accum_steps field of every optimizer config, the fp64
definition, the CPU runner (K micro-batches against one big batch, one comm call and one update per step),
the --grad_accum_steps flag of dist_main and mnist_single.py with its start-up refusals, the metrics JSONL,
and Gloo data parallelism at world 2."""
import dataclasses
import json

import pytest
import torch

from tensorflow_distributed_amd.training import optimizers as O

from dist_util import run_ranks

CONFIGS = [O.AdamOptimizer, O.GradientDescentOptimizer, O.MomentumOptimizer, O.LAMBOptimizer, O.LARSOptimizer]


# ---------------------------------------------------------------- the config field and the definition
@pytest.mark.parametrize("cls", CONFIGS)
def test_accum_steps_on_every_config(cls):
    assert cls().accum_steps == 1
    assert cls(accum_steps=4).accum_steps == 4
    assert dataclasses.replace(cls(), accum_steps=2).accum_steps == 2
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="accum_steps"):
            cls(accum_steps=bad)
    assert cls() == cls(accum_steps=1)
    assert O.base_optimizer(O.SyncReplicasOptimizer(cls(accum_steps=3))).accum_steps == 3


def test_accumulate_gradients_is_the_sequential_unscaled_sum():
    gs = [torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0.5, 0.25, 0.125]), torch.tensor([-1.0, 1e-9, 4.0])]
    got = O.accumulate_gradients(gs)
    assert got.dtype == torch.float64
    hand = torch.tensor([(1.0 + 0.5) + -1.0, (2.0 + 0.25) + 1e-9, (3.0 + 0.125) + 4.0], dtype=torch.float64)
    assert torch.equal(got, hand)
    assert torch.equal(O.accumulate_gradients(gs[:1]), gs[0].double())
    assert got.data_ptr() != gs[0].data_ptr() and torch.equal(gs[0], torch.tensor([1.0, 2.0, 3.0]))  # inputs untouched
    with pytest.raises(ValueError):
        O.accumulate_gradients([])
    with pytest.raises(ValueError):
        O.accumulate_gradients([torch.zeros(3), torch.zeros(4)])
    # fp64 keeps what a float32 running sum loses
    small = [torch.tensor([1.0], dtype=torch.float32)] + [torch.tensor([2.0 ** -25], dtype=torch.float32)] * 4
    assert float(O.accumulate_gradients(small)) == 1.0 + 4 * 2.0 ** -25


# ---------------------------------------------------------------- the CPU runner
def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 784, generator=g), torch.randint(0, 10, (n,), generator=g)


def _init():
    from tensorflow_distributed_amd.models import mnist_cnn as M

    return M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(4).items()})


def test_cpu_runner_k4_at_b8_is_one_step_at_b32():
    """SGD, keep_prob 1.0: the mean gradient of 32 rows is the sum of four 8-row means over 4, so the two
    updates differ by fp32 rounding alone (the autograd of both sides is fp32): 1e-5 relative is two
    orders above the 1e-7 of a float32 sum of four terms."""
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    x, y = _data(32, 3)
    calls = []

    def hook(g):
        calls.append(float(g.norm()))

    acc = TorchMnistRunner(8, O.GradientDescentOptimizer(0.1, accum_steps=4), keep_prob=1.0)
    one = TorchMnistRunner(32, O.GradientDescentOptimizer(0.1), keep_prob=1.0)
    assert acc.accum_steps == 4 and one.accum_steps == 1
    for r in (acc, one):
        r.load_flat(_init(), {}, 0)
        r.comm = hook
        r.train_step(x, y)
        assert r.global_step() == 1 and r.applier.t == 1
    assert len(calls) == 2  # one comm call per runner and step, not one per micro-batch
    assert calls[0] == pytest.approx(4 * calls[1], rel=1e-5)  # the hook sees the unscaled sum
    d_acc, d_one = acc.params() - _init(), one.params() - _init()
    rel = float((d_acc - d_one).norm() / d_one.norm())
    print("K=4 B=8 against B=32, relative difference of the update: %.3e" % rel)
    assert float(d_one.norm()) > 0 and rel < 1e-5
    with pytest.raises(AssertionError):
        acc.train_step(x[:8], y[:8])  # a step takes K * B rows


def test_cpu_runner_draws_a_dropout_mask_per_micro_batch_in_order():
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    x, y = _data(16, 5)
    acc = TorchMnistRunner(8, O.GradientDescentOptimizer(0.1, accum_steps=2), keep_prob=0.5, seed=2)
    ref = TorchMnistRunner(8, O.GradientDescentOptimizer(0.1), keep_prob=0.5, seed=2)
    for r in (acc, ref):
        r.load_flat(_init(), {}, 0)
    g0 = ref.compute_grads(x[:8], y[:8])[0].clone()
    g1 = ref.compute_grads(x[8:], y[8:])[0].clone()  # the generator moved on: the second mask
    acc.train_step(x, y)
    assert torch.equal(acc.grad, g0 + g1)
    assert float((acc.grad.double() - O.accumulate_gradients([g0, g1])).abs().max()) <= 1e-6 * float(acc.grad.abs().max())
    want = _init() - 0.1 * ((g0 + g1) * 0.5)
    assert torch.allclose(acc.params(), want, rtol=0, atol=1e-7)


# ---------------------------------------------------------------- Gloo DP at world 2
class _Counting:
    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def __call__(self, g):
        self.calls += 1
        return self.inner(g)

    def __getattr__(self, k):
        return getattr(self.inner, k)


def _dp_worker(rank, world, steps, B, K):
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
    from tensorflow_distributed_amd.parallel.sync_replicas import SyncReplicasStepper, broadcast_state

    r = TorchMnistRunner(B, O.AdamOptimizer(0.01, accum_steps=K), keep_prob=1.0, rank=rank)
    if rank == 0:
        r.load_flat(_init(), {}, 0)
    broadcast_state(r, 0)
    st = SyncReplicasStepper(r, rank, world, world)
    r.comm = _Counting(r.comm)
    x, y = _data(B * K * world * steps, 11)
    for s in range(steps):
        lo = (s * world + rank) * B * K
        st.step(x[lo:lo + B * K], y[lo:lo + B * K])
    return r.params().clone(), r.comm.calls, r.global_step()


@pytest.mark.slow
def test_gloo_dp_world2_k2_one_allreduce_per_step():
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    world, steps, B, K = 2, 3, 4, 2
    outs = run_ranks(_dp_worker, world, steps, B, K, timeout=400)
    assert torch.equal(outs[0][0], outs[1][0]), "replicas diverged"
    for _, calls, step in outs:
        assert calls == steps and step == steps  # one all-reduce per optimizer step
    # ... and equal, to rounding, to one process at batch K * B * world on the same rows
    ref = TorchMnistRunner(B * K * world, O.AdamOptimizer(0.01), keep_prob=1.0)
    ref.load_flat(_init(), {}, 0)
    x, y = _data(B * K * world * steps, 11)
    for s in range(steps):
        lo = s * world * B * K
        ref.train_step(x[lo:lo + world * B * K], y[lo:lo + world * B * K])
    init = _init()
    got, want = outs[0][0], ref.params()
    assert ((got - init) - (want - init)).norm() / (want - init).norm() < 1e-3  # Adam amplifies rounding near g = 0


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


def test_flag_reaches_every_optimizer():
    assert _with_flags([], lambda d: d._make_optimizer()) == O.AdamOptimizer(0.01)
    for name in ("adam", "sgd", "momentum", "lamb", "lars"):
        opt = _with_flags(["--grad_accum_steps=4", "--optimizer=" + name], lambda d: d._make_optimizer())
        assert opt.accum_steps == 4 and opt.kind == name
    _with_flags(["--grad_accum_steps=4"], lambda d: d.check_grad_accum_flags(2))  # the supported combination passes
    _with_flags(["--sync_replicas=False"], lambda d: d.check_grad_accum_flags(2))  # off: no complaint
    _with_flags(["--grad_accum_steps=2", "--dp_schedule=allreduce"], lambda d: d.check_grad_accum_flags(2))


@pytest.mark.parametrize("argv,word", [
    (["--grad_accum_steps=2", "--sync_replicas=False"], "sync_replicas"),
    (["--grad_accum_steps=2", "--replicas_to_aggregate=1"], "backup workers"),
    (["--grad_accum_steps=2", "--model=resnet18"], "resnet18"),
    (["--grad_accum_steps=2", "--dp_schedule=sfb"], "all-reduce schedule"),
    (["--grad_accum_steps=2", "--dp_schedule=sfb+zero+mr"], "all-reduce schedule"),
    (["--grad_accum_steps=0"], "grad_accum_steps"),
])
def test_unsupported_combinations_are_flag_errors(argv, word):
    with pytest.raises(ValueError, match=word):
        _with_flags(argv, lambda d: d.check_grad_accum_flags(2))


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
        F.FLAGS.parse(["prog", "--grad_accum_steps=2", "--sync_replicas=False", "--synthetic_data",
                       "--data_dir=/nonexistent", "--job_name=worker", "--task_index=0"])
        with pytest.raises(ValueError, match="sync_replicas"):
            dist_main.main()
    finally:
        F.FLAGS.reset()


def test_accumulation_restricts_gpu_schedules_to_allreduce():
    from tensorflow_distributed_amd.parallel import schedule as SCH

    assert _with_flags([], lambda d: d.dp_candidates("cuda", "bf16")) == list(SCH.MNIST_SCHEDULES)
    assert _with_flags(["--grad_accum_steps=2"], lambda d: d.dp_candidates("cuda", "bf16")) == ["allreduce"]
    for mode in ("fixed", "auto"):  # auto probes only allreduce: nothing to time
        got = _with_flags(["--grad_accum_steps=2", "--dp_schedule=" + mode],
                          lambda d: d.choose_dp_schedule(lambda name: 1.0, 0, 2, "cuda"))
        assert got[0] == "allreduce" and got[1] is None, got
    assert _with_flags(["--grad_accum_steps=2"], lambda d: d.dp_candidates("cpu", "bf16")) == list(SCH.CPU_SCHEDULES)


# ---------------------------------------------------------------- the launchers
@pytest.mark.slow
def test_launcher_run_counts_optimizer_steps_and_images(tmp_path):
    """1 ps + 2 workers, sync, --grad_accum_steps=2 on the CPU path: --train_steps counts optimizer steps,
    every step draws K * batch_size rows per worker, the JSONL carries accum_steps and counts K * B * world
    images per step."""
    from tensorflow_distributed_amd import launch

    mf = tmp_path / "m.jsonl"
    r = launch.launch(1, 2, ["--train_steps=3", f"--logdir={tmp_path}", f"--metrics_file={mf}", "--grad_accum_steps=2",
                             "--batch_size=8", "--synthetic_data", "--eval_batches=1", "--data_dir=/nonexistent"],
                      echo=False, timeout_s=300)
    assert r["ok"], r["outputs"]
    recs = [json.loads(ln) for ln in open(mf)]
    steps = [rec for rec in recs if "step" in rec and "event" not in rec]
    assert [rec["global_step"] for rec in steps] == [1, 2, 3]
    for rec in steps:
        assert rec["accum_steps"] == 2
        assert rec["images_per_sec"] == pytest.approx(2 * 8 * 2 / (rec["step_ms"] * 1e-3), rel=1e-6)
    out = "\n".join(r["outputs"].values())
    assert "2 micro-batches of 8 per optimizer step: 32 images per step" in out
    assert "images/sec (3 optimizer steps of 32 images)" in out


@pytest.mark.slow
def test_mnist_single_counts_optimizer_steps(tmp_path, capsys):
    import mnist_single

    rc = mnist_single.main(["--cpu", "--grad_accum_steps=2", "--batch_size=8", "--training_iters=80", "--display_step=2",
                            "--eval_batches=1", f"--data_dir={tmp_path}"])
    out = capsys.readouterr().out
    assert rc == 0
    assert "Iter 32, Minibatch Loss=" in out and "Iter 64, Minibatch Loss=" in out  # 16 images per step
    assert "4 optimizer steps of 2 micro-batches x 8 images" in out
    with pytest.raises(SystemExit):
        mnist_single.main(["--cpu", "--grad_accum_steps=0"])
