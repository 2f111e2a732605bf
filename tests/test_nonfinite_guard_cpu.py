"""The non-finite guard without a GPU: the fp64 definition, the skip_nonfinite field of every optimizer
config, the flat applier's identity update (parameters, slots and the moving average keep their bits; t is
consumed), the --skip_nonfinite flag of dist_main with its start-up refusals, the summary scalar, and a
2-worker Gloo dist_main run in which one worker's batch carries one inf pixel at one step."""
import dataclasses
import json
import math

import pytest
import torch

from tensorflow_distributed_amd.training import optimizers as O

from dist_util import free_port, run_ranks

INF, NAN = float("inf"), float("nan")
CONFIGS = [O.AdamOptimizer, O.GradientDescentOptimizer, O.MomentumOptimizer, O.LAMBOptimizer, O.LARSOptimizer]


# ---------------------------------------------------------------- the definition
def test_guard_of_a_finite_gradient_is_its_norm_and_ok():
    g = torch.randn(1000, generator=torch.Generator().manual_seed(5))
    norm, ok = O.nonfinite_guard(g)
    assert ok is True and norm == math.sqrt(float(g.double().pow(2).sum()))
    assert O.nonfinite_guard(g, 0.25) == (0.25 * norm, True)
    assert O.nonfinite_guard(torch.zeros(7)) == (0.0, True)
    assert O.nonfinite_guard(g)[0] == O.clip_by_global_norm(g, 1.0)[1]  # the norm clipping takes


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
@pytest.mark.parametrize("pos", [0, 3, 8])
def test_guard_sees_one_non_finite_element_anywhere(bad, pos):
    g = torch.full((9,), 0.5)
    g[pos] = bad
    norm, ok = O.nonfinite_guard(g)
    assert ok is False and not math.isfinite(norm)
    assert O.nonfinite_guard(g.double(), 1e-30)[1] is False  # no scale brings it back


def test_guard_skips_finite_gradients_whose_norm_overflows_fp32():
    """The device sums the squares in fp32: 1e20 squared is beyond it, 1e18 squared is not."""
    small = torch.full((64,), 1e-3)
    big = small.clone()
    big[5] = 1e20
    norm, ok = O.nonfinite_guard(big)
    assert ok is False and math.isfinite(norm)  # fp64 holds the norm; fp32 does not hold its square
    big[5] = 1e18
    assert O.nonfinite_guard(big)[1] is True
    assert O.nonfinite_guard(torch.tensor([1e19]), 1e20)[1] is False  # the scaled norm overflows
    assert O.nonfinite_guard(torch.tensor([1e19], dtype=torch.float64), 1.0)[1] is True


# ---------------------------------------------------------------- the config field
@pytest.mark.parametrize("cls", CONFIGS)
def test_skip_nonfinite_on_every_config_and_through_sync_replicas(cls):
    assert cls().skip_nonfinite is False
    assert cls(skip_nonfinite=True).skip_nonfinite is True
    assert cls() == cls(skip_nonfinite=False)
    assert O.base_optimizer(O.SyncReplicasOptimizer(cls(skip_nonfinite=True))).skip_nonfinite is True
    sr = O.SyncReplicasOptimizer(cls(), skip_nonfinite=True)
    assert sr.opt.skip_nonfinite is True and sr.resolve(2).opt.skip_nonfinite is True
    assert O.SyncReplicasOptimizer(cls()).resolve(2).opt.skip_nonfinite is False


# ---------------------------------------------------------------- FlatApplier
N = 257
SEGS = [(0, 128, O.LW_DECAY | O.LW_ADAPT), (128, 129, 0)]
APPLIER_CONFIGS = [O.AdamOptimizer(1e-2), O.GradientDescentOptimizer(0.1), O.MomentumOptimizer(0.1, 0.9),
                   O.LAMBOptimizer(1e-2, weight_decay=0.01), O.LARSOptimizer(0.1)]
IDS = ["adam", "sgd", "momentum", "lamb", "lars"]


def _applier(opt, **kw):
    opt = dataclasses.replace(opt, **kw)
    return O.FlatApplier(opt, N, segments=SEGS if opt.kind in O.LAYERWISE_KINDS else None)


def _grads(steps=3, seed=9):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, generator=g) * 1e-2 for _ in range(steps)]


def _bits(ap, p):
    out = {"p": p.clone()}
    out.update({k: v.clone() for k, v in ap.slots().items()})
    if ap.ema is not None:
        out["ema"] = ap.ema.clone()
    return {k: v.view(torch.int32) for k, v in out.items()}


@pytest.mark.parametrize("opt", APPLIER_CONFIGS, ids=IDS)
@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_poisoned_gradient_is_an_identity_update_that_consumes_its_t(opt, bad):
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(1))
    guarded = _applier(opt, skip_nonfinite=True, ema_decay=0.9)
    twin = _applier(opt, ema_decay=0.9)  # sees only the finite gradients, its t moved by hand
    p, q = p0.clone(), p0.clone()
    g0, g1, g2 = _grads()
    guarded.apply(p, g0, 0.5)
    twin.apply(q, g0, 0.5)
    before = _bits(guarded, p)
    poisoned = g1.clone()
    poisoned[N - 1] = bad
    guarded.apply(p, poisoned, 0.5)
    after = _bits(guarded, p)
    assert before.keys() == after.keys() and "ema" in before
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert guarded.skipped_steps == 1 and guarded.last_step_ok is False and guarded.t == 2
    twin.t += 1  # the skipped step consumed its t
    guarded.apply(p, g2, 0.5)
    twin.apply(q, g2, 0.5)
    assert guarded.skipped_steps == 1 and guarded.last_step_ok is True and guarded.t == 3
    a, b = _bits(guarded, p), _bits(twin, q)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("opt", APPLIER_CONFIGS, ids=IDS)
def test_finite_gradients_give_exactly_what_the_unguarded_applier_gives(opt):
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(2))
    for kw in ({}, {"clip_norm": 0.05}, {"ema_decay": 0.99, "ema_num_updates": True}):
        guarded, plain = _applier(opt, skip_nonfinite=True, **kw), _applier(opt, **kw)
        p, q = p0.clone(), p0.clone()
        for g in _grads():
            guarded.apply(p, g, 0.5)
            plain.apply(q, g, 0.5)
        a, b = _bits(guarded, p), _bits(plain, q)
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (kw, k)
        assert guarded.skipped_steps == 0 and guarded.last_step_ok is True and guarded.t == plain.t == 3
        assert plain.skipped_steps == 0


def test_a_skipped_first_step_starts_the_average_as_a_copy():
    ap = _applier(O.AdamOptimizer(1e-2), skip_nonfinite=True, ema_decay=0.9)
    p = torch.randn(N, generator=torch.Generator().manual_seed(3))
    p0 = p.clone()
    ap.apply(p, torch.full((N,), NAN))
    assert torch.equal(p, p0) and torch.equal(ap.ema, p0) and ap.skipped_steps == 1
    assert not ap.m.any() and not ap.v.any()


def test_without_the_guard_the_poison_is_written():
    ap = _applier(O.AdamOptimizer(1e-2))
    p = torch.zeros(N)
    g = torch.zeros(N)
    g[4] = NAN
    ap.apply(p, g)
    assert torch.isnan(p[4]) and torch.isnan(ap.m[4]) and ap.skipped_steps == 0


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


def test_skip_nonfinite_flag_reaches_every_optimizer():
    assert _with_flags([], lambda d: d._make_optimizer()) == O.AdamOptimizer(0.01)
    for name in ("adam", "sgd", "momentum", "lamb", "lars"):
        opt = _with_flags(["--skip_nonfinite", "--optimizer=" + name], lambda d: d._make_optimizer())
        assert opt.skip_nonfinite is True, name
        assert _with_flags(["--optimizer=" + name], lambda d: d._make_optimizer()).skip_nonfinite is False
    opt = _with_flags(["--skip_nonfinite", "--ema_decay=0.9", "--clip_norm=2"], lambda d: d._make_optimizer())
    assert opt == O.AdamOptimizer(0.01, clip_norm=2.0, ema_decay=0.9, ema_num_updates=True, skip_nonfinite=True)
    _with_flags(["--skip_nonfinite"], lambda d: d.check_skip_nonfinite_flags(2))  # the supported combination passes
    for sched in ("fixed", "auto", "allreduce", "flat", "buckets"):
        _with_flags(["--skip_nonfinite", "--dp_schedule=" + sched], lambda d: d.check_skip_nonfinite_flags(2))
    _with_flags(["--sync_replicas=False", "--model=resnet18"], lambda d: d.check_skip_nonfinite_flags(2))  # off: silent


@pytest.mark.parametrize("argv,word", [
    (["--sync_replicas=False"], "sync_replicas"),
    (["--replicas_to_aggregate=1"], "backup workers"),
    (["--model=resnet18"], "resnet18"),
    (["--model=resnet50"], "resnet50"),
    (["--dp_schedule=sfb"], "dp_schedule=sfb"),
    (["--dp_schedule=sfb+zero+mr"], "SFB / ZeRO"),
    (["--dp_schedule=sfb+zero"], "all-reduce schedule"),
])
def test_unsupported_skip_nonfinite_combinations_are_flag_errors(argv, word):
    import re

    with pytest.raises(ValueError, match=re.escape(word)):
        _with_flags(["--skip_nonfinite"] + argv, lambda d: d.check_skip_nonfinite_flags(2))


def test_flag_errors_come_before_any_process_group(monkeypatch):
    """main() raises on the flags alone: the cluster's Server (its process groups) is never built."""
    from tensorflow_distributed_amd.parallel import cluster
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    def no_server(*a, **k):
        raise AssertionError("a Server was built before the flag check")

    monkeypatch.setattr(cluster, "Server", no_server)
    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog", "--skip_nonfinite", "--sync_replicas=False", "--synthetic_data", "--data_dir=/nonexistent",
                       "--job_name=worker", "--task_index=0"])
        with pytest.raises(ValueError, match="skip_nonfinite"):
            dist_main.main()
    finally:
        F.FLAGS.reset()


def test_skip_nonfinite_restricts_gpu_schedules_to_allreduce():
    from tensorflow_distributed_amd.parallel import schedule as SCH

    assert _with_flags([], lambda d: d.dp_candidates("cuda", "bf16")) == list(SCH.MNIST_SCHEDULES)
    assert _with_flags(["--skip_nonfinite"], lambda d: d.dp_candidates("cuda", "bf16")) == ["allreduce"]
    assert _with_flags(["--skip_nonfinite"], lambda d: d.dp_candidates("cuda", "fp32")) == ["allreduce"]
    assert _with_flags(["--skip_nonfinite"], lambda d: d.dp_candidates("cpu", "bf16")) == list(SCH.CPU_SCHEDULES)


# ---------------------------------------------------------------- reporting
def test_supervisor_writes_skipped_steps(tmp_path):
    from tensorflow_distributed_amd.training import summary as S
    from tensorflow_distributed_amd.training.supervisor import Supervisor

    class Runner:
        opt = O.AdamOptimizer(0.01, skip_nonfinite=True)

        def global_step(self):
            return 0

        def skipped_steps(self):
            return 3

    sv = Supervisor(True, str(tmp_path), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(7)
    sv.writer.close()
    got = {tag: v for step, tag, v in S.read_scalars(sv.writer.path) if step == 7}
    assert got["skipped_steps"] == 3.0
    Runner.opt = O.AdamOptimizer(0.01)
    sv = Supervisor(True, str(tmp_path / "b"), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(7)
    sv.writer.close()
    assert "skipped_steps" not in {tag for _, tag, _ in S.read_scalars(sv.writer.path)}


# ---------------------------------------------------------------- a 2-worker Gloo dist_main run
B, STEPS, POISON_STEP = 8, 4, 1


def _dist_main_worker(rank, world, ports, tmp):
    """One worker task of dist_main.main() in this process (the Gloo group is run_ranks's). Worker 1's
    second fed batch carries one inf pixel. The runner is kept so that its end state can be returned."""
    from tensorflow_distributed_amd.models import mnist_runner
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F
    from tensorflow_distributed_amd.utils import input_data

    kept = {}
    make = mnist_runner.make_runner

    def make_and_keep(*a, **k):
        kept["runner"] = make(*a, **k)
        return kept["runner"]

    read = input_data.read_data_sets

    def read_and_poison(*a, **k):
        mnist = read(*a, **k)
        next_batch, calls = mnist.train.next_batch, [0]

        def poisoned_next_batch(n, *aa, **kk):
            x, y = next_batch(n, *aa, **kk)
            if rank == 1 and calls[0] == POISON_STEP:
                x = x.copy()
                x[3, 300] = INF
            calls[0] += 1
            return x, y

        mnist.train.next_batch = poisoned_next_batch
        return mnist

    mnist_runner.make_runner = make_and_keep
    input_data.read_data_sets = read_and_poison
    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    mf = "%s/m%d.jsonl" % (tmp, rank)
    try:
        F.FLAGS.parse(["prog", "--skip_nonfinite", "--num_gpus=0", "--job_name=worker", "--task_index=%d" % rank,
                       "--ps_hosts=", "--worker_hosts=" + ",".join("127.0.0.1:%d" % p for p in ports),
                       "--train_steps=%d" % STEPS, "--batch_size=%d" % B, "--synthetic_data", "--data_dir=/nonexistent",
                       "--eval_batches=1", "--eval_batch_size=20", "--check_consistency_every=1", "--quiet",
                       "--logdir=%s/log%d" % (tmp, rank), "--metrics_file=" + mf, "--rendezvous_timeout=120"])
        dist_main.main()
    finally:
        F.FLAGS.reset()
        mnist_runner.make_runner = make
        input_data.read_data_sets = read
    r = kept["runner"]
    return r.params().clone(), r.skipped_steps(), r.global_step(), r.last_step_ok()


@pytest.mark.slow
def test_two_gloo_workers_skip_the_poisoned_step_together(tmp_path):
    """The guard reads the all-reduced gradient, so the worker with the clean batch skips too; --check_
    consistency_every=1 would raise on the first diverging step."""
    outs = run_ranks(_dist_main_worker, 2, [free_port(), free_port()], str(tmp_path), timeout=400)
    for p, skipped, step, ok in outs:
        assert skipped == 1 and step == STEPS and ok is True
        assert torch.isfinite(p).all()
        assert torch.equal(p.view(torch.int32), outs[0][0].view(torch.int32)), "replicas diverged"
    recs = [json.loads(ln) for ln in open(tmp_path / "m0.jsonl")]  # the chief's metrics file
    steps = [r for r in recs if "step" in r and "event" not in r]
    assert len(steps) == STEPS
    assert [r["step_ok"] for r in steps] == [s != POISON_STEP for s in range(STEPS)]
    assert [r["skipped_steps"] for r in steps] == [int(s >= POISON_STEP) for s in range(STEPS)]
    assert [r["global_step"] for r in steps] == list(range(1, STEPS + 1))  # a skipped step consumes its step
    final = [r for r in recs if r.get("event") == "final"]
    assert len(final) == 1 and final[0]["skipped_steps"] == 1
