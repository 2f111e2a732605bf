"""Global-norm gradient clipping (tf.clip_by_global_norm) on the host side: the fp64 definition, the
flat applier, sync data parallelism over Gloo (the norm is taken of the AVERAGED gradient, so N ranks
at batch B stay equal to one process at N*B), the launcher's flags and its metrics."""
import json
import math

import pytest
import torch

from tensorflow_distributed_amd.training import optimizers as O

from dist_util import run_ranks


# ---------------------------------------------------------------- the definition
def _vec(n=1000, seed=5):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_factor_is_exactly_one_while_the_norm_is_within_the_bound():
    g = _vec()
    norm = math.sqrt(float((g * g).sum()))
    for c in (norm, norm * (1 + 2 ** -40), 2 * norm, 1e30):
        f, n = O.clip_by_global_norm(g, c)
        assert f == 1.0 and n == norm
    f, n = O.clip_by_global_norm(torch.zeros(8), 3.0)
    assert f == 1.0 and n == 0.0
    # TF's form, clip_norm * min(1 / norm, 1 / clip_norm), is 1 only up to rounding; this one exactly
    assert any(c * min(1.0 / 3.0, 1.0 / c) != 1.0 for c in (0.1 * k for k in range(1, 200)))
    assert all(O.clip_by_global_norm(torch.tensor([3.0]), 3.0 + 0.1 * k)[0] == 1.0 for k in range(200))


def test_active_factor_brings_the_norm_to_the_bound():
    g = _vec()
    norm = math.sqrt(float((g * g).sum()))
    for c in (norm * (1 - 2 ** -40), 0.5 * norm, 1e-3 * norm, 1e-30):
        f, n = O.clip_by_global_norm(g, c)
        assert n == norm and f < 1.0
        assert f * n == pytest.approx(c, rel=4 * 2.0 ** -53)
    with pytest.raises(ValueError):
        O.clip_by_global_norm(g, 0.0)


def test_scale_folds_into_norm_and_factor():
    g = _vec()
    raw = math.sqrt(float((g * g).sum()))
    f, n = O.clip_by_global_norm(g, 0.125 * raw, scale=0.25)  # the averaged gradient's norm is raw / 4
    assert n == 0.25 * raw
    assert f == pytest.approx(0.25 * 0.5, rel=4 * 2.0 ** -53)  # 1/N, times 1/2 for the clip
    f, n = O.clip_by_global_norm(g, raw, scale=0.25)  # inactive: the factor is the bare 1/N
    assert f == 0.25 and n == 0.25 * raw
    # the clipped averaged gradient has norm clip_norm
    assert float((g * O.clip_by_global_norm(g, 0.125 * raw, 0.25)[0]).norm()) == pytest.approx(0.125 * raw, rel=1e-12)


def test_non_finite_norms_get_no_special_handling():
    f, n = O.clip_by_global_norm(torch.tensor([float("inf"), 1.0]), 2.0)
    assert n == float("inf") and f == 0.0
    f, n = O.clip_by_global_norm(torch.tensor([float("nan"), 1.0]), 2.0)
    assert math.isnan(n) and f == 1.0  # the NaN gradient itself propagates, as without clipping


# ---------------------------------------------------------------- FlatApplier
N = 257
CLIP = 0.05


def _grads(steps=5, seed=9):
    g = torch.Generator().manual_seed(seed)
    # norms of about 0.16, 0.016, ...: the first steps clip at CLIP = 0.05, the later ones do not
    return [torch.randn(N, generator=g) * (1e-2 * 10.0 ** -(s // 2)) for s in range(steps)]


def _clip(g, c, scale=1.0):
    norm = scale * math.sqrt(float(g.double().pow(2).sum()))
    return g * (scale * (c / max(norm, c))), norm


def test_flat_applier_adam_clips_like_a_hand_written_reference():
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(1))
    ap = O.FlatApplier(O.AdamOptimizer(1e-2, clip_norm=CLIP), N)
    p, ref = p0.clone(), p0.clone()
    m, v = torch.zeros(N), torch.zeros(N)
    active = []
    for t, g in enumerate(_grads(), 1):
        ap.apply(p, g)
        gc, norm = _clip(g, CLIP)
        active.append(norm > CLIP)
        assert ap.last_grad_norm == norm and ap.last_clip_scale == pytest.approx(CLIP / max(norm, CLIP), rel=1e-15)
        lr_t = 1e-2 * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
        m = m + (gc - m) * (1 - 0.9)
        v = v + (gc * gc - v) * (1 - 0.999)
        ref = ref - lr_t * m / (v.sqrt() + 1e-8)
        torch.testing.assert_close(p, ref, rtol=1e-6, atol=1e-7)
    assert any(active) and not all(active), active
    plain = O.FlatApplier(O.AdamOptimizer(1e-2), N)
    q = p0.clone()
    for g in _grads():
        plain.apply(q, g)
    assert not torch.allclose(q, p, rtol=1e-4, atol=1e-5)  # the clip was felt


def test_flat_applier_momentum_clips_like_a_hand_written_reference():
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(2))
    ap = O.FlatApplier(O.MomentumOptimizer(0.1, 0.9, clip_norm=CLIP), N)
    p, ref, acc = p0.clone(), p0.clone(), torch.zeros(N)
    for g in _grads():
        ap.apply(p, g, 0.5)  # with the 1/N of a two-worker sum
        gc, norm = _clip(g, CLIP, 0.5)
        assert ap.last_grad_norm == norm
        acc = acc * 0.9 + gc
        ref = ref - 0.1 * acc
        torch.testing.assert_close(p, ref, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("opt", [O.AdamOptimizer(1e-2), O.MomentumOptimizer(0.1, 0.9), O.GradientDescentOptimizer(0.1)])
def test_flat_applier_without_clip_norm_is_bit_identical(opt):
    """clip_norm=None (the default, last field of every config) leaves today's arithmetic: spelled out."""
    assert opt.clip_norm is None
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(3))
    ap, p = O.FlatApplier(opt, N), p0.clone()
    ref, m, v = p0.clone(), torch.zeros(N), torch.zeros(N)
    for t, g in enumerate(_grads(), 1):
        ap.apply(p, g, 0.5)
        gs = g * 0.5
        if opt.kind == "adam":
            lr_t = opt.learning_rate * (1 - opt.beta2 ** t) ** 0.5 / (1 - opt.beta1 ** t)
            m.add_(gs - m, alpha=1 - opt.beta1)
            v.add_(gs * gs - v, alpha=1 - opt.beta2)
            ref.sub_(lr_t * m / (v.sqrt() + opt.epsilon))
        elif opt.kind == "momentum":
            m.mul_(opt.momentum).add_(gs)
            ref.sub_(opt.learning_rate * m)
        else:
            ref.sub_(opt.learning_rate * gs)
        assert torch.equal(p, ref)
    assert ap.last_grad_norm is None
    # a bound far above the norm changes no bit either
    import dataclasses

    ap2, p2 = O.FlatApplier(dataclasses.replace(opt, clip_norm=1e30), N), p0.clone()
    for g in _grads():
        ap2.apply(p2, g, 0.5)
    assert torch.equal(p2, p) and ap2.last_clip_scale == 1.0


# ---------------------------------------------------------------- sync DP over Gloo
DP_CLIP = 1.0


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 784, generator=g), torch.randint(0, 10, (n,), generator=g)


def _init():
    from tensorflow_distributed_amd.models import mnist_cnn as M

    return M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(4).items()})


def _dp_worker(rank, world, steps, B):
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
    from tensorflow_distributed_amd.parallel.sync_replicas import SyncReplicasStepper, broadcast_state

    r = TorchMnistRunner(B, O.AdamOptimizer(0.01, clip_norm=DP_CLIP), keep_prob=1.0, rank=rank)
    if rank == 0:
        r.load_flat(_init(), {}, 0)
    broadcast_state(r, 0)
    st = SyncReplicasStepper(r, rank, world, world)
    x, y = _data(B * world * steps, 11)
    norms = []
    for s in range(steps):
        lo = (s * world + rank) * B
        st.step(x[lo:lo + B], y[lo:lo + B])
        norms.append(r.last_grad_norm())
    return r.params().clone(), norms


@pytest.mark.slow
def test_clipped_sync_dp_equals_big_batch_single_process():
    """2 Gloo ranks at B=8 with clipping == one process at B=16: the norm is that of the averaged
    gradient, after the all-reduce. Tolerances: those of test_sync_dp_equals_big_batch_single_process."""
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    world, steps, B = 2, 3, 8
    outs = run_ranks(_dp_worker, world, steps, B, timeout=400)
    assert torch.equal(outs[0][0], outs[1][0]), "replicas diverged"
    assert outs[0][1] == outs[1][1]
    ref = TorchMnistRunner(B * world, O.AdamOptimizer(0.01, clip_norm=DP_CLIP), keep_prob=1.0)
    ref.load_flat(_init(), {}, 0)
    x, y = _data(B * world * steps, 11)
    ref_norms = []
    for s in range(steps):
        lo = s * world * B
        ref.train_step(x[lo:lo + world * B], y[lo:lo + world * B])
        ref_norms.append(ref.last_grad_norm())
    for (n, sc), (rn, rsc) in zip(outs[0][1], ref_norms):
        assert n == pytest.approx(rn, rel=1e-3) and sc == pytest.approx(rsc, rel=1e-3)
    assert ref_norms[0][1] < 1.0, ref_norms  # the clip is active: this is not the unclipped test again
    init = _init()
    got, want = outs[0][0], ref.params()
    d = (got - want).abs()
    assert ((got - init) - (want - init)).norm() / (want - init).norm() < 1e-3
    assert int((d > 1e-4 + 1e-3 * want.abs()).sum()) <= 3 and d.max() < 1e-3, d.max()


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


def test_clip_norm_flag_reaches_every_optimizer():
    assert _with_flags([], lambda d: d._make_optimizer()) == O.AdamOptimizer(0.01)
    assert _with_flags(["--clip_norm=5"], lambda d: d._make_optimizer()) == O.AdamOptimizer(0.01, clip_norm=5.0)
    assert _with_flags(["--clip_norm=5", "--optimizer=momentum"], lambda d: d._make_optimizer()) == \
        O.MomentumOptimizer(0.01, 0.9, clip_norm=5.0)
    assert _with_flags(["--clip_norm=0.5", "--optimizer=sgd"], lambda d: d._make_optimizer()).clip_norm == 0.5
    _with_flags(["--clip_norm=5"], lambda d: d.check_clip_norm_flags(2))  # the supported combination passes
    _with_flags(["--sync_replicas=False"], lambda d: d.check_clip_norm_flags(2))  # and no clip, no complaint


@pytest.mark.parametrize("argv,word", [
    (["--clip_norm=5", "--sync_replicas=False"], "sync_replicas"),
    (["--clip_norm=5", "--replicas_to_aggregate=1"], "backup workers"),
    (["--clip_norm=5", "--model=resnet18"], "resnet18"),
    (["--clip_norm=5", "--model=resnet50"], "resnet50"),
    (["--clip_norm=-1"], "clip_norm"),
])
def test_unsupported_clip_norm_combinations_are_flag_errors(argv, word):
    with pytest.raises(ValueError, match=word):
        _with_flags(argv, lambda d: d.check_clip_norm_flags(2))


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
        F.FLAGS.parse(["prog", "--clip_norm=5", "--sync_replicas=False", "--synthetic_data", "--data_dir=/nonexistent",
                       "--job_name=worker", "--task_index=0"])
        with pytest.raises(ValueError, match="sync_replicas"):
            dist_main.main()
    finally:
        F.FLAGS.reset()


def test_clip_norm_restricts_gpu_schedules_to_allreduce():
    from tensorflow_distributed_amd.parallel import schedule as SCH

    assert _with_flags([], lambda d: d.dp_candidates("cuda", "bf16")) == list(SCH.MNIST_SCHEDULES)
    assert len(SCH.MNIST_SCHEDULES) > 1
    assert _with_flags(["--clip_norm=5"], lambda d: d.dp_candidates("cuda", "bf16")) == ["allreduce"]
    assert _with_flags(["--clip_norm=5"], lambda d: d.dp_candidates("cuda", "fp32")) == ["allreduce"]
    for mode in ("fixed", "auto"):
        got = _with_flags(["--clip_norm=5", "--dp_schedule=" + mode],
                          lambda d: d.choose_dp_schedule(lambda name: 1.0, 0, 2, "cuda"))
        assert got[0] == "allreduce" and got[1] is None, got
    with pytest.raises(ValueError, match="allreduce"):  # a pinned sharded schedule is an error, not ignored
        _with_flags(["--clip_norm=5", "--dp_schedule=sfb"], lambda d: d.choose_dp_schedule(lambda n: 1.0, 0, 2, "cuda"))
    # the Gloo schedules all reduce the whole gradient: untouched
    assert _with_flags(["--clip_norm=5"], lambda d: d.dp_candidates("cpu", "bf16")) == list(SCH.CPU_SCHEDULES)


# ---------------------------------------------------------------- reporting
def test_supervisor_writes_global_norm(tmp_path):
    from tensorflow_distributed_amd.training import summary as S
    from tensorflow_distributed_amd.training.supervisor import Supervisor

    class Runner:
        opt = O.AdamOptimizer(0.01, clip_norm=1.0)

        def global_step(self):
            return 0

        def last_grad_norm(self):
            return 12.5, 0.08

    sv = Supervisor(True, str(tmp_path), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(7)
    sv.writer.close()
    got = {tag: v for step, tag, v in S.read_scalars(sv.writer.path) if step == 7}
    assert got["global_norm"] == 12.5
    Runner.opt = O.AdamOptimizer(0.01)
    sv = Supervisor(True, str(tmp_path / "b"), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(7)
    sv.writer.close()
    assert "global_norm" not in {tag for _, tag, _ in S.read_scalars(sv.writer.path)}


@pytest.mark.slow
def test_launcher_run_logs_grad_norm_and_clip_scale(tmp_path):
    from tensorflow_distributed_amd import launch

    mf = tmp_path / "m.jsonl"
    r = launch.launch(1, 2, ["--train_steps=4", f"--logdir={tmp_path}", f"--metrics_file={mf}", "--clip_norm=1",
                             "--synthetic_data", "--eval_batches=1", "--data_dir=/nonexistent"], echo=False,
                      timeout_s=300)
    assert r["ok"], r["outputs"]
    steps = [rec for rec in (json.loads(ln) for ln in open(mf)) if "step" in rec and "event" not in rec]
    assert len(steps) == 4
    for rec in steps:
        assert math.isfinite(rec["grad_norm"]) and rec["grad_norm"] > 0, rec
        assert 0 < rec["clip_scale"] <= 1, rec
    # N(0,1)-initialised variables: the first gradients are far above 1, so the clip was active
    assert steps[0]["clip_scale"] < 1 and steps[0]["grad_norm"] * steps[0]["clip_scale"] == pytest.approx(1.0, rel=1e-6)
