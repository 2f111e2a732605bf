"""LAMB and LARS on the host side: the fp64 definitions on hand-computed cases, the flat applier against
a hand-written per-variable reference, sync data parallelism over Gloo (the norms are taken of the
AVERAGED gradient, so N ranks at batch B stay equal to one process at N*B), the launcher's flags, the
checkpoint's slot names and the trust ratios in the metrics and the summaries."""
import json
import math

import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import LW_ADAPT, LW_DECAY

from dist_util import run_ranks

BOTH = LW_DECAY | LW_ADAPT


# ---------------------------------------------------------------- the definitions
def test_trust_ratio_and_its_guards():
    assert O.trust_ratio(32.0, 64.0) == 0.5                       # LAMB: |p| / |u|
    assert O.trust_ratio(32.0, 16.0, True, 2.0 ** -3) == 0.25     # LARS: eeta |p| / |g|
    assert O.trust_ratio(32.0, 16.0, True, 2.0 ** -3, 0.5) == 0.125
    assert O.trust_ratio(32.0, 16.0, True, 2.0 ** -3, 0.0, 16.0) == 0.125  # eps in the denominator
    for eeta in (None, 2.0 ** -3):
        assert O.trust_ratio(0.0, 16.0, True, eeta) == 1.0
        assert O.trust_ratio(32.0, 0.0, True, eeta) == 1.0
        assert O.trust_ratio(32.0, 16.0, False, eeta) == 1.0      # not adapted


def test_lars_update_exact_cases():
    """p = 0.5, g = 0.25 over 4096 elements, eeta = 2^-3, eps = 0, lr = 0.5, mu = 0."""
    p, g, z = torch.full((4096,), 0.5), torch.full((4096,), 0.25), torch.zeros(4096)
    for lam, r in ((0.0, 0.25), (0.5, 0.125)):
        p2, a2, nr = O.lars_update(p, z, g, 0.5, 0.0, lam, 2.0 ** -3, 0.0)
        assert nr == (32.0, 16.0, r)
        assert (a2 == 2.0 ** -5).all() and (p2 == 0.46875).all()
    # a variable that is not decayed uses lambda = 0, one that is not adapted r = 1
    assert O.lars_update(p, z, g, 0.5, 0.0, 0.5, 2.0 ** -3, 0.0, decay=False)[2] == (32.0, 16.0, 0.25)
    p2, a2, nr = O.lars_update(p, z, g, 0.5, 0.0, 0.5, 2.0 ** -3, 0.0, adapt=False)
    assert nr[2] == 1.0 and (a2 == 0.5 * (0.25 + 0.25)).all()
    # mu = 0.5, two steps
    p2, a2, _ = O.lars_update(p, z, g, 0.5, 0.5, 0.0, 2.0 ** -3, 0.0)
    p3, a3, nr = O.lars_update(p2, a2, g, 0.5, 0.5, 0.0, 2.0 ** -3, 0.0)
    assert nr == (30.0, 16.0, 0.234375) and (a3 == 0.044921875).all() and (p3 == 0.423828125).all()


def test_lamb_update_exact_case_at_t1():
    """b1 = 0.5, b2 = 0.75, eps = 0, lambda = 0, lr = 0.25, g = +-0.25: c_t = 1, u = +-1, r = 0.5."""
    sign = torch.ones(4096, dtype=torch.float64)
    sign[1::2] = -1
    p, z = torch.full((4096,), 0.5), torch.zeros(4096)
    p2, m2, v2, nr = O.lamb_update(p, z, z, 0.25 * sign, 1, 0.25, 0.5, 0.75, 0.0)
    assert nr == (32.0, 64.0, 0.5)
    assert torch.equal(m2, 0.125 * sign) and (v2 == 2.0 ** -6).all() and torch.equal(p2, 0.5 - 0.125 * sign)
    # with a decay and no adaptation it is AdamW: p' = p - lr (u_adam + lambda p)
    p2, _, _, nr = O.lamb_update(p, z, z, 0.25 * sign, 1, 0.25, 0.5, 0.75, 0.0, 0.5, adapt=False)
    assert nr[2] == 1.0 and torch.equal(p2, 0.5 - 0.25 * (sign + 0.25))


def test_segments_of_the_mnist_layout():
    s = M.segments(True)
    assert [(b, n) for b, n, _ in s] == [(0, 800), (800, 32), (832, 51200), (52032, 64), (52096, 3211264),
                                        (3263360, 1024), (3264384, 10240), (3274624, 10)]
    assert [f for _, _, f in s] == [BOTH, 0] * 4
    assert [f for _, _, f in M.segments(False)] == [BOTH] * 8
    assert sum(n for _, n, _ in s) == M.NUM_PARAMS and s[-1][0] + s[-1][1] == M.NUM_PARAMS < M.TOTAL
    assert O.check_segments(s, M.TOTAL) == s
    for bad, what in (([(8, 4, 3), (0, 4, 3)], "sorted"), ([(0, 8, 3), (4, 4, 3)], "overlaps"), ([(2, 4, 3)], "multiple of 4"),
                      ([(0, 0, 3)], "empty"), ([(60, 8, 3)], "outside"), ([(0, 4, 4)], "flags"), ([], "at least one")):
        with pytest.raises(ValueError, match=what):
            O.check_segments(bad, 64)


# ---------------------------------------------------------------- FlatApplier
N = 300


def _table(skip_bias):
    """Two weight / bias pairs with a gap after the first pair; [288, 300) belongs to no variable."""
    b = 0 if skip_bias else BOTH
    return [(0, 100, BOTH), (100, 7, b), (112, 160, BOTH), (272, 13, b)]


def _grads(steps=5, seed=9):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(N, generator=g) * 1e-2 for _ in range(steps)]


@pytest.mark.parametrize("skip_bias", [True, False])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_flat_applier_follows_a_hand_written_per_variable_reference(kind, skip_bias):
    lr, lam = 0.01, 0.05
    opt = O.LAMBOptimizer(lr, 0.9, 0.999, 1e-6, lam, skip_bias) if kind == "lamb" else \
        O.LARSOptimizer(lr, 0.9, lam, 1e-2, 1e-9, skip_bias)
    segs = _table(skip_bias)
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(1))
    ap, p = O.FlatApplier(opt, N, None, segs), p0.clone()
    ref = [p0[b:b + n].double() for b, n, _ in segs]
    s1 = [torch.zeros(n, dtype=torch.float64) for _, n, _ in segs]
    s2 = [torch.zeros(n, dtype=torch.float64) for _, n, _ in segs]
    for t, g in enumerate(_grads(), 1):
        ap.apply(p, g, 0.5)  # with the 1/N of a two-worker sum
        assert ap.t == t and len(ap.last_layer_norms) == len(segs)
        for i, (b, n, fl) in enumerate(segs):
            gs = g[b:b + n].double() * 0.5
            w, a = ref[i], fl == BOTH
            pn = math.sqrt(float((w * w).sum()))
            if kind == "lamb":
                s1[i] = 0.9 * s1[i] + 0.1 * gs
                s2[i] = 0.999 * s2[i] + 0.001 * gs * gs
                u = (s1[i] / (1 - 0.9 ** t)) / ((s2[i] / (1 - 0.999 ** t)).sqrt() + 1e-6 / math.sqrt(1 - 0.999 ** t))
                u = u + (lam if a else 0.0) * w
                xn = math.sqrt(float((u * u).sum()))
                r = pn / xn if a else 1.0
                ref[i] = w - lr * r * u
            else:
                xn = math.sqrt(float((gs * gs).sum()))
                r = 1e-2 * pn / (xn + lam * pn + 1e-9) if a else 1.0
                s1[i] = 0.9 * s1[i] + lr * r * (gs + (lam if a else 0.0) * w)
                ref[i] = w - s1[i]
            got = ap.last_layer_norms[i]
            # parameters and slots are stored in fp32 after every update: 5 updates of rounding
            assert got[0] == pytest.approx(pn, rel=2e-6) and got[1] == pytest.approx(xn, rel=1e-5)
            assert got[2] == pytest.approx(r, rel=1e-5) and (a or got[2] == 1.0)
            torch.testing.assert_close(p[b:b + n].double(), ref[i], rtol=2e-6, atol=1e-9)
            torch.testing.assert_close(ap.m[b:b + n].double(), s1[i], rtol=1e-5, atol=1e-9)  # |m| ~ 1e-3, sums cancel
    outside = torch.ones(N, dtype=torch.bool)
    for b, n, _ in segs:
        outside[b:b + n] = False
    assert outside.sum() == 5 + 15 and torch.equal(p[outside], p0[outside]) and (ap.m[outside] == 0).all()
    assert not torch.equal(p[~outside], p0[~outside])
    assert ap.powers() == {} and list(ap.slots()) == (["m", "v"] if kind == "lamb" else ["m"])


def test_a_layerwise_config_needs_the_variable_table():
    for opt in (O.LAMBOptimizer(), O.LARSOptimizer()):
        with pytest.raises(ValueError, match="segments"):
            O.FlatApplier(opt, N)
        assert O.is_layerwise(opt) and O.is_layerwise(O.SyncReplicasOptimizer(opt))
    assert not O.is_layerwise(O.AdamOptimizer())
    assert (O.LAMBOptimizer().name, O.LAMBOptimizer().epsilon, O.LAMBOptimizer().weight_decay) == ("LAMB", 1e-6, 0.0)
    d = O.LARSOptimizer()
    assert (d.name, d.momentum, d.weight_decay, d.eeta, d.epsilon, d.skip_bias) == ("LARS", 0.9, 1e-4, 1e-3, 0.0, True)
    with pytest.raises(ValueError):
        O.LAMBOptimizer(weight_decay=-1.0)
    with pytest.raises(ValueError):
        O.LARSOptimizer(eeta=0.0)


@pytest.mark.parametrize("opt", [O.AdamOptimizer(1e-2), O.MomentumOptimizer(0.1, 0.9), O.GradientDescentOptimizer(0.1)])
def test_flat_applier_with_a_plain_config_is_bit_identical(opt):
    """Today's arithmetic, spelled out; a variable table handed to a plain config changes nothing."""
    p0 = torch.randn(N, generator=torch.Generator().manual_seed(3))
    ap, p = O.FlatApplier(opt, N), p0.clone()
    ap2, p2 = O.FlatApplier(opt, N, None, _table(True)), p0.clone()
    ref, m, v = p0.clone(), torch.zeros(N), torch.zeros(N)
    for t, g in enumerate(_grads(), 1):
        ap.apply(p, g, 0.5)
        ap2.apply(p2, g, 0.5)
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
        assert torch.equal(p, ref) and torch.equal(p2, ref)
    assert ap.last_layer_norms is None and ap.segments is None and ap2.segments is None


# ---------------------------------------------------------------- sync DP over Gloo
def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 784, generator=g), torch.randint(0, 10, (n,), generator=g)


def _init():
    return M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(4).items()})


def _dp_opt(kind):
    return O.LAMBOptimizer(0.01, weight_decay=0.01) if kind == "lamb" else O.LARSOptimizer(0.5, eeta=0.02)


def _dp_worker(rank, world, steps, B, kind):
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner
    from tensorflow_distributed_amd.parallel.sync_replicas import SyncReplicasStepper, broadcast_state

    r = TorchMnistRunner(B, _dp_opt(kind), keep_prob=1.0, rank=rank)
    if rank == 0:
        r.load_flat(_init(), {}, 0)
    broadcast_state(r, 0)
    st = SyncReplicasStepper(r, rank, world, world)
    x, y = _data(B * world * steps, 11)
    ratios = []
    for s in range(steps):
        lo = (s * world + rank) * B
        st.step(x[lo:lo + B], y[lo:lo + B])
        ratios.append([v[2] for v in r.last_layer_norms().values()])
    return r.params().clone(), ratios


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_layerwise_sync_dp_equals_big_batch_single_process(kind):
    """2 Gloo ranks at B=8 == one process at B=16: the norms are those of the averaged gradient, after
    the all-reduce. Tolerances: those of test_clipped_sync_dp_equals_big_batch_single_process."""
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    world, steps, B = 2, 3, 8
    outs = run_ranks(_dp_worker, world, steps, B, kind, timeout=400)
    assert torch.equal(outs[0][0], outs[1][0]), "replicas diverged"
    assert outs[0][1] == outs[1][1]
    ref = TorchMnistRunner(B * world, _dp_opt(kind), keep_prob=1.0)
    ref.load_flat(_init(), {}, 0)
    x, y = _data(B * world * steps, 11)
    for s in range(steps):
        lo = s * world * B
        ref.train_step(x[lo:lo + world * B], y[lo:lo + world * B])
        want = [v[2] for v in ref.last_layer_norms().values()]
        assert outs[0][1][s] == pytest.approx(want, rel=1e-3)
        assert [r == 1.0 for r in want] == [False, True] * 4  # the biases are skipped
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


def test_optimizer_flags_build_the_configs():
    mk = lambda d: d._make_optimizer()  # noqa: E731
    assert _with_flags([], mk) == O.AdamOptimizer(0.01)
    assert _with_flags(["--optimizer=lamb"], mk) == O.LAMBOptimizer(0.01)
    assert _with_flags(["--optimizer=lamb", "--weight_decay=0.01", "--layerwise_skip_bias=False", "--clip_norm=5"], mk) == \
        O.LAMBOptimizer(0.01, weight_decay=0.01, skip_bias=False, clip_norm=5.0)
    assert _with_flags(["--optimizer=lars", "--momentum=0.8", "--lars_eeta=0.02", "--ema_decay=0.9"], mk) == \
        O.LARSOptimizer(0.01, 0.8, eeta=0.02, ema_decay=0.9, ema_num_updates=True)
    assert _with_flags(["--optimizer=lars"], mk).weight_decay == 1e-4
    assert _with_flags(["--optimizer=lars", "--weight_decay=0"], mk).weight_decay == 0.0
    for argv in (["--optimizer=lamb"], ["--optimizer=lars", "--dp_schedule=allreduce"], ["--sync_replicas=False"]):
        _with_flags(argv, lambda d: d.check_layerwise_flags(2))  # supported, or not layer-wise: no complaint


@pytest.mark.parametrize("opt", ["lamb", "lars"])
@pytest.mark.parametrize("argv,word", [
    (["--sync_replicas=False"], "sync_replicas"),
    (["--replicas_to_aggregate=1"], "backup workers"),
    (["--model=resnet18"], "resnet18"),
    (["--model=resnet50"], "resnet50"),
    (["--dp_schedule=sfb+zero"], "dp_schedule"),
])
def test_unsupported_layerwise_combinations_are_flag_errors(opt, argv, word):
    with pytest.raises(ValueError, match=word) as e:
        _with_flags(["--optimizer=" + opt] + argv, lambda d: d.check_layerwise_flags(2))
    assert "--optimizer=" + opt in str(e.value)


def test_other_layerwise_flag_errors():
    with pytest.raises(ValueError, match="weight_decay"):
        _with_flags(["--weight_decay=0.1"], lambda d: d.check_layerwise_flags(2))  # Adam has no way to express it
    with pytest.raises(ValueError, match="lars_eeta"):
        _with_flags(["--optimizer=lars", "--lars_eeta=0"], lambda d: d.check_layerwise_flags(2))


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
        F.FLAGS.parse(["prog", "--optimizer=lamb", "--sync_replicas=False", "--synthetic_data", "--data_dir=/nonexistent",
                       "--job_name=worker", "--task_index=0"])
        with pytest.raises(ValueError, match="sync_replicas"):
            dist_main.main()
    finally:
        F.FLAGS.reset()


@pytest.mark.parametrize("opt", ["lamb", "lars"])
def test_layerwise_restricts_gpu_schedules_to_allreduce(opt):
    from tensorflow_distributed_amd.parallel import schedule as SCH

    flag = "--optimizer=" + opt
    assert _with_flags([], lambda d: d.dp_candidates("cuda", "bf16")) == list(SCH.MNIST_SCHEDULES)
    assert _with_flags([flag], lambda d: d.dp_candidates("cuda", "bf16")) == ["allreduce"]
    assert _with_flags([flag], lambda d: d.dp_candidates("cuda", "fp32")) == ["allreduce"]
    for mode in ("fixed", "auto"):
        got = _with_flags([flag, "--dp_schedule=" + mode], lambda d: d.choose_dp_schedule(lambda name: 1.0, 0, 2, "cuda"))
        assert got[0] == "allreduce" and got[1] is None, got
    with pytest.raises(ValueError, match="allreduce"):  # a pinned sharded schedule is an error, not ignored
        _with_flags([flag, "--dp_schedule=sfb"], lambda d: d.choose_dp_schedule(lambda n: 1.0, 0, 2, "cuda"))
    assert _with_flags([flag], lambda d: d.dp_candidates("cpu", "bf16")) == list(SCH.CPU_SCHEDULES)


# ---------------------------------------------------------------- checkpoint and reporting
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_torch_runner_checkpoint_round_trip(kind):
    """Slots are saved by TF's slot-variable rule under the optimizer's name; no beta powers (t is
    global_step); a run resumed from the checkpoint is bit-identical to the uninterrupted one."""
    from tensorflow_distributed_amd.models.mnist_runner import TorchMnistRunner

    opt = O.LAMBOptimizer(0.01, weight_decay=0.01) if kind == "lamb" else O.LARSOptimizer(0.5, eeta=0.02)
    x, y = _data(5 * 4, 3)

    def runner():
        r = TorchMnistRunner(4, opt, keep_prob=1.0)
        r.load_flat(_init(), {}, 0)
        return r

    a = runner()
    for i in range(3):
        a.train_step(x[4 * i:4 * i + 4], y[4 * i:4 * i + 4])
    sd = a.state_dict_tf()
    slot_keys = sorted(k for k in sd if "/" in k)
    if kind == "lamb":
        assert slot_keys == sorted([n + s for _, n, _ in M.PARAM_SPECS for s in ("/LAMB", "/LAMB_1")])
        assert "Variable/LAMB" in sd and "Variable/LAMB_1" in sd
    else:
        assert slot_keys == sorted(n + "/LARS" for _, n, _ in M.PARAM_SPECS)
    assert "beta1_power" not in sd and "beta2_power" not in sd and int(sd["global_step"]) == 3
    assert any(abs(sd[k]).max() > 0 for k in slot_keys)
    b = runner()
    b.load_state_dict_tf(sd)
    assert b.global_step() == 3 and torch.equal(b.params(), a.params())
    for i in range(3, 5):
        a.train_step(x[4 * i:4 * i + 4], y[4 * i:4 * i + 4])
        b.train_step(x[4 * i:4 * i + 4], y[4 * i:4 * i + 4])
    assert torch.equal(a.params(), b.params()) and a.last_layer_norms() == b.last_layer_norms()
    for k, v in a.slot_tensors().items():
        assert torch.equal(v, b.slot_tensors()[k]), k
    assert list(a.last_layer_norms()) == ["wc1", "bc1", "wc2", "bc2", "wd1", "bd1", "out", "out_b"]


def test_supervisor_writes_trust_ratios(tmp_path):
    from tensorflow_distributed_amd.training import summary as S
    from tensorflow_distributed_amd.training.supervisor import Supervisor

    class Runner:
        opt = O.LAMBOptimizer(0.01)
        layerwise = True

        def global_step(self):
            return 0

        def last_layer_norms(self):
            return {"wc1": (2.0, 4.0, 0.5), "bc1": (1.0, 3.0, 1.0)}

    sv = Supervisor(True, str(tmp_path), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(7)
    sv.writer.close()
    got = {tag: v for step, tag, v in S.read_scalars(sv.writer.path) if step == 7}
    assert got["trust_ratio/wc1"] == 0.5 and got["trust_ratio/bc1"] == 1.0
    Runner.layerwise = False
    sv = Supervisor(True, str(tmp_path / "b"), Runner(), init_fn=lambda: None, save_model_secs=0, save_summaries_secs=0)
    sv.write_summary(7)
    sv.writer.close()
    assert not any(tag.startswith("trust_ratio") for _, tag, _ in S.read_scalars(sv.writer.path))


@pytest.mark.slow
def test_launcher_run_logs_trust_ratios(tmp_path):
    from tensorflow_distributed_amd import launch

    mf = tmp_path / "m.jsonl"
    r = launch.launch(1, 2, ["--train_steps=3", f"--logdir={tmp_path}", f"--metrics_file={mf}", "--optimizer=lamb",
                             "--weight_decay=0.01", "--synthetic_data", "--eval_batches=1", "--data_dir=/nonexistent"],
                      echo=False, timeout_s=300)
    assert r["ok"], r["outputs"]
    steps = [rec for rec in (json.loads(ln) for ln in open(mf)) if "step" in rec and "event" not in rec]
    assert len(steps) == 3
    for rec in steps:
        tr = rec["trust_ratio"]
        assert list(tr) == ["wc1", "bc1", "wc2", "bc2", "wd1", "bd1", "out", "out_b"]
        assert all(math.isfinite(v) and v > 0 for v in tr.values())
        assert [tr[k] == 1.0 for k in tr] == [False, True] * 4
