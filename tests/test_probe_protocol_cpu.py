"""The schedule probe's collective protocol (parallel/schedule.timed_probe) over Gloo, world 3: a
failure in any section on one rank is raised on every rank and the ranks' collective sequences stay
matched; and the gradient-sync objects' --log_device_placement texts (training/grad_sync.py)."""
import math
from types import SimpleNamespace

import pytest

from dist_util import run_ranks

WORLD = 3


def _probe_rank(rank, world, fail_in):
    import torch
    import torch.distributed as dist

    from tensorflow_distributed_amd.parallel.schedule import timed_probe

    calls = {"setup": 0, "warmup": 0, "timed": 0, "teardown": 0, "max": 0, "max_before_timed": None}

    def section(name, value=None):
        def run():
            calls[name] += 1
            if name == "timed":
                calls["max_before_timed"] = calls["max"]
            if rank == 1 and name == fail_in:
                raise ValueError("injected in " + name)
            return value
        return run

    def max_over(v):
        calls["max"] += 1
        t = torch.tensor([float(v)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    ms, raised = None, None
    try:
        ms = timed_probe(section("setup"), section("warmup"), section("timed", 1.5 + rank), section("teardown"),
                         max_over_ranks=max_over, barrier=dist.barrier, what="schedule probe x")
    except RuntimeError as e:
        raised = str(e)
    ids = torch.ones(1, dtype=torch.int64)  # the next collective of every rank meets its peers'
    dist.all_reduce(ids)
    return {"ms": ms, "raised": raised, "calls": calls, "sum": int(ids.item())}


@pytest.mark.parametrize("fail_in", ["setup", "warmup", "timed"])
def test_probe_failure_on_one_rank_is_raised_on_every_rank(fail_in):
    res = run_ranks(_probe_rank, WORLD, fail_in, timeout=60)
    for rank, r in enumerate(res):
        assert r["raised"] is not None and fail_in in r["raised"], (rank, r)
        assert ("injected in " + fail_in in r["raised"]) == (rank == 1), (rank, r)
        c = r["calls"]
        assert c["teardown"] <= 1, (rank, c)
        if not (fail_in == "setup" and rank == 1):  # this rank's setup succeeded
            assert c["teardown"] == 1, (rank, c)
        assert c["warmup"] == (0 if fail_in == "setup" else 1) and c["timed"] == (1 if fail_in == "timed" else 0), c
        assert r["sum"] == WORLD, (rank, r)
    assert len({r["calls"]["max"] for r in res}) == 1, res  # same number of agreements on every rank


def test_probe_success_path():
    res = run_ranks(_probe_rank, WORLD, None, timeout=60)
    for rank, r in enumerate(res):
        assert r["raised"] is None and r["ms"] == 1.5 + rank and math.isfinite(r["ms"]) and r["ms"] > 0, (rank, r)
        c = r["calls"]
        assert (c["setup"], c["warmup"], c["timed"], c["teardown"]) == (1, 1, 1, 1), (rank, c)
        # setup agreement + warm-up agreement before the timed section, the timed agreement after it
        assert c["max_before_timed"] == 2 and c["max"] == 3, (rank, c)
        assert r["sum"] == WORLD, (rank, r)


class _Runner:
    """What a gradient-sync object touches at construction."""

    def __init__(self, transport_kind=None):
        self.transport = SimpleNamespace(kind=transport_kind) if transport_kind else None
        self.comm = None
        self.eng = object()  # a native runner: the stepper installs no Gloo reducer
        self.sync_shadow = None

    def params(self):
        return None


def _sync_object(monkeypatch, *, sync=True, r2a=2, backup_ps=False, gpu_ps=False, transport_kind=None, num_ps=1):
    from tensorflow_distributed_amd.parallel import async_ps
    from tensorflow_distributed_amd.parallel.cluster import ClusterSpec
    from tensorflow_distributed_amd.training import dist_main, grad_sync, optimizers

    dist_main.define_flags(0, "worker")
    dist_main.FLAGS.parse(["prog", "--num_gpus=2"])
    cluster = ClusterSpec({"ps": ["h:%d" % (1 + i) for i in range(num_ps)], "worker": ["h:10", "h:11"]})
    roles = dist_main.Roles(sync, r2a, backup_ps, (not sync) or backup_ps, gpu_ps)
    if gpu_ps:  # the client would open the ps tasks' GPU mailboxes
        from tensorflow_distributed_amd.parallel import gpu_ps as gpu_ps_mod

        monkeypatch.setattr(gpu_ps_mod, "GpuPSClient", lambda *a, **k: SimpleNamespace(last_dropped=False))
    return grad_sync.make_grad_sync(_Runner(transport_kind), cluster, roles, async_ps.mnist_layout(num_ps),
                                    optimizers.AdamOptimizer(0.01), None), cluster


NAMES = ["global_step", "Variable", "Variable_1", "Variable_2"]
WDEV = "/job:worker/task:0/gpu:0"


def test_describe_and_placement_gloo_all_reduce(monkeypatch):
    from tensorflow_distributed_amd.training.grad_sync import AllReduceSync

    s, cluster = _sync_object(monkeypatch)
    assert type(s) is AllReduceSync and s.logs_lr and s.device_input and not s.last_dropped
    assert s.describe() == "Gloo all-reduce"
    assert s.placement(cluster, NAMES, "/job:worker/task:0/cpu:0") == {
        n: "/job:worker/task:0/cpu:0 (replicated)" for n in NAMES}
    s, _ = _sync_object(monkeypatch, transport_kind="rccl+ipc+sfb")
    assert s.describe() == "rccl+ipc all-reduce (fc layers: all-gathered sufficient factors)"
    s, _ = _sync_object(monkeypatch, transport_kind="ipc")
    assert s.describe() == "ipc all-reduce"


def test_describe_and_placement_host_async_ps(monkeypatch):
    from tensorflow_distributed_amd.training.grad_sync import HostPsSync

    s, cluster = _sync_object(monkeypatch, sync=False, num_ps=2)
    assert type(s) is HostPsSync and not s.logs_lr and not s.device_input and not s.last_dropped
    assert s.runner.ps_client is s.client
    assert s.describe() == "async PS push/pull"
    assert s.placement(cluster, NAMES, WDEV) == {
        "global_step": "/job:ps/task:0/cpu:0", "Variable": "/job:ps/task:1/cpu:0",
        "Variable_1": "/job:ps/task:0/cpu:0", "Variable_2": "/job:ps/task:1/cpu:0"}


def test_describe_ps_accumulator(monkeypatch):
    s, _ = _sync_object(monkeypatch, r2a=1, backup_ps=True)
    assert s.describe() == "PS accumulator (1 of 2 replicas)"
    s.client.last_dropped = True
    assert s.last_dropped
    s, _ = _sync_object(monkeypatch, sync=False)
    s.client.last_dropped = True  # only the accumulator drops stale gradients
    assert not s.last_dropped


def test_describe_and_placement_gpu_ps(monkeypatch):
    from tensorflow_distributed_amd.training.grad_sync import GpuPsSync

    s, cluster = _sync_object(monkeypatch, sync=False, gpu_ps=True, num_ps=3)
    assert type(s) is GpuPsSync and not s.logs_lr and not s.device_input
    assert s.describe() == "GPU ps mailbox push / peer-memory pull"
    # each ps task's shard on GPU task % --num_gpus (2)
    assert s.placement(cluster, NAMES, WDEV) == {
        "global_step": "/job:ps/task:0/gpu:0", "Variable": "/job:ps/task:1/gpu:1",
        "Variable_1": "/job:ps/task:2/gpu:0", "Variable_2": "/job:ps/task:0/gpu:0"}
    s, _ = _sync_object(monkeypatch, r2a=1, backup_ps=True, gpu_ps=True)
    assert s.describe() == "PS accumulator (1 of 2 replicas)"
