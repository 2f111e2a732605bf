"""How a dist_main MNIST worker synchronises gradients: one object per mode, chosen once by
:func:`make_grad_sync` from the resolved roles. The worker loop calls ``broadcast`` / ``step`` /
``describe`` / ``placement`` / ``close`` and never asks which mode it is in.

  * :class:`AllReduceSync` -- all-reduce DP with SyncReplicasOptimizer semantics
    (parallel/sync_replicas.py): N of N, the R < N all-gather stepper without a ps task, world 1.
  * :class:`HostPsSync` -- the host parameter server over Gloo (parallel/async_ps.py): Hogwild
    async, or the backup-worker accumulator (R < N with a ps task).
  * :class:`GpuPsSync` -- the same two protocols with the variables on the ps tasks' GPUs
    (parallel/gpu_ps.py).
"""
from __future__ import annotations

import time

import torch

from ..models import mnist_cnn as M
from ..parallel import async_ps, sync_replicas
from ..parallel.cluster import ps_task_of, replica_device_setter
from ..utils.flags import FLAGS


def straggler_delays() -> dict:
    """--straggler_delay 'task:seconds,...' (test hook: artificial per-step slowness)."""
    return {int(k): float(v) for k, v in (item.split(":") for item in FLAGS.straggler_delay.split(",") if item)}


class AllReduceSync:
    # PS modes overwrite the runner's step with the PS global step after every push, and the device
    # permutation is indexed by that step: each worker would see ~1/N of its epoch. Those modes keep
    # the reference's per-worker sequential next_batch (mnist_python_m.py:291) on the host instead.
    device_input = True
    # lr of the update that produced a global step, from the host's step mirror (no device read). Not
    # logged in the parameter-server modes: there every ps shard evaluates the schedule at its own
    # update count, which is not this worker's global step
    logs_lr = True
    last_dropped = False

    def __init__(self, runner, cluster, roles, group, dp_sched=None):
        self.runner, self.world, self.group, self.src = runner, cluster.num_workers, group, cluster.num_ps
        self.stepper = sync_replicas.SyncReplicasStepper(
            runner, FLAGS.task_index, self.world, roles.r2a, group=group, straggler_delay_s=straggler_delays(),
            splits=[M.BUCKET_SPLIT] if dp_sched == "buckets" else None)

    def broadcast(self, sv) -> None:
        if self.world > 1:
            sync_replicas.broadcast_state(self.runner, 0, group=self.group, group_src_rank=self.src)

    def step(self, x, y, step: int) -> int:
        self.stepper.step(x, y)
        return self.runner.global_step()

    def describe(self) -> str:
        tr = getattr(self.runner, "transport", None)
        if tr is None:
            return "Gloo all-reduce"
        return (tr.kind.replace("+sfb", "") + " all-reduce"
                + (" (fc layers: all-gathered sufficient factors)" if "+sfb" in tr.kind else ""))

    def placement(self, cluster, names, worker_device: str) -> dict:
        return {n: worker_device + " (replicated)" for n in names}

    def close(self) -> None:
        pass


class _PsSync:
    """What the two parameter-server modes share: the client's life, the restored optimizer moments
    for the chief's ``init``, where the variables are placed, what a dropped gradient means."""
    device_input = False
    logs_lr = False

    def __init__(self, runner, cluster, roles, client):
        self.runner, self.client, self.roles, self.world = runner, client, roles, cluster.num_workers
        self.delay = straggler_delays().get(FLAGS.task_index)
        runner.ps_client = client  # the chief's checkpoints read the PS-resident state (params + slots)

    def _restored_slots(self, sv):
        """Restored moments go back to the PS as host tensors (fresh init: None, the PS starts at zero)."""
        if not sv.restored_from:
            return None
        # the runners call Momentum's / LARS's slot "accum", FlatApplier keeps it in "m"; Adagrad's is "accum" in both
        names = set(getattr(self.client, "slot_names", ()))
        return {("m" if k == "accum" and "accum" not in names else k): v.detach().float().cpu()
                for k, v in self.runner.slot_tensors().items()}

    def _straggle(self) -> None:
        if self.delay is not None:
            time.sleep(self.delay)  # test hook: a straggling worker

    @property
    def last_dropped(self) -> bool:
        """Backup workers: a faster replica finished this step first and the PS dropped our gradient."""
        return self.roles.backup_ps and self.client.last_dropped

    def describe(self) -> str:
        if self.roles.backup_ps:
            return "PS accumulator (%d of %d replicas)" % (self.roles.r2a, self.world)
        return self.async_text

    def placement(self, cluster, names, worker_device: str) -> dict:
        return replica_device_setter(cluster, names, worker_device)

    def close(self) -> None:
        self.client.stop()


class HostPsSync(_PsSync):
    async_text = "async PS push/pull"
    grad_cpu = None  # the gradient's host buffer, reused by every step

    def broadcast(self, sv) -> None:
        r = self.runner
        flat = r.params().detach().float().cpu()
        if sv.is_chief:  # t = global_step
            self.client.init(flat, step=r.global_step(), t=r.global_step(), slots=self._restored_slots(sv))
        gs = self.client.pull(flat)
        r.set_params(flat)
        r.set_global_step(gs)

    def step(self, x, y, step: int) -> int:
        r = self.runner
        g, _ = r.compute_grads(x, y)
        if self.grad_cpu is None:
            self.grad_cpu = torch.zeros(M.TOTAL)
        self.grad_cpu.copy_(g.detach().float().cpu())
        self._straggle()
        flat = r.params().detach().float().cpu()
        # sync: the gradient is tagged with the global step it was computed at (stale ones are
        # dropped by the PS accumulator); async: applied as it comes
        step = self.client.push_pull(flat, self.grad_cpu, local_step=step)
        r.set_params(flat)
        r.set_global_step(step)
        return step


class GpuPsSync(_PsSync):
    async_text = "GPU ps mailbox push / peer-memory pull"

    def broadcast(self, sv) -> None:
        r = self.runner
        if sv.is_chief:
            # the ps tasks read the initial / restored values from the chief's engine (peer memory)
            self.client.init(step=r.global_step(), t=r.global_step(), slots=self._restored_slots(sv))
        r.set_global_step(self.client.pull())

    def step(self, x, y, step: int) -> int:
        g, _ = self.runner.compute_grads(x, y, with_loss=False)
        self._straggle()
        # the gradient goes GPU -> the ps tasks' GPU mailboxes, the fresh values come back into the
        # engine's parameters; only the 32-byte control messages touch the host
        step = self.client.push_pull(g, local_step=step)
        self.runner.set_global_step(step)
        return step

    def placement(self, cluster, names, worker_device: str) -> dict:
        # each ps task's shard lives on its GPU (task % num_gpus), not on the reference's ps cpu
        placed = super().placement(cluster, names, worker_device)
        return {n: "/job:ps/task:%d/gpu:%d" % (ps_task_of(placed, n), ps_task_of(placed, n) % FLAGS.num_gpus)
                for n in names}


def make_grad_sync(runner, cluster, roles, layout, opt, group, dp_sched=None):
    """The one place that turns the resolved roles into a mode."""
    if not roles.ps_mode:
        return AllReduceSync(runner, cluster, roles, group, dp_sched)
    from .optimizers import FlatApplier

    slots = list(FlatApplier(opt, 0).slots())
    if not roles.use_gpu_ps:
        return HostPsSync(runner, cluster, roles, async_ps.AsyncPSClient(FLAGS.task_index, layout, slot_names=slots))
    from ..parallel import gpu_ps

    return GpuPsSync(runner, cluster, roles, gpu_ps.GpuPSClient(FLAGS.task_index, layout, runner.params(),
                                                                runner.sync_shadow, slot_names=slots))
