"""Device runners for the reference MNIST CNN: what ``sess.run(train_step)`` executes.

* :class:`NativeMnistRunner` (GPU): the C++ ``MnistEngine`` (``csrc/runtime/mnist_engine.cpp``) --
  fused HIP/MFMA forward+backward, bucketed RCCL gradient all-reduce overlapped with the conv
  backward, fused flat optimizer, optional hipGraph replay. This is the only GPU path; it fails
  loudly if the native library is missing.
* :class:`TorchMnistRunner` (CPU, the reference's default ``--num_gpus=0`` worker device,
  ``/root/reference/mnist_python_m.py:169-172``): fp32 PyTorch ops + autograd + the same optimizer
  equations (:class:`training.optimizers.FlatApplier`), gradients averaged over Gloo.

Both keep the parameters in the flat layout of ``csrc/mnist_layout.h`` so checkpoints, broadcasts
and the async parameter-server protocol are layout-identical across devices.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..training.optimizers import (FlatApplier, base_optimizer, ema_decay_at, is_layerwise, is_schedule, lr_at,
                                   schedule_args)
from ..training import inference
from . import mnist_cnn as M


EMA_SUFFIX = "/ExponentialMovingAverage"  # tf.train.ExponentialMovingAverage's shadow-variable name
LAYER_NAMES = tuple(M.OFFSETS)  # the variables in flat-layout order: the rows of last_layer_norms()


def _slot_suffixes(opt):
    """``[(checkpoint suffix, slot)]`` by TF's slot-variable rule: a slot is saved as
    ``<var>/<optimizer name>``, a second one as ``<var>/<optimizer name>_1``."""
    kind = getattr(opt, "kind", "adam")
    if kind == "lamb":
        return [("/" + opt.name, "m"), ("/" + opt.name + "_1", "v")]
    if kind == "lars":
        return [("/" + opt.name, "accum")]
    if kind == "rmsprop":
        # TF creates the slots in the order rms, mg (centered only), momentum
        names = ["ms", "mg", "mom"] if opt.centered else ["ms", "mom"]
        return [("/" + opt.name + ("_%d" % i if i else ""), n) for i, n in enumerate(names)]
    if kind == "adagrad":
        return [("/" + opt.name, "accum")]
    return [("/Adam", "m"), ("/Adam_1", "v"), ("/Momentum", "accum")]


def _labels_to_ids(y) -> torch.Tensor:
    y = torch.as_tensor(np.asarray(y)) if not isinstance(y, torch.Tensor) else y
    if y.dim() == 2:
        y = y.argmax(1)
    return y.to(torch.int32)


def _as_f32(x) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    return x.reshape(x.shape[0], -1).to(torch.float32)


def _as_rows(x) -> torch.Tensor:
    """``_as_f32`` that also takes no rows at all ([0, ...] has no width to infer)."""
    x = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    return _as_f32(x) if x.numel() else torch.zeros(0, 784, dtype=torch.float32)


def _check_eval_split(images, labels):
    x, y = _as_rows(images), _labels_to_ids(labels)
    if x.dim() != 2 or x.shape[1] != 784 or y.dim() != 1 or y.shape[0] != x.shape[0]:
        raise ValueError(f"set_eval_dataset: images [N,784] and labels [N], got {tuple(x.shape)} and {tuple(y.shape)}")
    if y.numel() and (int(y.min()) < 0 or int(y.max()) >= M.NCLS):
        raise ValueError(f"set_eval_dataset: labels must be in [0, {M.NCLS}), got [{int(y.min())}, {int(y.max())}]")
    return x.contiguous(), y.contiguous()


def _eval_range(split, first, count, group):
    if split is None:
        raise ValueError("evaluate_dataset: set_eval_dataset first")
    n = split.shape[0]
    first = int(first)
    count = n - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > n:
        raise ValueError(f"evaluate_dataset: rows [{first}, {first + count}) outside the evaluation split of {n} rows")
    group = max(count, 1) if group is None else int(group)
    if group < 1:
        raise ValueError(f"evaluate_dataset: group >= 1, got {group}")
    return first, count, group


class MnistRunnerBase:
    batch_size: int
    device: torch.device

    def current_lr(self) -> float:
        """Learning rate of the NEXT update, from the host's mirror of global_step (no device read)."""
        step = getattr(self, "_hstep", None)
        if step is None:
            step = self.global_step()
        return lr_at(self.opt.learning_rate, step)

    # -- moving average of the weights (ema_decay on the optimizer config) --
    @property
    def ema_on(self) -> bool:
        return bool(getattr(getattr(self, "opt", None), "ema_decay", None))

    def current_ema_decay(self) -> float:
        """``d_t`` of the LAST update, from the host's mirror of global_step (no device read)."""
        step = getattr(self, "_hstep", None)
        if step is None:
            step = self.global_step()
        return ema_decay_at(self.opt.ema_decay, step, self.opt.ema_num_updates)

    # -- layer-wise optimizers (LAMB, LARS) --
    @property
    def layerwise(self) -> bool:
        return is_layerwise(getattr(self, "opt", None))

    def last_layer_norms(self) -> "dict":
        """``{variable: (|p|, |u| or |g|, trust ratio)}`` of the last update, in flat-layout order; empty
        without a layer-wise optimizer or before the first update."""
        return {}

    def ema_params(self) -> torch.Tensor: ...
    def load_ema(self, flat: torch.Tensor) -> None: ...
    def reset_ema(self) -> None: ...

    # -- state (flat layout) --
    def params(self) -> torch.Tensor: ...
    def global_step(self) -> int: ...

    ps_client = None  # parallel.async_ps.AsyncPSClient when the variables live on PS tasks

    def state_dict_tf(self) -> "dict":
        """TF-named tensors for the checkpoint (mnist_python_m.py:178,185-196 creation order).
        With the variables on parameter servers (async / backup-worker modes) the values AND the
        optimizer slots are pulled from the PS tasks -- what TF's Saver would save."""
        from collections import OrderedDict

        flat = self.params().detach().float().cpu().clone()
        step = self.global_step()
        slot_t = {k: v.detach().float().cpu() for k, v in self.slot_tensors().items()}
        powers = self.powers()
        if self.ps_client is not None:
            got, t, step = self.ps_client.pull_state(flat)
            kind = getattr(getattr(self, "opt", None), "kind", "adam")
            slot_t = {("accum" if kind == "momentum" else k): v for k, v in got.items()}
            o = self.opt
            powers = {"beta1_power": o.beta1 ** t, "beta2_power": o.beta2 ** t} if kind == "adam" else {}
        out = OrderedDict()
        out["global_step"] = np.array(step, dtype=np.int64)
        views = M.dict_from_flat(flat)
        slots = {k: M.dict_from_flat(v) for k, v in slot_t.items()}
        # the Saver writes the shadow variables beside the variables they average
        ema = M.dict_from_flat(self.ema_params().detach().float().cpu().clone()) if self.ema_on else None
        for key, tf_name, _ in M.PARAM_SPECS:
            out[tf_name] = views[key].numpy().copy()
            if ema is not None:
                out[tf_name + EMA_SUFFIX] = ema[key].numpy().copy()
            for suffix, slot in _slot_suffixes(getattr(self, "opt", None)):
                if slot in slots:
                    out[tf_name + suffix] = slots[slot][key].numpy().copy()
        for k, v in powers.items():
            out[k] = np.array(v, dtype=np.float32)
        return out

    def load_state_dict_tf(self, tensors) -> None:
        flat = torch.zeros(M.TOTAL)
        views = M.dict_from_flat(flat)
        slots = {}
        for key, tf_name, _ in M.PARAM_SPECS:
            views[key].copy_(torch.from_numpy(np.asarray(tensors[tf_name])))
            for suffix, slot in _slot_suffixes(getattr(self, "opt", None)):
                if tf_name + suffix in tensors:
                    sflat = slots.setdefault(slot, torch.zeros(M.TOTAL))
                    M.dict_from_flat(sflat)[key].copy_(torch.from_numpy(np.asarray(tensors[tf_name + suffix])))
        step = int(np.asarray(tensors.get("global_step", 0)))
        self.load_flat(flat, slots, step)  # (restarts the averages from the restored values)
        # the averages, when the checkpoint carries all of them; with EMA off they are ignored
        if self.ema_on and all(tf_name + EMA_SUFFIX in tensors for _, tf_name, _ in M.PARAM_SPECS):
            eflat = torch.zeros(M.TOTAL)
            eviews = M.dict_from_flat(eflat)
            for key, tf_name, _ in M.PARAM_SPECS:
                eviews[key].copy_(torch.from_numpy(np.asarray(tensors[tf_name + EMA_SUFFIX])))
            self.load_ema(eflat)

    def slot_tensors(self) -> "dict":
        return {}

    def powers(self) -> "dict":
        return {}

    # -- step log: one record per optimizer step (set_step_log / train_steps / read_step_log) --
    STEP_LOG_KEYS = ("step", "loss", "correct", "rows", "lr", "grad_norm", "clip_scale", "ok")

    @staticmethod
    def _check_log_range(first_t: int, last_t: int, capacity: int) -> None:
        if capacity <= 0:
            raise ValueError("read_step_log: the step log is off; set_step_log() first")
        if first_t < 1 or last_t < first_t:
            raise ValueError("read_step_log: need 1 <= first_t <= last_t, got %d..%d" % (first_t, last_t))
        if last_t - first_t + 1 > capacity:
            raise ValueError("read_step_log: steps %d..%d are more than the log's capacity %d" % (first_t, last_t, capacity))

    def load_flat(self, flat: torch.Tensor, slots: "dict", step: int) -> None: ...


class TorchMnistRunner(MnistRunnerBase):
    """fp32 PyTorch implementation (CPU workers, the reference's default device)."""

    def __init__(self, batch_size: int, optimizer, keep_prob: float = 0.75, seed: int = 0, rank: int = 0,
                 device: Optional[torch.device] = None):
        self.batch_size = batch_size
        self.device = device or torch.device("cpu")
        self.keep_prob = keep_prob
        self.opt = base_optimizer(optimizer)
        self.accum_steps = int(getattr(self.opt, "accum_steps", 1))  # micro-batches of batch_size per update
        self.flat = torch.zeros(M.TOTAL, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros_like(self.flat)
        segs = M.segments(self.opt.skip_bias) if is_layerwise(self.opt) else None
        self.applier = FlatApplier(self.opt, M.TOTAL, self.device, segs)
        self._step = 0
        self.gen = torch.Generator(device=self.device).manual_seed(seed * 7919 + rank)
        self.comm = None  # DP reducer: callable(flat_grad) -> None (in-place average)
        self._log_cap = 0   # step log (set_step_log): capacity, 0 = off
        self._log = {}      # slot -> record
        self._log_sums = []  # (loss sum, correct, rows) of the current step's micro-batches

    def params(self) -> torch.Tensor:
        return self.flat

    def global_step(self) -> int:
        return self._step

    def set_global_step(self, s: int) -> None:
        self._step = int(s)

    def load_flat(self, flat, slots, step):
        self.flat.copy_(flat.to(self.device))
        for name, t in slots.items():
            # Momentum's / LARS's "accum" is FlatApplier's m; Adagrad's is its accum
            dst = getattr(self.applier, name, None)
            if dst is None:
                dst = getattr(self.applier, {"accum": "m"}.get(name, name), None)
            if dst is not None and (name in ("ms", "mom", "mg") or (name == "accum" and self.opt.kind == "adagrad")):
                # the padding behind the variables is in no checkpoint: it keeps its initial value (a zero
                # accumulator there would divide 0 by 0)
                dst[:M.NUM_PARAMS].copy_(t.to(self.device)[:M.NUM_PARAMS])
            elif dst is not None:
                dst.copy_(t.to(self.device))
        self.applier.t = int(step)
        self._step = int(step)
        self.reset_ema()

    def ema_params(self) -> torch.Tensor:
        assert self.ema_on, "ema_params: the optimizer config has no ema_decay"
        if self.applier.ema is None:
            self.applier.reset_ema(self.flat)
        return self.applier.ema

    def load_ema(self, flat) -> None:
        self.applier.load_ema(flat.to(self.device))

    def reset_ema(self) -> None:
        self.applier.reset_ema(self.flat)

    def slot_tensors(self):
        s = self.applier.slots()
        if self.opt.kind in ("momentum", "lars"):
            return {"accum": s["m"]}
        return s

    def last_layer_norms(self):
        n = self.applier.last_layer_norms
        return dict(zip(LAYER_NAMES, (tuple(float(x) for x in row) for row in n))) if n else {}

    def powers(self):
        return self.applier.powers()

    def set_params(self, flat: torch.Tensor) -> None:
        self.flat.copy_(flat.to(self.device))
        self.reset_ema()

    def _forward(self, x, keep_prob, mask=None, flat=None):
        p = M.dict_from_flat(self.flat if flat is None else flat)
        return M.conv_net(x, p, keep_prob, dropout_mask=mask)

    def compute_grads(self, x, y) -> Tuple[torch.Tensor, float]:
        x = _as_f32(x).to(self.device)
        y = _labels_to_ids(y).to(self.device)
        self.flat.requires_grad_(True)
        mask = (torch.rand(x.shape[0], M.HID, generator=self.gen, device=self.device) < self.keep_prob).float() \
            if self.keep_prob < 1.0 else None
        logits = self._forward(x, self.keep_prob, mask)
        loss = F.cross_entropy(logits, y.long())
        g, = torch.autograd.grad(loss, self.flat)
        self.flat.requires_grad_(False)
        self.grad.copy_(g)
        self._last_loss = float(loss.item())
        if self._log_cap:  # this micro-batch's share of the step's record
            self._log_sums.append((self._last_loss * x.shape[0], int((logits.detach().argmax(1) == y.long()).sum().item()),
                                   int(x.shape[0])))
        return self.grad, self._last_loss

    def apply_grads(self, grad: torch.Tensor, scale: float = 1.0) -> None:
        self.applier.apply(self.flat, grad, scale)
        self._step += 1

    def train_step(self, x, y) -> None:
        """One update from ``accum_steps * batch_size`` rows: the micro-batches' gradients, each with its
        own dropout mask drawn in order, are summed in fp32 as the device sums them, reduced once and
        applied once at scale ``1 / accum_steps``. The loss is the last micro-batch's."""
        K, B = self.accum_steps, self.batch_size
        self._log_sums = []
        if K == 1:
            g, _ = self.compute_grads(x, y)
            if self.comm is not None:
                self.comm(g)
            self.apply_grads(g)
            self._log_step()
            return
        x, y = _as_f32(x), _labels_to_ids(y)
        assert x.shape[0] == K * B, f"{x.shape[0]} rows != accum_steps {K} x batch {B}"
        acc = None
        for j in range(K):
            g, _ = self.compute_grads(x[j * B:(j + 1) * B], y[j * B:(j + 1) * B])
            acc = g.clone() if acc is None else acc.add_(g)
        self.grad.copy_(acc)
        if self.comm is not None:
            self.comm(self.grad)
        self.apply_grads(self.grad, 1.0 / K)
        self._log_step()

    # ---- step log: the device runner's three methods over a plain Python ring ----
    def set_step_log(self, capacity: int = 1024) -> None:
        """Keep one record per ``train_step`` -- what the device step log keeps (csrc/step_log.h) -- in a
        ring of ``capacity`` slots; 0 turns it off."""
        if capacity < 0:
            raise ValueError("set_step_log: capacity >= 0 (0 = off)")
        self._log_cap, self._log, self._log_sums = int(capacity), {}, []

    def _log_step(self) -> None:
        if not self._log_cap:
            return
        t = self._step
        rows = sum(r for _, _, r in self._log_sums)
        norm, scale = self.last_grad_norm()
        self._log[(t - 1) % self._log_cap] = dict(
            step=t, loss=sum(l for l, _, _ in self._log_sums) / rows, correct=sum(c for _, c, _ in self._log_sums),
            rows=rows, lr=float(lr_at(self.opt.learning_rate, t - 1)), grad_norm=norm, clip_scale=scale,
            ok=self.last_step_ok())

    def train_steps(self, n: int, next_batch=None) -> None:
        """``n`` optimizer steps; ``next_batch()`` -> ``(x, y)`` supplies each step's ``accum_steps *
        batch_size`` rows (this runner has no device-resident split)."""
        if next_batch is None:
            raise ValueError("train_steps: the CPU runner is fed from the host; pass next_batch")
        if n < 1:
            raise ValueError("train_steps: n >= 1")
        for _ in range(n):
            self.train_step(*next_batch())

    def read_step_log(self, first_t: int, last_t: int) -> list:
        """The records of steps ``first_t..last_t``; ``ValueError`` when the range exceeds the capacity or a
        slot holds another step (overwritten or never written)."""
        self._check_log_range(first_t, last_t, self._log_cap)
        out = []
        for t in range(first_t, last_t + 1):
            rec = self._log.get((t - 1) % self._log_cap)
            if rec is None or rec["step"] != t:
                raise ValueError("read_step_log: step %d is not in the log (slot holds %s)"
                                 % (t, "nothing" if rec is None else "step %d" % rec["step"]))
            out.append(dict(rec))
        return out

    def last_loss(self) -> float:
        return float(getattr(self, "_last_loss", float("nan")))

    def last_grad_norm(self) -> Tuple[float, float]:
        """``(norm, clip scale)`` of the last step's averaged gradient (``clip_norm`` set; the flat
        applier clips after the all-reduce), else ``(nan, 1.0)``."""
        a = self.applier
        if a.last_grad_norm is None:
            return float("nan"), 1.0
        return float(a.last_grad_norm), float(a.last_clip_scale if a.last_clip_scale is not None else 1.0)

    def skipped_steps(self) -> int:
        """Steps the non-finite guard skipped so far (``skip_nonfinite`` on the config; a statistic, not
        checkpointed)."""
        return int(self.applier.skipped_steps)

    def last_step_ok(self) -> bool:
        return bool(self.applier.last_step_ok)

    def set_phase_timing(self, on: bool = True) -> None:
        pass

    def sync_state(self) -> None:
        pass  # never sharded

    def phase_times(self) -> dict:
        """CPU path: host time of the last Gloo gradient all-reduce (the only timed phase)."""
        ms = getattr(self.comm, "last_ms", None)
        return {"allreduce_ms": round(ms, 4)} if ms is not None else {}

    @torch.no_grad()
    def evaluate(self, x, y, use_ema: bool = False) -> Tuple[float, int]:
        """``use_ema``: the forward reads the moving averages in place of the parameters."""
        x = _as_f32(x).to(self.device)
        y = _labels_to_ids(y).to(self.device).long()
        logits = self._forward(x, 1.0, flat=self.ema_params() if use_ema else None)
        loss = F.cross_entropy(logits, y, reduction="sum").item()
        return float(loss), int((logits.argmax(1) == y).sum().item())

    # ---- inference (training/inference.py holds the definitions) ----
    _PREDICT_CHUNK = 1000  # rows per forward: bounds the activations of a whole split

    @torch.no_grad()
    def predict(self, x, use_ema: bool = False):
        """``(logits [n,10] fp32, classes [n] int32)``: the forward without dropout; a row's class is the
        first maximum of its logits. ``use_ema``: the moving averages in place of the parameters."""
        x = _as_rows(x).to(self.device)
        flat = self.ema_params() if use_ema else None
        parts = [self._forward(x[o:o + self._PREDICT_CHUNK], 1.0, flat=flat)
                 for o in range(0, x.shape[0], self._PREDICT_CHUNK)]
        logits = torch.cat(parts) if parts else torch.zeros(0, M.NCLS, device=self.device)
        # numpy's argmax returns the first maximum; torch's makes no promise about ties
        classes = torch.from_numpy(logits.cpu().numpy().argmax(1).astype(np.int32)) if len(parts) else \
            torch.zeros(0, dtype=torch.int32)
        return logits, classes.to(self.device)

    def set_eval_dataset(self, images, labels) -> None:
        """Keep an evaluation split for ``evaluate_dataset``; labels outside [0, 10) are refused."""
        self._eval_x, self._eval_y = _check_eval_split(images, labels)

    def evaluate_dataset(self, first: int = 0, count: Optional[int] = None, group: Optional[int] = None,
                         use_ema: bool = False) -> list:
        """Records ``{loss_sum, rows, correct, confusion}`` of rows ``[first, first + count)`` of the
        evaluation split, one per group of ``group`` rows (default: all of them in one group)."""
        first, count, group = _eval_range(getattr(self, "_eval_x", None), first, count, group)
        out = []
        for g0 in range(first, first + count, group):
            g1 = min(g0 + group, first + count)
            logits, _ = self.predict(self._eval_x[g0:g1], use_ema)
            out.append(inference.eval_record(logits.cpu().numpy(), self._eval_y[g0:g1].numpy()))
        return out


class NativeMnistRunner(MnistRunnerBase):
    """GPU runner over the native MnistEngine (HIP kernels + RCCL + hipGraph)."""

    def __init__(self, batch_size: int, optimizer, keep_prob: float = 0.75, seed: int = 0, rank: int = 0,
                 device: Optional[torch.device] = None, comm=None, bf16_grads: bool = True, use_graph: bool = True,
                 dtype: str = "bf16"):
        from .. import _native

        _native.require()
        self.batch_size = batch_size
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.keep_prob = keep_prob
        self.opt = base_optimizer(optimizer)
        self.eng = torch.classes.tfd.MnistEngine(batch_size, self.device.index, keep_prob, seed, rank)
        self.eng.set_dtype(dtype)  # "bf16" MFMA operands, or "fp32" (the reference's precision)
        o = self.opt
        lr0 = lr_at(o.learning_rate, 0)
        if o.kind == "adam":
            self.eng.set_adam(lr0, o.beta1, o.beta2, o.epsilon)
        elif o.kind == "lamb":
            # per-variable norms and trust ratios formed on the device inside the step (csrc/layerwise.h)
            self.eng.set_lamb(lr0, o.beta1, o.beta2, o.epsilon, o.weight_decay, bool(o.skip_bias))
        elif o.kind == "lars":
            self.eng.set_lars(lr0, o.momentum, o.weight_decay, o.eeta, o.epsilon, bool(o.skip_bias))
        elif o.kind == "momentum":
            self.eng.set_momentum(lr0, o.momentum, o.use_nesterov)
        elif o.kind == "rmsprop":
            # one flat kernel per update (csrc/kernels/optim_rules.hip); the setter fills the slots with TF's
            # initial values on the current stream, which the runner's own stream must not overtake
            self.eng.set_rmsprop(lr0, o.decay, o.momentum, o.epsilon, bool(o.centered))
            torch.cuda.current_stream(self.device).synchronize()
        elif o.kind == "adagrad":
            self.eng.set_adagrad(lr0, o.initial_accumulator_value)
            torch.cuda.current_stream(self.device).synchronize()
        elif o.kind != "sgd":
            raise ValueError(f"NativeMnistRunner: no native rule for optimizer kind {o.kind!r}")
        else:
            self.eng.set_momentum(lr0, 0.0, False)
        if is_schedule(o.learning_rate):
            # evaluated by the optimizer kernels from the device global_step (csrc/lr_schedule.h)
            self.eng.set_lr_schedule(*schedule_args(o.learning_rate))
        if getattr(o, "clip_norm", None):
            # norm and clip factor taken on the device inside the step graph (csrc/kernels/grad_norm.hip)
            self.eng.set_clip_norm(float(o.clip_norm))
        if getattr(o, "skip_nonfinite", False):
            # decided on the device inside the step graph; the optimizer kernels store nothing on a skipped
            # step (csrc/kernels/grad_guard.hip, optim_guard.hip)
            self.eng.set_skip_nonfinite(True)
        self.comm = comm
        if comm is not None:
            self.eng.set_comm(comm, bf16_grads)
        self.stream = torch.cuda.Stream(self.device)
        if self.ema_on:
            # the optimizer kernels update the shadow themselves from p' in registers (csrc/ema.h)
            with torch.cuda.stream(self.stream):
                self.eng.set_ema(float(o.ema_decay), bool(o.ema_num_updates))
        # gradient accumulation: one train_step is accum_steps micro-batches of batch_size rows, summed on
        # the device (csrc/kernels/grad_accum.hip); the engine's micro counter is accum_steps * global_step
        # at every step boundary, which is all the host needs to mirror it
        self.accum_steps = int(getattr(o, "accum_steps", 1))
        if self.accum_steps > 1:
            with torch.cuda.stream(self.stream):
                self.eng.set_grad_accum(self.accum_steps)
        self.use_graph = use_graph
        self._graph_ready = False
        self._grads_graph = False
        self._multi_ready = set()  # lengths n whose n-step graph "train<n>" is captured (train_steps)
        self._x_stage = torch.empty(self.accum_steps * batch_size, 784, dtype=torch.float32).pin_memory()
        self._y_stage = torch.empty(self.accum_steps * batch_size, dtype=torch.int32).pin_memory()
        self.transport = None  # parallel.transport.DPTransport when DP runs over RCCL/IPC
        self._dev_data = None  # device-resident split (set_device_dataset)
        self._hstep = 0        # host mirror of the device global_step (epoch bookkeeping, no sync)
        self._epoch = -1

    # ---- observability ----
    PHASES = ("fwd_ms", "bwd_fc_ms", "bwd_conv_ms", "optim_ms", "allreduce_ms", "comm_wait_ms", "step_ms_gpu")

    def set_lr_schedule(self, learning_rate) -> None:
        """Replace the learning rate (a float or a schedule from ``training.optimizers``). Like the
        phase timing it is baked into captured graphs: the next step captures again."""
        import dataclasses

        self.opt = dataclasses.replace(self.opt, learning_rate=learning_rate)
        self.eng.set_lr_schedule(*schedule_args(learning_rate))
        self._stale_graphs()

    def set_phase_timing(self, on: bool = True) -> None:
        """HIP timing events at the step's phase boundaries (recorded inside the captured graph too).
        Takes effect for graphs captured afterwards."""
        self.eng.set_phase_timing(bool(on))
        self._stale_graphs()

    def _stale_graphs(self) -> None:
        """A setting baked into captured step graphs changed: the next step captures again."""
        self._graph_ready = False
        self._multi_ready.clear()

    # ---- device step log (csrc/step_log.h) ----
    def set_step_log(self, capacity: int = 1024) -> None:
        """Keep a device-side ring of ``capacity`` per-step records -- loss, correct, lr and, with
        ``clip_norm`` / ``skip_nonfinite``, the norm, the clip factor and the guard's decision -- written
        inside the step graph, so ``train_steps(n)`` needs no host read per step. 0 turns it off. Takes
        effect for graphs captured afterwards: the captured ones are dropped."""
        if capacity < 0:
            raise ValueError("set_step_log: capacity >= 0 (0 = off)")
        if int(capacity) == int(self.eng.step_log_capacity()):
            return
        self.stream.synchronize()  # the engine drops its graphs: none may still be running
        with torch.cuda.stream(self.stream):
            self.eng.set_step_log(int(capacity))
        self._stale_graphs()
        self._grads_graph = False

    def read_step_log(self, first_t: int, last_t: int) -> list:
        """The records of optimizer steps ``first_t..last_t`` (``t`` = global_step after the step) as dicts
        ``{step, loss, correct, rows, lr, grad_norm, clip_scale, ok}``: one synchronisation and one copy.
        ``ValueError`` when the range exceeds the capacity or a slot holds another step (overwritten, or
        never written)."""
        cap = int(self.eng.step_log_capacity())
        self._check_log_range(first_t, last_t, cap)
        with torch.cuda.stream(self.stream):
            t_dev, rec_dev = self.eng.step_log()
            lo, hi = (first_t - 1) % cap, (last_t - 1) % cap + 1
            if lo < hi:  # the slots are one run of the ring: views, no gather
                t_sel, rec_sel = t_dev[lo:hi], rec_dev[lo:hi]
            else:        # the run wraps
                t_sel, rec_sel = torch.cat([t_dev[lo:], t_dev[:hi]]), torch.cat([rec_dev[lo:], rec_dev[:hi]])
            # t's two 32-bit halves ride beside the eight fp32 fields: one device-to-host copy
            packed = torch.cat([t_sel.view(torch.float32).view(-1, 2), rec_sel], dim=1).cpu()
        ts = packed[:, :2].contiguous().view(torch.int64).view(-1).tolist()
        out = []
        for t, got, r in zip(range(first_t, last_t + 1), ts, packed[:, 2:].tolist()):
            if got != t:
                raise ValueError("read_step_log: step %d is not in the log (slot holds %s)"
                                 % (t, "step %d" % got if got else "nothing"))
            out.append(dict(step=t, loss=r[0], correct=int(r[1]), rows=int(r[6]), lr=r[2], grad_norm=r[3],
                            clip_scale=r[4], ok=r[5] != 0.0))
        return out

    def phase_times(self) -> dict:
        """GPU milliseconds of the last step's phases (all 0 when timing is off)."""
        self.stream.synchronize()
        return {k: round(float(v), 4) for k, v in zip(self.PHASES, self.eng.phase_times().tolist())}

    def last_loss(self) -> float:
        """Mean training loss of the last step's batch (with its dropout mask)."""
        self.stream.synchronize()
        return float(self.eng.loss_rows().mean().item())

    def last_grad_norm(self) -> Tuple[float, float]:
        """``(norm, clip scale)`` of the last clipped step's averaged gradient: a host read of the
        device pair, so call it only when something is logged. ``(nan, 1.0)`` without ``clip_norm`` and
        without ``skip_nonfinite``."""
        if not (self.eng.clip_norm() > 0 or self.eng.skip_nonfinite()):
            return float("nan"), 1.0
        self.stream.synchronize()
        norm, scale = self.eng.grad_norm().tolist()
        return float(norm), float(scale)

    def skipped_steps(self) -> int:
        """Steps the non-finite guard skipped so far: a host read of the device counter (a statistic, not
        checkpointed), so call it only when something is logged."""
        self.stream.synchronize()
        return int(self.eng.skipped_steps())

    def last_step_ok(self) -> bool:
        self.stream.synchronize()
        return bool(self.eng.last_step_ok())

    def last_layer_norms(self):
        """A host read of the device table: call it only when something is logged."""
        if not self.layerwise or self._hstep == 0:
            return {}
        self.stream.synchronize()
        return dict(zip(LAYER_NAMES, (tuple(row) for row in self.eng.layer_norms().tolist())))

    # ---- device-resident input (reference feed: mnist_python_m.py:291-294) ----
    def set_device_dataset(self, images, labels, seed: int = 0) -> None:
        """Upload a training split once; every later ``train_step(None, None)`` gathers its batch on
        the device from ``perm[(global_step * B + b) % n]``. The permutation is redrawn at every
        epoch boundary, which is ``DataSet.next_batch``'s per-epoch reshuffle without a host feed.
        With ``accum_steps = K`` micro-batch ``m = K * global_step + j`` gathers ``perm[(m * B + b) % n]``:
        a step trains on ``K * B`` consecutive positions, and the reshuffle happens at the first step
        boundary after an epoch ends."""
        x = _as_f32(images)
        y = _labels_to_ids(labels)
        n = x.shape[0]
        self._perm_gen = torch.Generator().manual_seed(int(seed))
        with torch.cuda.stream(self.stream):
            self._dev_data = x.to(self.device, non_blocking=False).contiguous()
            self._dev_labels = y.to(self.device).contiguous()
            self._dev_perm = torch.randperm(n, generator=self._perm_gen).to(torch.int32).to(self.device)
            self.eng.set_dataset(self._dev_data, self._dev_labels, self._dev_perm)
            self.eng.set_input_mode(1)
        self.stream.synchronize()
        self._hstep = self.global_step()
        self._epoch = (self._hstep * self._step_rows) // n

    @property
    def _step_rows(self) -> int:
        """Rows one train_step consumes: ``accum_steps`` micro-batches of ``batch_size``."""
        return self.accum_steps * self.batch_size

    def last_device_batch(self):
        """(x, y) device tensors of the rows the last device-input step trained on (``accum_steps *
        batch_size`` of them, in micro-batch order)."""
        n = self._dev_data.shape[0]
        pos = ((self._hstep - 1) * self._step_rows + torch.arange(self._step_rows, device=self.device)) % n
        with torch.cuda.stream(self.stream):
            rows = self._dev_perm[pos].long()
            out = self._dev_data[rows], self._dev_labels[rows]
        self.stream.synchronize()
        return out

    def _device_batch(self) -> None:
        n = self._dev_data.shape[0]
        ep = (self._hstep * self._step_rows) // n
        if ep != self._epoch:
            self._epoch = ep
            p = torch.randperm(n, generator=self._perm_gen).to(torch.int32)
            with torch.cuda.stream(self.stream):
                self._dev_perm.copy_(p.to(self.device))
                self.eng.invalidate_prefetch()  # rows prefetched from the old permutation

    # ---- state ----
    def params(self) -> torch.Tensor:
        return self.eng.params()

    def global_step(self) -> int:
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return int(self.eng.step_tensor().item())

    def set_global_step(self, s: int) -> None:
        with torch.cuda.stream(self.stream):
            self.eng.step_tensor().fill_(int(s))
            self.eng.sync_micro_step()  # micro = accum_steps * global_step
        self._hstep = int(s)

    def load_flat(self, flat, slots, step):
        with torch.cuda.stream(self.stream):
            self.eng.params().copy_(flat.to(self.device))
            self.eng.sync_shadow()
            if "m" in slots or "accum" in slots:
                self.eng.adam_m().copy_(slots.get("m", slots.get("accum")).to(self.device))
            if "v" in slots:
                self.eng.adam_v().copy_(slots["v"].to(self.device))
            for name, dst in self._rule_slots().items():  # RMSProp / Adagrad
                if name in slots:
                    # the padding behind the variables is in no checkpoint: it keeps its initial value (a
                    # zero accumulator there would divide 0 by 0)
                    dst[:M.NUM_PARAMS].copy_(slots[name].to(self.device)[:M.NUM_PARAMS])
            self.eng.step_tensor().fill_(int(step))
            self.eng.sync_micro_step()
            if self.ema_on:
                self.eng.load_ema(self.eng.params())
        self.stream.synchronize()
        self._hstep = int(step)

    def ema_params(self) -> torch.Tensor:
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return self.eng.ema_params()

    def load_ema(self, flat) -> None:
        if self.ema_on:
            with torch.cuda.stream(self.stream):
                self.eng.load_ema(flat.to(self.device))
            self.stream.synchronize()

    def reset_ema(self) -> None:
        if self.ema_on:
            with torch.cuda.stream(self.stream):
                self.eng.load_ema(self.eng.params())

    def _rule_slots(self) -> "dict":
        """RMSProp's / Adagrad's slots where the engine keeps them: ms / accum in the v buffer, mom in the m
        buffer, the centered rule's mg in the third."""
        o = self.opt
        if o.kind == "rmsprop":
            out = {"ms": self.eng.adam_v(), "mom": self.eng.adam_m()}
            if o.centered:
                out["mg"] = self.eng.slot3()
            return out
        if o.kind == "adagrad":
            return {"accum": self.eng.adam_v()}
        return {}

    def slot_tensors(self):
        self.stream.synchronize()
        if self.opt.kind in ("rmsprop", "adagrad"):
            return self._rule_slots()
        if self.opt.kind in ("adam", "lamb"):
            return {"m": self.eng.adam_m(), "v": self.eng.adam_v()}
        if self.opt.kind in ("momentum", "lars"):
            return {"accum": self.eng.adam_m()}
        return {}

    def powers(self):
        o = self.opt
        if o.kind != "adam":
            return {}
        t = self.global_step()
        return {"beta1_power": o.beta1 ** t, "beta2_power": o.beta2 ** t}

    def set_params(self, flat: torch.Tensor) -> None:
        with torch.cuda.stream(self.stream):
            self.eng.params().copy_(flat.to(self.device, non_blocking=True))
            self.eng.sync_shadow()
            if self.ema_on:
                self.eng.load_ema(self.eng.params())

    def broadcast_from(self, root: int = 0) -> None:
        """Chief init -> every worker (reference M6: init_op on PS vars; here an RCCL broadcast)."""
        if self.comm is None:
            return
        with torch.cuda.stream(self.stream):
            self.comm.broadcast(self.eng.params(), root)
            self.comm.broadcast(self.eng.adam_m(), root)
            self.comm.broadcast(self.eng.adam_v(), root)
            if self.opt.kind == "rmsprop" and self.opt.centered:
                self.comm.broadcast(self.eng.slot3(), root)
            self.comm.broadcast(self.eng.step_tensor(), root)
            self.eng.sync_micro_step()
            if self.ema_on:
                self.comm.broadcast(self.eng.ema_params(), root)
            self.eng.sync_shadow()
        self.stream.synchronize()
        self._hstep = int(self.eng.step_tensor().item())

    # ---- feeds ----
    def _feed(self, x, y) -> None:
        if x is None:
            assert self._dev_data is not None, "train_step(None, None) needs set_device_dataset() first"
            self._device_batch()
            return
        if self._dev_data is not None:
            raise ValueError("host batches fed to a runner in device-input mode")
        x = _as_f32(x)
        y = _labels_to_ids(y)
        assert x.shape[0] == self._step_rows, \
            f"batch {x.shape[0]} != accum_steps {self.accum_steps} x engine batch {self.batch_size}"
        self._x_stage.copy_(x)
        self._y_stage.copy_(y)
        with torch.cuda.stream(self.stream):
            self.eng.feed_x().copy_(self._x_stage, non_blocking=True)
            self.eng.feed_y().copy_(self._y_stage, non_blocking=True)

    # ---- steps ----
    def train_step(self, x, y) -> None:
        self._feed(x, y)
        with torch.cuda.stream(self.stream):
            if self.use_graph:
                if not self._graph_ready:
                    self.eng.train_step()
                    self.eng.capture_train_step("train")
                    self._graph_ready = True
                else:
                    self.eng.replay("train", 1)
            else:
                self.eng.train_step()
        self._hstep += 1
        if x is not None:
            # the pinned staging buffers are reused next step: wait for the H2D copies to land
            self.stream.synchronize()

    def _steps_to_reshuffle(self) -> int:
        """Steps until the step boundary where ``_device_batch`` redraws the permutation (>= 1)."""
        n, rows = self._dev_data.shape[0], self._step_rows
        return -(-((self._epoch + 1) * n - self._hstep * rows) // rows)

    def train_steps(self, n: int) -> None:
        """``n`` optimizer steps with no host synchronisation (device input only): one replay of an
        ``n``-step graph, captured once per distinct ``n``. The permutation is redrawn exactly at the step
        boundaries where ``train_step(None, None)`` redraws it, so the stream of permutations is the same;
        a call that such a boundary cuts runs as one-step replays. Read the steps' losses and metrics with
        ``read_step_log`` (``set_step_log`` first)."""
        if self._dev_data is None:
            raise ValueError("train_steps needs the device-resident split (set_device_dataset); host-fed batches "
                             "go through train_step")
        if not 1 <= n <= 1000:
            raise ValueError("train_steps: 1 <= n <= 1000 (one captured graph), got %d" % n)
        left = n
        while left > 0:
            self._device_batch()  # the reshuffle, when one is due at this boundary
            k = min(left, max(1, self._steps_to_reshuffle()))
            if k == n and self.use_graph:
                name = "train%d" % n
                if n in self._multi_ready:
                    with torch.cuda.stream(self.stream):
                        self.eng.replay(name, 1)
                    self._hstep += n
                else:
                    # the first call of this length: one-step replays (the first of which runs eagerly, as
                    # train_step's does), then the capture for the calls to come
                    for _ in range(n):
                        self.train_step(None, None)
                    with torch.cuda.stream(self.stream):
                        self.eng.capture_train_steps(name, n)
                    self._multi_ready.add(n)
            else:
                for _ in range(k):
                    self.train_step(None, None)
            left -= k

    def compute_grads(self, x, y, with_loss: bool = True) -> Tuple[torch.Tensor, Optional[float]]:
        """Forward + backward only (no reduction / optimizer). Bumps the engine's local step. With
        ``use_graph`` the three launches replay as one captured graph (``MnistEngine.capture_grads``).
        ``with_loss=False`` skips the loss read-back (no device-to-host transfer). One batch only: with
        ``accum_steps > 1`` it raises (the parameter-server modes that use it do not accumulate)."""
        if self.accum_steps > 1:
            raise ValueError(f"compute_grads handles one batch; the optimizer has accum_steps={self.accum_steps}")
        self._feed(x, y)
        with torch.cuda.stream(self.stream):
            if self.use_graph:
                if not self._grads_graph:
                    self.eng.forward(True)
                    self.eng.backward_a()
                    self.eng.backward_b()
                    self.eng.capture_grads("grads")
                    self._grads_graph = True
                else:
                    self.eng.replay("grads", 1)
            else:
                self.eng.forward(True)
                self.eng.backward_a()
                self.eng.backward_b()
        self.stream.synchronize()
        self._hstep += 1
        return self.eng.grads(), (float(self.eng.loss_rows().mean().item()) if with_loss else None)

    def sync_state(self) -> None:
        """ZeRO-1 (``eng.zero()``): every worker gathers the fc1 shards of the fp32 master and the Adam
        slots, so ``params()`` / ``slot_tensors()`` are whole (a collective: all workers call it)."""
        with torch.cuda.stream(self.stream):
            self.eng.sync_params()
        self.stream.synchronize()

    def sync_shadow(self) -> None:
        """Re-derive the bf16 operand shadow from the fp32 master (after a parameter server wrote the
        fresh values into ``params()``)."""
        with torch.cuda.stream(self.stream):
            self.eng.sync_shadow()

    def reduce_grads(self, weight: float = 1.0) -> None:
        """Sum-all-reduce of (weight * local grads) over the worker communicator."""
        with torch.cuda.stream(self.stream):
            self.eng.reduce_grads(weight)
        self.stream.synchronize()

    def apply_grads(self, grad: Optional[torch.Tensor] = None, scale: float = 1.0) -> None:
        with torch.cuda.stream(self.stream):
            if grad is not None and grad.data_ptr() != self.eng.grads().data_ptr():
                self.eng.grads().copy_(grad.to(self.device))
            self.eng.apply_optimizer(scale)
        self.stream.synchronize()

    def evaluate(self, x, y, use_ema: bool = False) -> Tuple[float, int]:
        """``use_ema``: the forward reads the moving averages in place of the parameters."""
        x = _as_f32(x).to(self.device)
        y = _labels_to_ids(y).to(self.device)
        with torch.cuda.stream(self.stream):
            r = self.eng.evaluate(x, y, bool(use_ema))
        self.stream.synchronize()
        r = r.cpu()
        return float(r[0]), int(round(float(r[1])))

    # ---- device inference (csrc/mnist_infer.h) ----
    def predict(self, x, use_ema: bool = False):
        """``(logits [n,10] fp32, classes [n] int32)`` on the device: the forward up to fc1 and the
        inference head, rows in chunks of the engine's batch. ``use_ema`` as in ``evaluate``."""
        x = _as_rows(x).to(self.device).contiguous()
        none = torch.empty(0, dtype=torch.int32, device=self.device)
        with torch.cuda.stream(self.stream):
            logits, classes, _, _ = self.eng.predict(x, none, bool(use_ema))
        self.stream.synchronize()
        return logits, classes

    def set_eval_dataset(self, images, labels) -> None:
        """Upload an evaluation split once; ``evaluate_dataset`` reads it on the device. Labels outside
        [0, 10) are refused."""
        x, y = _check_eval_split(images, labels)
        self.stream.synchronize()  # the engine drops its evaluation graphs: none may still be running
        with torch.cuda.stream(self.stream):
            self._eval_x = x.to(self.device).contiguous()
            self._eval_y = y.to(self.device).contiguous()
            self.eng.set_eval_dataset(self._eval_x, self._eval_y)
        self.stream.synchronize()
        self._eval_graphs = set()

    def evaluate_dataset(self, first: int = 0, count: Optional[int] = None, group: Optional[int] = None,
                         use_ema: bool = False) -> list:
        """Records ``{loss_sum, rows, correct, confusion}`` of rows ``[first, first + count)`` of the
        evaluation split, one per group of ``group`` rows (default: all of them in one group), folded on
        the device. With ``use_graph`` the whole pass is one hipGraph per ``(first, count, group,
        use_ema)``, captured at its first use: a call is one replay, one synchronisation and one copy."""
        first, count, group = _eval_range(getattr(self, "_eval_x", None), first, count, group)
        if count == 0:
            return []
        with torch.cuda.stream(self.stream):
            if self.use_graph:
                name = "eval:%d:%d:%d:%d" % (first, count, group, int(bool(use_ema)))
                if name not in self._eval_graphs:
                    self.eng.capture_eval(name, first, count, group, bool(use_ema))
                    self._eval_graphs.add(name)
                self.eng.replay(name, 1)
                rec = self.eng.eval_records(name)
            else:
                rec = self.eng.evaluate_dataset(first, count, group, bool(use_ema))
        self.stream.synchronize()
        return [inference.record_from_device(r) for r in rec.cpu().numpy()]


def make_runner(batch_size: int, optimizer, device: torch.device, keep_prob: float = 0.75, seed: int = 0,
                rank: int = 0, comm=None, bf16_grads: bool = True, use_graph: bool = True,
                dtype: str = "bf16") -> MnistRunnerBase:
    if device.type == "cuda":
        return NativeMnistRunner(batch_size, optimizer, keep_prob, seed, rank, device, comm, bf16_grads, use_graph,
                                 dtype)
    return TorchMnistRunner(batch_size, optimizer, keep_prob, seed, rank, device)
