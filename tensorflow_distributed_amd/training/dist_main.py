"""The distributed trainer behind ``mnist_python_m.py`` / ``mnist_python_w1.py`` / ``mnist_python_w2.py``
(``/root/reference/mnist_python_m.py:49-326``): same 14 flags and defaults, same roles, same stdout.

Roles:
  * ``--job_name=ps``: hosts the rendezvous store at ``--ps_hosts[task_index]`` (task 0), joins the
    control group and runs ``server.join()`` -- the async parameter-server service when
    ``--sync_replicas=False``, otherwise it just waits for the workers' completion signal.
  * ``--job_name=worker``: task 0 is the chief. GPU ``task_index % num_gpus`` (``--num_gpus>0``)
    or CPU. Chief initialises (or restores) and broadcasts; the loop runs until the GLOBAL step
    reaches ``--train_steps``; then a 5 x 1000 validation pass.

Sync mode = all-reduce DP with SyncReplicasOptimizer semantics (parallel/sync_replicas.py); async
mode = Hogwild PS over Gloo point-to-point (parallel/async_ps.py). ``main`` resolves the roles once and
hands over to ``_run_ps``, ``_mnist_worker`` or ``_resnet_worker``; how the MNIST worker synchronises
gradients is one object of training/grad_sync.py.
"""
from __future__ import annotations

import os
import sys
import tempfile
import time
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from ..models import mnist_cnn as M
from ..parallel import async_ps
from ..parallel import schedule as SCH
from ..utils import flags as flags_mod
from ..utils.flags import FLAGS

_DEFINED = False


def define_flags(task_index_default: int = 0, job_name_default: str = "ps") -> None:
    """The reference's 14 flags (mnist_python_m.py:49-87) + framework extras."""
    global _DEFINED
    f = flags_mod
    if _DEFINED:
        FLAGS._flags["task_index"].default = task_index_default
        FLAGS._flags["job_name"].default = job_name_default
        FLAGS.reset()
        return
    _DEFINED = True
    f.DEFINE_string("data_dir", "/tmp/mnist-data", "Directory for storing mnist data")
    f.DEFINE_boolean("download_only", False, "Only perform downloading of data; Do not proceed to "
                     "session preparation, model definition or training")
    f.DEFINE_integer("task_index", task_index_default, "Worker task index, should be >= 0. task_index=0 is "
                     "the master worker task the performs the variable initialization ")
    f.DEFINE_integer("num_gpus", 0, "Total number of gpus for each machine. If you don't use GPU, please set it to '0'")
    f.DEFINE_integer("replicas_to_aggregate", 2, "Number of replicas to aggregate before parameter update"
                     "is applied (For sync_replicas mode only; default: num_workers)")
    f.DEFINE_integer("hidden_units", 100, "Number of units in the hidden layer of the NN (unused by the CNN, "
                     "kept for flag compatibility)")
    f.DEFINE_integer("train_steps", 4, "Number of (global) training steps to perform")
    f.DEFINE_integer("batch_size", 128, "Training batch size")
    f.DEFINE_float("learning_rate", 0.01, "Learning rate")
    # learning-rate schedule over global_step (training/optimizers.py; evaluated on the device by the
    # optimizer kernels, csrc/lr_schedule.h). The defaults are the constant --learning_rate.
    f.DEFINE_enum("lr_schedule", "constant", ["constant", "exponential", "piecewise", "polynomial", "cosine"],
                  "Learning rate as a function of global_step: constant = --learning_rate; exponential = "
                  "lr * rate^(step / decay_steps) (tf.train.exponential_decay); piecewise = --lr_values between "
                  "--lr_boundaries (tf.train.piecewise_constant); polynomial = (lr - end) * (1 - step/decay_steps)"
                  "^power + end; cosine = lr * ((1 - alpha) * 0.5 * (1 + cos(pi * step/decay_steps)) + alpha)")
    f.DEFINE_integer("lr_decay_steps", 1000, "--lr_schedule exponential / polynomial / cosine: decay steps")
    f.DEFINE_float("lr_decay_rate", 0.96, "--lr_schedule=exponential: decay rate")
    f.DEFINE_boolean("lr_staircase", False, "--lr_schedule=exponential: integer step / decay_steps")
    f.DEFINE_string("lr_boundaries", "", "--lr_schedule=piecewise: comma-separated increasing global steps (at most 4); "
                    "the rate is values[i] for the first i with step <= boundaries[i]")
    f.DEFINE_string("lr_values", "", "--lr_schedule=piecewise: comma-separated rates, one more than boundaries")
    f.DEFINE_float("lr_end", 0.0001, "--lr_schedule=polynomial: end learning rate")
    f.DEFINE_float("lr_power", 1.0, "--lr_schedule=polynomial: power")
    f.DEFINE_float("lr_alpha", 0.0, "--lr_schedule=cosine: floor, as a fraction of --learning_rate")
    f.DEFINE_integer("lr_warmup_steps", 0, "Linear warm-up: for step < this, the rate is scaled by (step + 1) / this")
    f.DEFINE_float("clip_norm", 0.0, "tf.clip_by_global_norm on the aggregated (averaged) gradient before the "
                   "optimizer; on GPUs the norm and the clip factor are taken on the device inside the step "
                   "graph. 0 = off. Synchronous all-reduce training of --model mnist_cnn only")
    f.DEFINE_boolean("skip_nonfinite", False, "Non-finite guard: an optimizer step whose aggregated gradient is not "
                     "finite (an inf / NaN element, or a norm beyond fp32) is skipped -- parameters, optimizer slots "
                     "and the moving averages keep their bits; global_step, the data cursor and the schedules advance. "
                     "On GPUs decided on the device inside the step graph. Synchronous all-reduce training of --model "
                     "mnist_cnn only")
    f.DEFINE_float("ema_decay", 0.0, "tf.train.ExponentialMovingAverage of the weights (SyncReplicasOptimizer's "
                   "variable_averages), updated inside the optimizer kernels after every aggregated update; "
                   "0 = off. The checkpoint carries <var>/ExponentialMovingAverage")
    f.DEFINE_boolean("ema_num_updates", True, "--ema_decay: TF's num_updates=global_step, the decay of update t is "
                     "min(ema_decay, (1 + t) / (10 + t))")
    f.DEFINE_boolean("ema_eval", True, "--ema_decay: --eval_at_steps, the validation prints and the final accuracy "
                     "read the averages instead of the variables")
    f.DEFINE_integer("grad_accum_steps", 1, "Gradient accumulation: every optimizer step sums this many micro-batches "
                     "of --batch_size rows per worker (on GPUs on the device, inside the step graph) before the one "
                     "clip, trust ratio, all-reduce and update. --train_steps, global_step/sec, checkpoints and "
                     "--eval_at_steps count optimizer steps. 1 = off. Synchronous all-reduce training of --model "
                     "mnist_cnn only")
    f.DEFINE_integer("steps_per_call", 1, "TF's iterations_per_loop: optimizer steps per host round trip. N > 1 "
                     "replays N steps as one captured graph with no host synchronisation between them and reads "
                     "every step's loss, lr, gradient norm and guard decision once per call from the device step "
                     "log (csrc/step_log.h); a call also ends at every --eval_at_steps value, "
                     "--check_consistency_every multiple and at --fault_inject_step. The Supervisor, the summaries "
                     "and the watchdog see one step per call. 1 = one step per call (the default). GPU "
                     "--device_input training of --model mnist_cnn, one worker or synchronous all-reduce DP")
    f.DEFINE_boolean("sync_replicas", True, "Use the sync_replicas (synchronized replicas) mode, "
                     "wherein the parameter updates from workers are aggregated before applied to "
                     "avoid stale gradients")
    f.DEFINE_boolean("existing_servers", False, "Whether servers already exists. If True, will use "
                     "the worker hosts via their GRPC URLs (one client process per worker host). "
                     "Otherwise, will create an in-process TensorFlow server.")
    f.DEFINE_string("ps_hosts", "10.0.1.3:2222", "Comma-separated list of hostname:port pairs")
    f.DEFINE_string("worker_hosts", "10.0.1.6:2223,10.0.1.2:2224", "Comma-separated list of hostname:port pairs")
    f.DEFINE_string("job_name", job_name_default, "job name: worker or ps")
    # ---- framework extras ----
    f.DEFINE_string("logdir", "", "Supervisor logdir (checkpoints, events). Empty = tempfile.mkdtemp() "
                    "like the reference; set it to a stable path to enable resume")
    f.DEFINE_float("save_model_secs", 600.0, "Checkpoint period (chief)")
    f.DEFINE_float("save_summaries_secs", 120.0, "Summary (global_step/sec) period (chief)")
    f.DEFINE_integer("seed", 0, "Init seed (normal(0,1) params, chief)")
    f.DEFINE_float("keep_prob", 0.75, "Dropout keep probability during training")
    f.DEFINE_enum("optimizer", "adam", ["adam", "sgd", "momentum", "lamb", "lars", "rmsprop", "adagrad"],
                  "Optimizer (reference: adam). lamb "
                  "and lars scale every variable's update by a trust ratio formed from two per-variable L2 norms "
                  "(on GPUs on the device, inside the step graph); synchronous all-reduce training of --model "
                  "mnist_cnn only. rmsprop and adagrad (tf.train.RMSPropOptimizer / AdagradOptimizer): --model "
                  "mnist_cnn, every training mode but the GPU-resident parameter server")
    f.DEFINE_float("momentum", 0.9, "Momentum for --optimizer=momentum and lars (rmsprop has --rmsprop_momentum)")
    f.DEFINE_float("rmsprop_decay", 0.9, "--optimizer=rmsprop: decay of the moving averages of g^2 (and g, centered)")
    f.DEFINE_float("rmsprop_momentum", 0.0, "--optimizer=rmsprop: momentum")
    f.DEFINE_float("rmsprop_epsilon", 1e-10, "--optimizer=rmsprop: epsilon under the square root")
    f.DEFINE_boolean("rmsprop_centered", False, "--optimizer=rmsprop: normalise by the estimated variance (a third slot)")
    f.DEFINE_float("adagrad_init_accum", 0.1, "--optimizer=adagrad: initial_accumulator_value (> 0)")
    f.DEFINE_float("weight_decay", -1.0, "--optimizer=lamb / lars: weight decay lambda (default: 0 for lamb, 1e-4 for "
                   "lars)")
    f.DEFINE_float("lars_eeta", 1e-3, "--optimizer=lars: the trust coefficient eeta")
    f.DEFINE_boolean("layerwise_skip_bias", True, "--optimizer=lamb / lars: the biases take neither the weight decay "
                     "nor the trust ratio (LARS's skip_list, LAMB's exclude_from_*)")
    f.DEFINE_boolean("synthetic_data", False, "Use the synthetic MNIST-shaped dataset even if IDX files exist")
    f.DEFINE_boolean("bf16_grads", True, "All-reduce gradients in bf16 (GPU)")
    f.DEFINE_boolean("use_graph", True, "Replay the captured hipGraph of the train step (GPU)")
    f.DEFINE_integer("eval_batches", 5, "Validation batches after training")
    f.DEFINE_integer("eval_batch_size", 1000, "Validation batch size")
    f.DEFINE_boolean("device_eval", False, "Evaluate on the device: the validation split is uploaded once and the "
                     "final pass and every --eval_at_steps row are one evaluate_dataset over its first --eval_batches x "
                     "--eval_batch_size rows, in split order (not next_batch's shuffle: the same mean whenever they are "
                     "the whole split, as the default 5 x 1000 are), one record per batch folded by the engine (GPU: "
                     "one replayed graph, one read-back). --model mnist_cnn, synchronous all-reduce training")
    f.DEFINE_boolean("confusion_matrix", False, "--device_eval: print the 10 x 10 confusion matrix and the per-class "
                     "recall and precision of the final pass; the metrics file's evaluation record carries them")
    f.DEFINE_string("metrics_file", "", "Chief: JSONL metrics per step")
    f.DEFINE_string("trace_file", "", "Chrome-trace JSON of host step phases")
    f.DEFINE_integer("check_consistency_every", 0, "Every N steps all-reduce a param checksum and "
                     "fail on cross-worker desync (sync mode)")
    f.DEFINE_integer("fault_inject_step", -1, "Test hook: the worker --fault_inject_task exits abruptly "
                     "when its global step reaches this value (first attempt only)")
    f.DEFINE_integer("fault_inject_task", -1, "Worker task index for --fault_inject_step")
    f.DEFINE_string("straggler_delay", "", "Test hook: 'task:seconds,...' artificial per-step delay "
                    "(backup-worker tests)")
    f.DEFINE_float("rendezvous_timeout", 600.0, "Seconds to wait for the cluster to assemble")
    f.DEFINE_boolean("quiet", False, "Suppress per-step prints")
    f.DEFINE_boolean("debug_sync", False, "Serialise every HIP launch/copy (AMD_SERIALIZE_KERNEL=3, "
                     "HIP_LAUNCH_BLOCKING=1): race-hunting mode")
    f.DEFINE_float("step_timeout_secs", 0.0, "Watchdog: abort the communicator and exit non-zero when no step "
                   "completes for this long (0 = off); the launcher then restarts from the last checkpoint")
    f.DEFINE_string("eval_at_steps", "", "Chief: comma-separated global steps at which to run the validation "
                    "pass and print a 'performance' table row (steps, training seconds, accuracy %, lr)")
    f.DEFINE_boolean("log_device_placement", False, "Print where every variable and the compute live "
                     "(ConfigProto.log_device_placement, mnist_python_m.py:257)")
    f.DEFINE_enum("dp_transport", "auto", ["auto", "rccl", "ipc"], "GPU sync gradient transport: auto = "
                  "peer-to-peer IPC when workers share a GPU (--num_gpus < workers; RCCL refuses that), else "
                  "RCCL over xGMI (+ IPC one-shot for the small conv bucket)")
    f.DEFINE_string("dp_schedule", "fixed", "Sync DP schedule (workers > 1). fixed (default) = one schedule per "
                    "device/dtype, so two identical runs train the same trajectory (GPU bf16 sfb+zero+mr, GPU fp32 "
                    "allreduce, CPU flat); auto = before training every worker times each candidate for "
                    "--dp_probe_steps steps and all keep the fastest (max over workers) -- the schedules round "
                    "differently, so auto trades bit-reproducibility across runs for speed; or "
                    "a name. GPU bf16: sfb+zero+mr, sfb+mr, sfb+zero, sfb, allreduce (parallel/schedule.py: "
                    "sufficient-factor fc gradients, ZeRO-1 fc1 sharding, slab reduce merged into the SFB GEMM, "
                    "bucketed all-reduce); GPU fp32: allreduce; CPU (Gloo): flat, buckets")
    f.DEFINE_integer("dp_probe_steps", 200, "Timed steps per --dp_schedule=auto candidate (CPU: at most 5)")
    f.DEFINE_integer("dp_probe_warmup", 30, "Untimed steps before each candidate's timing (CPU: 1)")
    f.DEFINE_integer("zero_sync_every", 100, "ZeRO-1 schedules: every this many global steps all workers agree "
                     "whether the chief's checkpoint is due and, if so, gather the sharded fc1 state first")
    f.DEFINE_boolean("phase_timing", False, "GPU: HIP timing events at the step's phase boundaries (forward, fc "
                     "backward, conv backward, optimizer, all-reduce), written to --metrics_file (always on when "
                     "--metrics_file is set on the chief)")
    f.DEFINE_enum("dtype", "bf16", ["bf16", "fp32"], "GPU compute precision: bf16 MFMA operands (fp32 accumulate, "
                  "master weights and optimizer), or fp32 everywhere (the reference's precision, "
                  "mnist_python_m.py:185-200)")
    f.DEFINE_float("bucket_mb", 0.0, "Gradient all-reduce bucketing: 0 = the MNIST engine's two buckets (fc 12.9 "
                   "MB over RCCL, conv 0.2 MB over the IPC one-shot kernel); > 0 = bucket size for the "
                   "generic bucket reducer (--model resnet*)")
    f.DEFINE_enum("model", "mnist_cnn", ["mnist_cnn", "resnet18", "resnet50"], "Model: the reference CNN, or the "
                  "synthetic-ImageNet ResNet family (BASELINE configs 4-5; trained by bench_resnet.py)")
    f.DEFINE_integer("image_size", 224, "--model resnet*: synthetic image height = width")
    f.DEFINE_boolean("bn_deterministic", False, "--model resnet*: batch-norm statistics in row mode (fixed summation "
                     "order, bit-reproducible runs) instead of slot mode's fp32 atomics (~3 % faster, order varies)")
    f.DEFINE_boolean("ps_on_gpu", True, "Parameter-server modes (async, backup workers) with --num_gpus > 0: each "
                     "ps task keeps its variables, optimizer slots and accumulator on GPU task_index % num_gpus; "
                     "workers push gradients into its GPU mailbox and the ps writes fresh values straight into "
                     "the workers' engine parameters (IPC peer memory, no host copies). False = the reference's "
                     "CPU ps (ps_device=/job:ps/cpu:0)")
    f.DEFINE_boolean("device_input", True, "GPU: upload the training split once and index it on the device "
                     "by a per-epoch shuffle (no per-step host feed); False = host next_batch + H2D per step")


def _make_learning_rate():
    """--learning_rate, or the schedule the --lr_* flags describe (a float when they are all default)."""
    from . import optimizers as O

    lr, w, kind = FLAGS.learning_rate, FLAGS.lr_warmup_steps, FLAGS.lr_schedule
    if kind == "exponential":
        return O.ExponentialDecay(lr, FLAGS.lr_decay_steps, FLAGS.lr_decay_rate, FLAGS.lr_staircase, w)
    if kind == "piecewise":
        bounds = tuple(int(b) for b in FLAGS.lr_boundaries.split(",") if b.strip())
        values = tuple(float(v) for v in FLAGS.lr_values.split(",") if v.strip())
        return O.PiecewiseConstant(bounds, values, w)
    if kind == "polynomial":
        return O.PolynomialDecay(lr, FLAGS.lr_decay_steps, FLAGS.lr_end, FLAGS.lr_power, w)
    if kind == "cosine":
        return O.CosineDecay(lr, FLAGS.lr_decay_steps, FLAGS.lr_alpha, w)
    return O.ConstantWarmup(lr, w) if w > 0 else lr


def _make_optimizer():
    from .optimizers import (AdagradOptimizer, AdamOptimizer, GradientDescentOptimizer, LAMBOptimizer, LARSOptimizer,
                             MomentumOptimizer, RMSPropOptimizer)

    lr = _make_learning_rate()
    clip = FLAGS.clip_norm if FLAGS.clip_norm > 0 else None
    acc = int(FLAGS.grad_accum_steps)
    ema = dict(ema_decay=FLAGS.ema_decay, ema_num_updates=bool(FLAGS.ema_num_updates)) if FLAGS.ema_decay > 0 else {}
    if FLAGS.skip_nonfinite:  # rides with the EMA keywords: every config takes it
        ema["skip_nonfinite"] = True
    if FLAGS.optimizer in LAYERWISE_OPTIMIZERS:
        wd = {} if FLAGS.weight_decay < 0 else dict(weight_decay=FLAGS.weight_decay)
        common = dict(skip_bias=bool(FLAGS.layerwise_skip_bias), clip_norm=clip, **wd, **ema)
        if FLAGS.optimizer == "lamb":
            return LAMBOptimizer(lr, accum_steps=acc, **common)
        return LARSOptimizer(lr, FLAGS.momentum, eeta=FLAGS.lars_eeta, accum_steps=acc, **common)
    if FLAGS.optimizer == "sgd":
        return GradientDescentOptimizer(lr, clip_norm=clip, accum_steps=acc, **ema)
    if FLAGS.optimizer == "momentum":
        return MomentumOptimizer(lr, FLAGS.momentum, clip_norm=clip, accum_steps=acc, **ema)
    if FLAGS.optimizer == "rmsprop":  # --momentum is momentum's / lars's: RMSProp's own default is 0
        return RMSPropOptimizer(lr, FLAGS.rmsprop_decay, FLAGS.rmsprop_momentum, FLAGS.rmsprop_epsilon,
                                bool(FLAGS.rmsprop_centered), clip_norm=clip, accum_steps=acc, **ema)
    if FLAGS.optimizer == "adagrad":
        return AdagradOptimizer(lr, FLAGS.adagrad_init_accum, clip_norm=clip, accum_steps=acc, **ema)
    return AdamOptimizer(lr, clip_norm=clip, accum_steps=acc, **ema)


LAYERWISE_OPTIMIZERS = ("lamb", "lars")


def check_layerwise_flags(num_workers: int) -> None:
    """--optimizer=lamb / lars form per-variable norms of the aggregated gradient of synchronous all-reduce
    training. The combinations they do not cover are flag errors, raised before any process group is
    built; each is a follow-up."""
    if FLAGS.optimizer not in LAYERWISE_OPTIMIZERS:
        if FLAGS.weight_decay >= 0:
            raise ValueError("--weight_decay belongs to --optimizer=lamb / lars (got --optimizer=%s)" % FLAGS.optimizer)
        return
    which = "--optimizer=%s" % FLAGS.optimizer
    if FLAGS.optimizer == "lars" and not FLAGS.lars_eeta > 0:
        raise ValueError("--lars_eeta=%g: must be > 0" % FLAGS.lars_eeta)
    if not FLAGS.sync_replicas:
        raise ValueError("%s with --sync_replicas=False: the asynchronous parameter server applies each worker's "
                         "gradient on its own shard, which has no per-variable norm (follow-up)" % which)
    r2a = FLAGS.replicas_to_aggregate
    if r2a is not None and r2a < num_workers:
        raise ValueError("%s with backup workers (--replicas_to_aggregate=%d < %d workers): the accumulator paths "
                         "have no layer-wise optimizer yet (follow-up)" % (which, r2a, num_workers))
    if FLAGS.model != "mnist_cnn":
        raise ValueError("%s with --model %s: the ResNet runner is not wired to the layer-wise ops yet "
                         "(follow-up; the flat ops are general over the variable table)" % (which, FLAGS.model))
    if FLAGS.dp_schedule not in ("fixed", "auto", "allreduce", "flat", "buckets"):
        raise ValueError("%s with --dp_schedule=%s: a sharded gradient has no per-variable norm; use the all-reduce "
                         "schedule" % (which, FLAGS.dp_schedule))


RULE_OPTIMIZERS = ("rmsprop", "adagrad")


def check_rules_flags(num_workers: int) -> None:
    """--optimizer=rmsprop / adagrad run wherever the flat optimizer of --model mnist_cnn runs, and on the
    host parameter server. The two places without the rules are flag errors, raised before any process
    group is built; each is a follow-up."""
    if FLAGS.optimizer not in RULE_OPTIMIZERS:
        return
    which = "--optimizer=%s" % FLAGS.optimizer
    if FLAGS.model != "mnist_cnn":
        raise ValueError("%s with --model %s: the ResNet runner's bucketed optimizer has no such rule (follow-up)"
                         % (which, FLAGS.model))
    r2a = FLAGS.replicas_to_aggregate
    ps_mode = not FLAGS.sync_replicas or (r2a is not None and r2a < num_workers and bool(FLAGS.ps_hosts))
    if ps_mode and FLAGS.ps_on_gpu and FLAGS.num_gpus > 0:
        raise ValueError("%s with the GPU-resident parameter server: its shards know Adam, GradientDescent and "
                         "Momentum only (follow-up); pass --ps_on_gpu=False for the host parameter server, which "
                         "applies every rule" % which)


def check_grad_accum_flags(num_workers: int) -> None:
    """--grad_accum_steps sums micro-batch gradients ahead of the one aggregated update of synchronous
    all-reduce training. The combinations it does not cover are flag errors, raised before any process
    group is built (every rank sees the same flags), not silently unaccumulated runs."""
    k = FLAGS.grad_accum_steps
    if k < 1:
        raise ValueError("--grad_accum_steps=%d: must be >= 1 (1 = off)" % k)
    if k == 1:
        return
    which = "--grad_accum_steps=%d" % k
    if not FLAGS.sync_replicas:
        raise ValueError("%s with --sync_replicas=False: the asynchronous parameter server applies each worker's "
                         "gradient as it arrives; there is no update to accumulate towards" % which)
    r2a = FLAGS.replicas_to_aggregate
    if r2a is not None and r2a < num_workers:
        raise ValueError("%s with backup workers (--replicas_to_aggregate=%d < %d workers): the accumulator paths "
                         "take one batch per worker and step" % (which, r2a, num_workers))
    if FLAGS.model != "mnist_cnn":
        raise ValueError("%s with --model %s: the ResNet runner does not accumulate" % (which, FLAGS.model))
    if FLAGS.dp_schedule not in ("fixed", "auto", "allreduce", "flat", "buckets"):
        raise ValueError("%s with --dp_schedule=%s: the SFB / ZeRO schedules fuse gradient production with their "
                         "collectives, so there is no whole gradient to sum; use the all-reduce schedule"
                         % (which, FLAGS.dp_schedule))


def check_clip_norm_flags(num_workers: int) -> None:
    """--clip_norm clips the aggregated gradient of synchronous all-reduce training. The combinations
    it does not cover yet are flag errors, raised before any process group is built, not silently
    unclipped runs; each is a follow-up."""
    if FLAGS.clip_norm < 0:
        raise ValueError("--clip_norm=%g: must be >= 0 (0 = off)" % FLAGS.clip_norm)
    if not FLAGS.clip_norm > 0:
        return
    if not FLAGS.sync_replicas:
        raise ValueError("--clip_norm with --sync_replicas=False: the asynchronous parameter server applies each "
                         "worker's gradient on its own, there is no aggregated gradient to clip (follow-up: "
                         "per-push clipping on the ps)")
    r2a = FLAGS.replicas_to_aggregate
    if r2a is not None and r2a < num_workers:
        raise ValueError("--clip_norm with backup workers (--replicas_to_aggregate=%d < %d workers): the "
                         "accumulator paths do not clip yet (follow-up)" % (r2a, num_workers))
    if FLAGS.model != "mnist_cnn":
        raise ValueError("--clip_norm with --model %s: the ResNet runner's bucketed optimizer does not clip yet "
                         "(follow-up)" % FLAGS.model)


def check_skip_nonfinite_flags(num_workers: int) -> None:
    """--skip_nonfinite guards the aggregated update of synchronous all-reduce training. The combinations
    it does not cover are flag errors, raised before any process group is built (every rank sees the same
    flags), not silently unguarded runs."""
    if not FLAGS.skip_nonfinite:
        return
    if not FLAGS.sync_replicas:
        raise ValueError("--skip_nonfinite with --sync_replicas=False: the asynchronous parameter server applies each "
                         "worker's gradient on its own, there is no aggregated gradient to guard")
    r2a = FLAGS.replicas_to_aggregate
    if r2a is not None and r2a < num_workers:
        raise ValueError("--skip_nonfinite with backup workers (--replicas_to_aggregate=%d < %d workers): the "
                         "accumulator paths have no guard" % (r2a, num_workers))
    if FLAGS.model != "mnist_cnn":
        raise ValueError("--skip_nonfinite with --model %s: the ResNet runner's bucketed optimizer has no guard"
                         % FLAGS.model)
    if FLAGS.dp_schedule not in ("fixed", "auto", "allreduce", "flat", "buckets"):
        raise ValueError("--skip_nonfinite with --dp_schedule=%s: the guard reads the whole aggregated gradient on "
                         "every rank, which the SFB / ZeRO schedules never form; use the all-reduce schedule"
                         % FLAGS.dp_schedule)


def check_steps_per_call_flags(num_workers: int) -> None:
    """--steps_per_call N > 1 takes N optimizer steps per host round trip on the device. What it does not
    cover is a flag error, raised before any process group is built (every rank sees the same flags)."""
    n = FLAGS.steps_per_call
    if n < 1 or n > 1000:
        raise ValueError("--steps_per_call=%d: must be in [1, 1000] (one captured graph; 1 = off)" % n)
    if n == 1:
        return
    which = "--steps_per_call=%d" % n
    if not FLAGS.sync_replicas:
        raise ValueError("%s with --sync_replicas=False: a parameter-server worker exchanges its gradient with the "
                         "ps tasks after every step" % which)
    r2a = FLAGS.replicas_to_aggregate
    if r2a is not None and r2a < num_workers:
        raise ValueError("%s with backup workers (--replicas_to_aggregate=%d < %d workers): the contributors are "
                         "chosen on the host after every step" % (which, r2a, num_workers))
    if FLAGS.model != "mnist_cnn":
        raise ValueError("%s with --model %s: the ResNet runner has no device step log" % (which, FLAGS.model))
    if FLAGS.num_gpus <= 0:
        raise ValueError("%s with --num_gpus=0: the CPU runner steps from the host; the multi-step graph is the "
                         "GPU engine's" % which)
    if not FLAGS.device_input:
        raise ValueError("%s with --device_input=False: a host-fed batch crosses to the device before every step"
                         % which)
    if not FLAGS.use_graph:
        raise ValueError("%s with --use_graph=False: the N steps of a call are one captured graph" % which)


def check_device_eval_flags(num_workers: int) -> None:
    """--device_eval evaluates on the worker's engine from a split uploaded once; --confusion_matrix prints
    what its records hold. What they do not cover is a flag error, raised before any process group is built."""
    if FLAGS.confusion_matrix and not FLAGS.device_eval:
        raise ValueError("--confusion_matrix without --device_eval: the matrix is folded by the device evaluation; "
                         "give both")
    if not FLAGS.device_eval:
        return
    if FLAGS.model != "mnist_cnn":
        raise ValueError("--device_eval with --model %s: the ResNet runner has no device inference" % FLAGS.model)
    r2a = FLAGS.replicas_to_aggregate
    if not FLAGS.sync_replicas or (r2a is not None and r2a < num_workers and bool(FLAGS.ps_hosts)):
        raise ValueError("--device_eval in the parameter-server role (--sync_replicas=False, or backup workers with "
                         "--ps_hosts): the variables live on the ps tasks and the worker's engine holds a copy that is "
                         "fetched step by step; evaluate those runs with the host-fed pass")
    if FLAGS.eval_batches < 1 or FLAGS.eval_batch_size < 1:
        raise ValueError("--device_eval: --eval_batches and --eval_batch_size must be >= 1")


def check_ema_flags(num_workers: int) -> None:
    """--ema_decay averages the variables of synchronous all-reduce training, where every worker holds
    them whole. The combinations it does not cover are flag errors, raised before any process group is
    built, not silently unaveraged runs."""
    if FLAGS.ema_decay < 0 or FLAGS.ema_decay >= 1:
        raise ValueError("--ema_decay=%g: must be in (0, 1) (0 = off)" % FLAGS.ema_decay)
    if not FLAGS.ema_decay > 0:
        return
    if not FLAGS.sync_replicas:
        raise ValueError("--ema_decay with --sync_replicas=False: the variables live on the asynchronous parameter "
                         "server, which keeps no averages (follow-up)")
    r2a = FLAGS.replicas_to_aggregate
    if r2a is not None and r2a < num_workers:
        raise ValueError("--ema_decay with backup workers (--replicas_to_aggregate=%d < %d workers): the variables "
                         "live on the accumulator's side, which keeps no averages (follow-up)" % (r2a, num_workers))
    if FLAGS.model != "mnist_cnn":
        raise ValueError("--ema_decay with --model %s: the ResNet runner's bucketed optimizer does not take the "
                         "shadow yet (follow-up; the flat ops do)" % FLAGS.model)
    if "zero" in FLAGS.dp_schedule:
        raise ValueError("--ema_decay with --dp_schedule=%s: under ZeRO-1 each worker would hold only its fc1 shard "
                         "of the averages; use a schedule without ZeRO" % FLAGS.dp_schedule)


def host_identity() -> str:
    """This machine as far as IPC peer memory is concerned: hostname + kernel boot id."""
    import socket

    boot = ""
    try:
        with open("/proc/sys/kernel/random/boot_id") as f:
            boot = f.read().strip()
    except OSError:
        pass
    return f"{socket.gethostname()}|{boot}"


def gpu_ps_capable() -> bool:
    """This task could run its side of the GPU-resident PS (flags + a visible GPU)."""
    return bool(FLAGS.ps_on_gpu and FLAGS.num_gpus > 0 and FLAGS.model == "mnist_cnn" and torch.cuda.is_available())


def agree_gpu_ps(capable: bool, host: str, group=None):
    """All-gather (host identity, capable) over every ps and worker task of ``group``. Returns
    (use the GPU-resident PS, reason if not): yes only if every task is capable and all share one
    host; otherwise every task falls back to the host parameter server -- the same answer on all."""
    rows = [(host, bool(capable))]
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        rows = [None] * dist.get_world_size(group)
        dist.all_gather_object(rows, (host, bool(capable)), group=group)
    if len({h for h, _ in rows}) > 1:
        return False, "tasks on different hosts"
    if not all(c for _, c in rows):
        return False, "a task without a GPU or with --ps_on_gpu=False"
    return True, ""


def _agree_gpu_ps() -> bool:
    ok, why = agree_gpu_ps(gpu_ps_capable(), host_identity())
    if FLAGS.ps_on_gpu and not ok:
        print("%s %d: --ps_on_gpu needs every task on one host with a GPU (%s); using the host parameter server"
              % (FLAGS.job_name, FLAGS.task_index, why))
    return ok


def _set_bn_mode(deterministic: bool) -> None:
    """--bn_deterministic: batch-norm statistics in row mode (fixed summation order). The switch is an
    op of _C.so, which nothing on the path to here has loaded yet: load it first."""
    if deterministic:
        from .. import _native

        _native.ops().set_bn_part_slots(0)


# ---- what the two workers share: the device, the reference's stdout around the training loop ----

def _task_device() -> torch.device:
    """GPU ``task_index % num_gpus`` (made the current device), or the CPU with --num_gpus=0."""
    if FLAGS.num_gpus <= 0:
        return torch.device("cpu")
    torch.cuda.set_device(FLAGS.task_index % FLAGS.num_gpus)
    return torch.device("cuda", FLAGS.task_index % FLAGS.num_gpus)


def _prepare_session(cluster, is_chief: bool, runner, init_fn, broadcast):
    """The Supervisor (mnist_python_m.py:235-253) with its session prepared: the chief initialises or restores,
    then ``broadcast(sv)`` takes the chief's state to every worker."""
    from .supervisor import Supervisor

    sv = Supervisor(is_chief=is_chief, logdir=FLAGS.logdir or tempfile.mkdtemp(), runner=runner, init_fn=init_fn,
                    broadcast_fn=lambda: broadcast(sv), save_model_secs=FLAGS.save_model_secs,
                    save_summaries_secs=FLAGS.save_summaries_secs, recovery_wait_secs=1)
    if is_chief:
        print("Worker %d: Initializing session..." % FLAGS.task_index)
    else:
        print("Worker %d: Waiting for session to be initialized..." % FLAGS.task_index)
    if FLAGS.existing_servers:
        print("Using existing server at: %s" % ("grpc://" + cluster.task_address("worker", FLAGS.task_index)))
    sys.stdout.flush()
    sv.prepare_or_wait_for_session()
    print("Worker %d: Session initialization complete." % FLAGS.task_index)
    return sv


def _training_begins() -> float:
    time_begin = time.time()
    print("Training begins @ %f" % time_begin)
    return time_begin


def _training_ends(time_begin: float, not_training: float = 0.0) -> float:
    """Training time in seconds, without the ``not_training`` ones spent in --eval_at_steps passes."""
    time_end = time.time()
    print("Training ends @ %f" % time_end)
    training_time = time_end - time_begin - not_training
    print("Training elapsed time: %f s" % training_time)
    return training_time


def _validate(eval_batch, batches: Optional[int] = None) -> float:
    """The reference's validation pass (5 x 1000 images, mnist_python_m.py:309-320) over --eval_batches
    batches (or ``batches`` of them); ``eval_batch()`` evaluates the next one -> (images, correct). Returns
    the mean accuracy."""
    accs = []
    for _ in range(FLAGS.eval_batches if batches is None else batches):
        n, correct = eval_batch()
        print("After %d training step(s)", FLAGS.train_steps)  # verbatim reference line (quirk Q3)
        print("Accuracy : %f" % (correct / float(n)))
        accs.append(correct / float(n))
    mean_accuracy = sum(accs) / len(accs) if accs else float("nan")
    print("Mean Accuracy : %f" % mean_accuracy)
    sys.stdout.flush()
    return mean_accuracy


def _leave(server, barrier_group=None) -> int:
    server.mark_done()
    if barrier_group is not None:
        dist.barrier(group=barrier_group)
    server.shutdown()
    return 0


def _resnet_worker(server, cluster, num_workers: int, is_chief: bool) -> int:
    """``--model resnet18|resnet50``: the same cluster roles, stdout and Supervisor services as the MNIST
    path, training the synthetic-ImageNet ResNet family (BASELINE configs 4-5) with synchronous DP --
    bucketed bf16 gradient all-reduce (``--bucket_mb``, default 8) overlapped with the backward, fused
    SGD-momentum (lr = ``--learning_rate``). RCCL between GPUs; the IPC transport when workers share a
    GPU. Synthetic data: one device-resident random ``--image_size``^2 x 3 batch per worker.

    Supervisor (/root/reference/mnist_python_m.py:235-253): the chief restores the newest checkpoint
    in ``--logdir`` or keeps its seeded init, then params, momentum, BN running statistics and the
    global step go to every worker; timed checkpoints (``--save_model_secs``) in the MNIST layout
    (models/resnet.ResNetRunner); after training an inference-mode validation pass over
    ``--eval_batches`` synthetic batches and a final checkpoint."""
    from ..models.resnet import ResNet, ResNetRunner
    from ..parallel.ipc import IpcCollectives, make_ipc_comm
    from ..parallel.transport import devices_shared, make_rccl

    if not FLAGS.sync_replicas or FLAGS.num_gpus <= 0:
        raise ValueError("--model %s: synchronous data parallelism on GPUs only (--num_gpus > 0)" % FLAGS.model)
    _set_bn_mode(FLAGS.bn_deterministic)
    device = _task_device()
    depth = int(FLAGS.model.replace("resnet", ""))
    m = ResNet(depth, num_classes=1000, device=device, seed=FLAGS.seed)
    runner = ResNetRunner(m)
    comm = None
    grp = server.worker_group
    if num_workers > 1:
        if devices_shared(device, num_workers, grp):
            comm = IpcCollectives(make_ipc_comm(FLAGS.task_index, num_workers, device.index, m.fp.total, group=grp))
        else:
            comm = make_rccl(FLAGS.task_index, num_workers, device.index, group=grp, src=cluster.num_ps)
    m.set_comm(comm, FLAGS.bucket_mb or 8.0)

    def broadcast(sv):  # chief's (restored or seeded) state -> every worker (reference M6)
        if num_workers <= 1:
            return
        for t in [m.fp.master, m.fp.momentum] + [b for bn in m.bns for b in (bn.rmean, bn.rvar)]:
            host = t.detach().cpu()
            dist.broadcast(host, cluster.num_ps, group=grp)
            t.copy_(host.to(device))
        m.fp.shadow.copy_(m.fp.master)
        st = torch.tensor([runner.global_step()], dtype=torch.int64)
        dist.broadcast(st, cluster.num_ps, group=grp)
        runner.set_global_step(int(st.item()))

    sv = _prepare_session(cluster, is_chief, runner, lambda: None, broadcast)
    S = FLAGS.image_size
    g = torch.Generator(device=device).manual_seed(100 + FLAGS.task_index)
    x = torch.randn(FLAGS.batch_size, S, S, 3, device=device, generator=g)
    y = torch.randint(0, 1000, (FLAGS.batch_size,), device=device, generator=g, dtype=torch.int32)
    time_begin = _training_begins()
    local_step = 0
    step = runner.global_step()
    learning_rate = _make_learning_rate()  # a float or a schedule of the runner's global_step
    runner.learning_rate = learning_rate   # the Supervisor's learning_rate summary scalar
    while step < FLAGS.train_steps:
        loss = runner.train_step(x, y, lr=learning_rate)
        step = runner.global_step()
        local_step += 1
        if not FLAGS.quiet:
            print("%f: Worker %d: training step %d done (global step: %d) loss %.4f" % (
                time.time(), FLAGS.task_index, local_step, step, float(loss)))
        sv.on_step(step)
    torch.cuda.synchronize(device)
    el = _training_ends(time_begin)
    print("Worker %d: %.1f images/sec (this worker)" % (FLAGS.task_index, FLAGS.batch_size * local_step / max(el, 1e-9)))
    # synthetic validation batches of at most --batch_size images through the inference-mode network
    # (running BN statistics)
    gv = torch.Generator(device=device).manual_seed(7 + FLAGS.task_index)
    nb = min(FLAGS.eval_batch_size, FLAGS.batch_size)

    def eval_batch():
        vx = torch.randn(nb, S, S, 3, device=device, generator=gv)
        vy = torch.randint(0, 1000, (nb,), device=device, generator=gv, dtype=torch.int32)
        return nb, m.evaluate(vx, vy)[1]

    _validate(eval_batch)
    if num_workers > 1:
        dist.barrier(group=grp)
    sv.stop(save=True)
    if isinstance(comm, IpcCollectives):
        if comm.ipc.error():
            raise RuntimeError("IPC collective barrier timed out")
        comm.ipc.close()
    return _leave(server)


# ---- --dp_schedule: which sync DP schedule (parallel/schedule.py) the workers train with ----

def _max_over(group, v: float) -> float:
    t = torch.tensor([float(v)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return float(t.item())


def dp_candidates(device_type: str, dtype: str):
    """The sync DP schedules this worker device can run (parallel/schedule.py), in probe order."""
    if device_type == "cuda":
        # --clip_norm: the global norm needs the whole aggregated gradient on every rank, which the
        # SFB / ZeRO schedules never form (MnistEngine.set_clip_norm)
        # --optimizer=lamb / lars: likewise for the per-variable norms (MnistEngine.set_lamb / set_lars)
        # --grad_accum_steps: the micro-batch gradients are summed whole before the one collective
        # (MnistEngine.set_grad_accum)
        # --skip_nonfinite: the guard reads the whole aggregated gradient (MnistEngine.set_skip_nonfinite)
        if dtype != "bf16" or FLAGS.clip_norm > 0 or FLAGS.optimizer in LAYERWISE_OPTIMIZERS or \
                FLAGS.grad_accum_steps > 1 or FLAGS.skip_nonfinite:
            return ["allreduce"]
        # --ema_decay: under ZeRO-1 a rank would hold only its fc1 shard of the averages (MnistEngine.set_ema)
        return [k for k, v in SCH.MNIST_SCHEDULES.items() if not (FLAGS.ema_decay > 0 and v["zero"])]
    return list(SCH.CPU_SCHEDULES)


def choose_dp_schedule(run_one, rank: int, num_workers: int, device_type: str, group=None, log=None):
    """(schedule, {candidate: ms/step max over workers} or None, how it was chosen).

    ``--dp_schedule=auto`` with more than one candidate: every worker times every candidate with
    ``run_one(name)`` (same names, same order), the slowest worker's time counts and all keep the
    fastest -- the same in-job probe as bench.py (parallel/schedule.py). The reference has one
    schedule, the PS star (/root/reference/mnist_python_m.py:177,210-233)."""
    known = dp_candidates(device_type, FLAGS.dtype)
    want = FLAGS.dp_schedule
    if want == "fixed":
        return known[0], None, "fixed"
    if want != "auto":
        if want not in known:
            raise ValueError("--dp_schedule=%s: not a %s schedule (known: %s)" % (want, device_type, ", ".join(known)))
        return want, None, "flag"
    if num_workers <= 1 or len(known) == 1:
        return known[0], None, "only"
    times = SCH.probe(known, run_one, lambda v: _max_over(group, v), log)
    return SCH.pick(times), times, "probe"


def _timed_probe(name, group, setup, warmup, timed, teardown) -> float:
    """The probe protocol of parallel/schedule.py over the workers' Gloo group."""
    return SCH.timed_probe(setup, warmup, timed, teardown, max_over_ranks=lambda v: _max_over(group, v),
                           barrier=lambda: dist.barrier(group=group), what="schedule probe %s" % name)


def _probe_gpu_schedule(name, mnist, device, num_workers, group, src, comm):
    """Local ms/step of one GPU DP schedule: a throwaway engine + transport on the worker's device,
    chief-style init, the device-resident split, --dp_probe_warmup untimed then --dp_probe_steps
    timed graph replays."""
    from ..models.mnist_runner import make_runner
    from ..parallel.transport import attach_schedule

    r = None

    def setup():
        nonlocal r
        r = make_runner(FLAGS.batch_size, _make_optimizer(), device, keep_prob=FLAGS.keep_prob, seed=FLAGS.seed,
                        rank=FLAGS.task_index, bf16_grads=FLAGS.bf16_grads, use_graph=True, dtype=FLAGS.dtype)
        attach_schedule(r, name, FLAGS.task_index, num_workers, device, group=group, src=src,
                        mode=FLAGS.dp_transport, comm=comm, bf16=FLAGS.bf16_grads, dtype=FLAGS.dtype)
        r.set_device_dataset(mnist.train.images, mnist.train.labels, seed=FLAGS.seed * 1000 + FLAGS.task_index + 31)
        r.load_flat(M.flat_from_dict(M.init_params(FLAGS.seed)), {}, 0)

    def replay(n: int, eager_first: bool = False):
        try:
            if eager_first:
                r.train_step(None, None)  # eager step + capture of the step graph
            with torch.cuda.stream(r.stream):
                r.eng.replay("train", n)
        finally:  # raised or not, the device is idle when the section ends
            torch.cuda.synchronize(device)

    def timed():
        n = max(1, FLAGS.dp_probe_steps)
        t0 = time.perf_counter()
        replay(n)
        dt = time.perf_counter() - t0
        r.transport.check("schedule probe %s" % name)  # an IPC barrier timeout is a failed candidate
        return dt * 1e3 / n

    def teardown():
        if r is not None:
            r.eng.drop_graph("train")
            if r.transport is not None:
                r.transport.close()

    return _timed_probe(name, group, setup, lambda: replay(max(1, FLAGS.dp_probe_warmup), eager_first=True), timed,
                        teardown)


def _probe_cpu_schedule(name, num_workers, group):
    """Local ms/step of one Gloo schedule on the CPU runner (random batch, 1 + min(5, steps) steps)."""
    from ..models.mnist_runner import TorchMnistRunner
    from ..parallel.sync_replicas import GlooGradAverager

    r = x = y = None

    def setup():
        nonlocal r, x, y
        r = TorchMnistRunner(FLAGS.batch_size, _make_optimizer(), FLAGS.keep_prob, FLAGS.seed, FLAGS.task_index)
        r.load_flat(M.flat_from_dict(M.init_params(FLAGS.seed)), {}, 0)
        r.comm = GlooGradAverager(group, num_workers, [M.BUCKET_SPLIT] if name == "buckets" else None)
        g = torch.Generator().manual_seed(FLAGS.task_index + 5)
        rows = FLAGS.batch_size * FLAGS.grad_accum_steps  # one step's rows
        x = torch.rand(rows, 784, generator=g)
        y = torch.randint(0, 10, (rows,), generator=g)

    def timed():
        n = max(1, min(FLAGS.dp_probe_steps, 5))
        t0 = time.perf_counter()
        for _ in range(n):
            r.train_step(x, y)
        return (time.perf_counter() - t0) * 1e3 / n

    return _timed_probe(name, group, setup, lambda: r.train_step(x, y), timed, lambda: None)


def _choose_schedule(server, cluster, mnist, device, is_chief):
    """All-reduce DP with more than one worker: which schedule -- probed in-job by every worker, or
    fixed by --dp_schedule. One RCCL communicator serves every probe and the training run.
    -> (schedule, {candidate: ms/step} or None, how it was chosen, the RCCL communicator or None)."""
    num_workers, grp, rccl = cluster.num_workers, server.worker_group, None
    if device.type == "cuda":
        from ..parallel.transport import devices_shared, make_rccl

        if FLAGS.dp_transport != "ipc" and not devices_shared(device, num_workers, grp):
            rccl = make_rccl(FLAGS.task_index, num_workers, device.index or 0, group=grp, src=cluster.num_ps)
        run_one = lambda name: _probe_gpu_schedule(name, mnist, device, num_workers, grp,  # noqa: E731
                                                   cluster.num_ps, rccl)
    else:
        run_one = lambda name: _probe_cpu_schedule(name, num_workers, grp)  # noqa: E731
    log = (lambda m: print(m, file=sys.stderr, flush=True)) if is_chief else None
    if is_chief and device.type == "cuda" and FLAGS.clip_norm > 0:
        print("Worker %d: --clip_norm clips the all-reduced gradient: DP schedule candidates restricted to allreduce"
              % FLAGS.task_index)
    if is_chief and device.type == "cuda" and FLAGS.optimizer in LAYERWISE_OPTIMIZERS:
        print("Worker %d: --optimizer=%s takes per-variable norms of the all-reduced gradient: DP schedule candidates "
              "restricted to allreduce" % (FLAGS.task_index, FLAGS.optimizer))
    dp_sched, dp_probe, dp_source = choose_dp_schedule(run_one, FLAGS.task_index, num_workers, device.type, grp, log)
    if is_chief:
        print("Worker %d: DP schedule %s (%s%s)" % (
            FLAGS.task_index, dp_sched, dp_source,
            (": " + ", ".join("%s %.4f ms/step" % kv for kv in dp_probe.items())) if dp_probe else ""))
    return dp_sched, dp_probe, dp_source, rccl


# ---- the roles ----

class Roles(NamedTuple):
    """How this job synchronises gradients, resolved once from the flags and the cluster (the same on
    every task). ``ps_mode`` false: all-reduce DP (parallel/sync_replicas.py)."""
    sync: bool        # --sync_replicas
    r2a: int          # replicas to aggregate per update, at most the number of workers
    backup_ps: bool   # backup workers (R < N) with a ps task: TF's accumulator semantics on the PS (stale
    #                   gradients of stragglers dropped, the first R fresh ones averaged); without a ps task:
    #                   the all-gather stepper
    ps_mode: bool     # the variables live on the ps tasks: async, or backup_ps
    use_gpu_ps: bool  # ... on the ps tasks' GPUs (parallel/gpu_ps.py)


def _resolve_roles(num_workers: int, has_ps: bool) -> Roles:
    sync = FLAGS.sync_replicas
    r2a = num_workers
    if sync:
        r2a = FLAGS.replicas_to_aggregate if FLAGS.replicas_to_aggregate is not None else num_workers
        if r2a > num_workers:
            # TF1 would wait forever for gradients that never come; clamp instead (and say so)
            print("Worker %d: replicas_to_aggregate=%d > %d workers; aggregating %d" %
                  (FLAGS.task_index, r2a, num_workers, num_workers))
            r2a = num_workers
    backup_ps = sync and r2a < num_workers and has_ps
    ps_mode = (not sync) or backup_ps
    # GPU-resident PS only when EVERY task (ps and worker) can take part: same host (the data path is
    # IPC peer memory) and a GPU on each. Decided collectively so the PS and the workers never pick
    # different protocols (the reference's default cluster spans three hosts, mnist_python_m.py:81-84).
    return Roles(sync, r2a, backup_ps, ps_mode, ps_mode and _agree_gpu_ps())


def main(argv=None) -> int:
    from ..parallel.cluster import ClusterSpec, Server
    from ..utils import input_data

    if FLAGS.download_only:
        # no network on MI355X boxes: materialise the IDX files (synthetic if absent) and stop
        print("MNIST data in %s: %s" % (FLAGS.data_dir, input_data.maybe_download(FLAGS.data_dir)))
        sys.exit(0)
    if FLAGS.debug_sync:
        from ..utils.tracing import enable_debug_sync

        enable_debug_sync()
    mnist = input_data.read_data_sets(FLAGS.data_dir, one_hot=True, fake_data=FLAGS.synthetic_data,
                                      seed=FLAGS.seed * 1000 + max(FLAGS.task_index, 0) + 17)

    if FLAGS.job_name is None or FLAGS.job_name == "":
        raise ValueError("Must specify an explicit `job_name`")
    if FLAGS.task_index is None or FLAGS.task_index == "":
        raise ValueError("Must specify an explicit `task_index`")

    check_clip_norm_flags(len(FLAGS.worker_hosts.split(",")))
    check_grad_accum_flags(len(FLAGS.worker_hosts.split(",")))
    check_layerwise_flags(len(FLAGS.worker_hosts.split(",")))
    check_rules_flags(len(FLAGS.worker_hosts.split(",")))
    check_ema_flags(len(FLAGS.worker_hosts.split(",")))
    check_skip_nonfinite_flags(len(FLAGS.worker_hosts.split(",")))
    check_steps_per_call_flags(len(FLAGS.worker_hosts.split(",")))
    check_device_eval_flags(len(FLAGS.worker_hosts.split(",")))

    print("job name = %s" % FLAGS.job_name)
    print("task index = %d" % FLAGS.task_index)

    cluster = ClusterSpec({"ps": FLAGS.ps_hosts.split(","), "worker": FLAGS.worker_hosts.split(",")})
    server = Server(cluster, job_name=FLAGS.job_name, task_index=FLAGS.task_index,
                    existing_servers=FLAGS.existing_servers, timeout_s=FLAGS.rendezvous_timeout)
    opt = _make_optimizer()
    layout = async_ps.mnist_layout(cluster.num_ps) if cluster.num_ps else None
    if not FLAGS.sync_replicas and layout is None:
        raise ValueError("--sync_replicas=False (async parameter-server mode) needs at least one --ps_hosts task")
    roles = _resolve_roles(cluster.num_workers, layout is not None)
    if FLAGS.job_name == "ps":
        return _run_ps(server, cluster, roles, layout, opt)
    if FLAGS.model != "mnist_cnn":
        return _resnet_worker(server, cluster, cluster.num_workers, FLAGS.task_index == 0)
    return _mnist_worker(server, cluster, roles, layout, opt, mnist)


def _run_ps(server, cluster, roles: Roles, layout, opt) -> int:
    """(reference quirk Q9: ps + existing_servers fell through to the worker code; a PS here always
    serves and then exits once every worker has finished)"""
    service = None
    if roles.use_gpu_ps:
        from ..parallel.gpu_ps import GpuParameterServerService

        service = GpuParameterServerService(FLAGS.task_index, cluster.num_ps, cluster.num_workers, layout, opt,
                                            _task_device(), sync=roles.backup_ps, replicas_to_aggregate=roles.r2a)
    elif roles.ps_mode:
        service = async_ps.ParameterServerService(FLAGS.task_index, cluster.num_ps, cluster.num_workers, layout, opt,
                                                  sync=roles.backup_ps, replicas_to_aggregate=roles.r2a)
    server.join(service)
    server.shutdown()
    if service is not None and roles.backup_ps:
        print("ps %d: %d synchronous updates, %d stale gradients dropped" % (FLAGS.task_index, service.updates,
                                                                           service.dropped))
    return 0


def _log_device_placement(gsync, cluster, device) -> None:
    """--log_device_placement: where every variable and the compute live."""
    names = ["global_step"] + [tf for _, tf, _ in M.PARAM_SPECS]
    wdev = "/job:worker/task:%d/%s:%d" % (FLAGS.task_index, "gpu" if device.type == "cuda" else "cpu",
                                          device.index or 0)
    placed = gsync.placement(cluster, names, wdev)
    for n in names:
        print("%s: %s" % (n, placed[n]))
    print("compute (conv_net, loss, gradients): %s; gradient sync: %s" % (wdev, gsync.describe()))


def _mnist_worker(server, cluster, roles: Roles, layout, opt, mnist) -> int:
    from ..models.mnist_runner import make_runner
    from ..utils.metrics import MetricsLogger, StepTimer, performance_table
    from ..utils.tracing import Watchdog, trace_range
    from . import inference
    from .grad_sync import make_grad_sync
    from .optimizers import ExponentialMovingAverage, SyncReplicasOptimizer, ema_decay_at, lr_at
    from .step_calls import call_lengths, multiples

    sync, num_workers, is_chief = roles.sync, cluster.num_workers, FLAGS.task_index == 0
    learning_rate = opt.learning_rate  # a float, or a schedule of global_step
    device = _task_device()
    if sync:  # tf.train.SyncReplicasOptimizer's check of 1 <= replicas_to_aggregate <= total_num_replicas
        va = ExponentialMovingAverage(opt.ema_decay, opt.ema_num_updates) if opt.ema_decay else None
        SyncReplicasOptimizer(opt, replicas_to_aggregate=roles.r2a, total_num_replicas=num_workers,
                              variable_averages=va, skip_nonfinite=bool(opt.skip_nonfinite)).resolve(num_workers)

    dp_sched = dp_probe = dp_source = rccl = None
    if sync and num_workers > 1 and not roles.ps_mode:
        dp_sched, dp_probe, dp_source, rccl = _choose_schedule(server, cluster, mnist, device, is_chief)
    # the R < N all-gather stepper (backup workers without a ps task) steps eagerly
    runner = make_runner(FLAGS.batch_size, opt, device, keep_prob=FLAGS.keep_prob, seed=FLAGS.seed,
                         rank=FLAGS.task_index, comm=None, bf16_grads=FLAGS.bf16_grads,
                         use_graph=FLAGS.use_graph and (roles.ps_mode or roles.r2a >= num_workers), dtype=FLAGS.dtype)
    if dp_sched is not None and device.type == "cuda":
        from ..parallel.transport import attach_schedule

        attach_schedule(runner, dp_sched, FLAGS.task_index, num_workers, device, group=server.worker_group,
                        src=cluster.num_ps, mode=FLAGS.dp_transport, comm=rccl, bf16=FLAGS.bf16_grads,
                        dtype=FLAGS.dtype)
    transport = getattr(runner, "transport", None)  # the GPU all-reduce DP transport (RCCL / IPC)
    zero = transport is not None and transport.zero
    gsync = make_grad_sync(runner, cluster, roles, layout, opt, server.worker_group, dp_sched)
    device_input = device.type == "cuda" and FLAGS.device_input and gsync.device_input
    if device_input:
        runner.set_device_dataset(mnist.train.images, mnist.train.labels,
                                  seed=FLAGS.seed * 1000 + FLAGS.task_index + 31)

    sv = _prepare_session(cluster, is_chief, runner,
                          lambda: runner.load_flat(M.flat_from_dict(M.init_params(FLAGS.seed)), {}, 0), gsync.broadcast)
    if FLAGS.log_device_placement:
        _log_device_placement(gsync, cluster, device)

    eval_at = sorted(int(v) for v in FLAGS.eval_at_steps.split(",") if v.strip()) if FLAGS.eval_at_steps else []
    eval_time, perf_rows = 0.0, []
    metrics = MetricsLogger(FLAGS.metrics_file if is_chief else "")
    if dp_sched is not None:
        metrics.log(event="dp_schedule", chosen=dp_sched, source=dp_source,
                    candidates_ms_per_step=({k: round(v, 5) for k, v in dp_probe.items()} if dp_probe else None))
    phase_timing = FLAGS.phase_timing or (is_chief and bool(FLAGS.metrics_file))
    if phase_timing:
        runner.set_phase_timing(True)
    timer = StepTimer(pid=FLAGS.task_index, enabled=bool(FLAGS.trace_file))
    restart_attempt = int(os.environ.get("TFD_RESTART_COUNT", "0"))
    dp_comm = transport.comm if transport is not None else None  # RCCL; the IPC transport has nothing to abort
    watchdog = Watchdog(FLAGS.step_timeout_secs, on_timeout=(dp_comm.abort if dp_comm is not None else None))

    ema_eval = bool(opt.ema_decay) and FLAGS.ema_eval  # evaluation reads the averages
    if is_chief and opt.ema_decay:
        print("Worker %d: moving averages of the variables, decay %g%s; evaluation reads the %s" % (
            FLAGS.task_index, opt.ema_decay, " (num_updates = global_step)" if opt.ema_num_updates else "",
            "averages" if ema_eval else "variables"))

    # --grad_accum_steps: --batch_size stays the micro-batch (the engine batch); a step draws accum of them
    accum = int(getattr(opt, "accum_steps", 1))
    step_rows = FLAGS.batch_size * accum
    if is_chief and accum > 1:
        print("Worker %d: gradient accumulation, %d micro-batches of %d per optimizer step: %d images per step over "
              "%d worker(s); steps are optimizer steps" % (FLAGS.task_index, accum, FLAGS.batch_size,
                                                          step_rows * (num_workers if sync else 1), num_workers))

    def eval_batch():
        val_x, val_y = mnist.validation.next_batch(FLAGS.eval_batch_size)
        return len(val_x), runner.evaluate(val_x, val_y, use_ema=ema_eval)[1]

    eval_rows = min(FLAGS.eval_batches * FLAGS.eval_batch_size, mnist.validation.num_examples)
    if FLAGS.device_eval:
        runner.set_eval_dataset(mnist.validation.images, mnist.validation.labels)  # uploaded once

    def eval_pass():
        """One validation pass -> [(images, correct)] per batch and, with --device_eval, its records."""
        if not FLAGS.device_eval:
            return [eval_batch() for _ in range(FLAGS.eval_batches)], None
        recs = runner.evaluate_dataset(0, eval_rows, FLAGS.eval_batch_size, use_ema=ema_eval)
        return [(r["rows"], r["correct"]) for r in recs], recs

    def after_step(step: int, local_step: int) -> None:
        """What follows a step -- or, with --steps_per_call, a call's last step -- on the host."""
        nonlocal eval_time
        if FLAGS.check_consistency_every and sync and local_step % FLAGS.check_consistency_every == 0:
            if zero:
                runner.sync_state()  # every worker: the fc1 shards -> whole fp32 state
            _check_consistency(runner, server, num_workers)
        if zero:
            # the fp32 fc1 master and its Adam slots are sharded over the workers: the chief's timed
            # checkpoint needs a gather that every worker joins, at agreed global steps
            save_now = False
            if step % max(1, FLAGS.zero_sync_every) == 0:
                due = torch.tensor([1 if sv.save_due() else 0], dtype=torch.int64)
                dist.all_reduce(due, op=dist.ReduceOp.MAX, group=server.worker_group)
                save_now = bool(due.item())
                if save_now:
                    runner.sync_state()
            sv.on_step(step, allow_save=save_now)
        else:
            sv.on_step(step)
        while is_chief and eval_at and step >= eval_at[0]:
            te = time.time()
            accs = [correct / float(n) for n, correct in eval_pass()[0]]
            acc = 100.0 * sum(accs) / len(accs)
            eval_time += time.time() - te
            row = dict(steps=eval_at.pop(0), time=time.time() - time_begin - eval_time, accuracy=round(acc, 2),
                       lr=lr_at(learning_rate, step))
            perf_rows.append(row)
            print("Performance row: %d %.1f %.2f %g" % (row["steps"], row["time"], row["accuracy"], row["lr"]))
            metrics.log(event="performance", **row)
        if (FLAGS.fault_inject_step >= 0 and FLAGS.task_index == FLAGS.fault_inject_task and restart_attempt == 0
                and step >= FLAGS.fault_inject_step):
            print("Worker %d: fault injection at global step %d" % (FLAGS.task_index, step), flush=True)
            os._exit(17)

    time_begin = _training_begins()
    local_step = 0
    step = runner.global_step()
    if FLAGS.steps_per_call > 1:
        # N steps per host round trip: one replayed N-step graph, then one read of the device step log. Every
        # rank forms the same call lengths from the same flags (the collectives are inside the graphs).
        assert device_input and not roles.ps_mode and roles.r2a >= num_workers, "--steps_per_call: check_steps_per_call_flags"
        runner.set_step_log(1024)
        cuts = list(eval_at) + multiples(FLAGS.check_consistency_every if sync else 0, step, FLAGS.train_steps, origin=step)
        if FLAGS.fault_inject_step >= 0:
            cuts.append(FLAGS.fault_inject_step)
        if zero:  # the workers agree on the chief's checkpoint at these global steps
            cuts += multiples(max(1, FLAGS.zero_sync_every), step, FLAGS.train_steps)
        skipped = runner.skipped_steps() if opt.skip_nonfinite else 0
        for k in call_lengths(step, FLAGS.steps_per_call, FLAGS.train_steps, cuts):
            t0 = time.time()
            with timer.phase("step"), trace_range("train_steps"):
                runner.train_steps(k)
                recs = runner.read_step_log(step + 1, step + k)  # the call's one synchronisation
            watchdog.kick()
            now = time.time()
            step_s = max(now - t0, 1e-9) / k
            for i, r in enumerate(recs):
                last = i == k - 1
                local_step += 1
                skipped += 0 if r["ok"] else 1
                if not FLAGS.quiet:
                    print("%f: Worker %d: training step %d done (global step: %d)" % (now, FLAGS.task_index, local_step,
                                                                                      r["step"]))
                if not metrics.path:
                    continue
                rec = dict(step=local_step, global_step=r["step"], step_ms=1e3 * step_s, loss=r["loss"],
                           images_per_sec=step_rows * (num_workers if sync else 1) / step_s, accum_steps=accum,
                           steps_in_call=k, train_accuracy=r["correct"] / float(r["rows"]))
                if gsync.logs_lr:
                    rec["lr"] = r["lr"]
                if FLAGS.clip_norm > 0:
                    rec["grad_norm"], rec["clip_scale"] = r["grad_norm"], r["clip_scale"]
                if last and FLAGS.optimizer in LAYERWISE_OPTIMIZERS:
                    rec["trust_ratio"] = {k_: v[2] for k_, v in runner.last_layer_norms().items()}
                if opt.skip_nonfinite:
                    rec["skipped_steps"], rec["step_ok"] = skipped, r["ok"]
                if opt.ema_decay:
                    rec["ema_decay"] = ema_decay_at(opt.ema_decay, r["step"], opt.ema_num_updates)
                if last and phase_timing:
                    ph = runner.phase_times()
                    rec.update(ph)
                    timer.add_gpu_phases(now, ph)
                rec.setdefault("allreduce_ms", 0.0 if (not sync or num_workers == 1) else None)
                metrics.log(**rec)
            step += k
            if opt.skip_nonfinite:
                assert skipped == runner.skipped_steps(), "step log: %d skipped steps counted from the records, " \
                    "the device counter says %d" % (skipped, runner.skipped_steps())
            after_step(step, local_step)
    while step < FLAGS.train_steps:
        with timer.phase("input"):
            if device_input:
                batch_xs = batch_ys = None  # the engine gathers the batch on the device
            else:
                batch_xs, batch_ys = mnist.train.next_batch(step_rows)
        t0 = time.time()
        with timer.phase("step"), trace_range("train_step"):
            step = gsync.step(batch_xs, batch_ys, step)
        local_step += 1
        watchdog.kick()
        now = time.time()
        if not FLAGS.quiet:
            print("%f: Worker %d: training step %d done (global step: %d)" % (now, FLAGS.task_index, local_step, step))
            if gsync.last_dropped:
                print("Worker %d: stale gradient dropped (a backup replica finished this step first)" % FLAGS.task_index)
        if metrics.path:
            rec = dict(step=local_step, global_step=step, step_ms=1e3 * (now - t0), loss=runner.last_loss(),
                       images_per_sec=step_rows * (num_workers if sync else 1) / max(now - t0, 1e-9),
                       accum_steps=accum)
            if gsync.logs_lr:
                rec["lr"] = lr_at(learning_rate, max(step - 1, 0))
            if FLAGS.clip_norm > 0:
                rec["grad_norm"], rec["clip_scale"] = runner.last_grad_norm()
            if FLAGS.optimizer in LAYERWISE_OPTIMIZERS:
                rec["trust_ratio"] = {k: v[2] for k, v in runner.last_layer_norms().items()}
            if opt.skip_nonfinite:  # cumulative count, and whether this step's update was applied
                rec["skipped_steps"], rec["step_ok"] = runner.skipped_steps(), runner.last_step_ok()
            if opt.ema_decay:  # d_t of this step's update (host mirror)
                rec["ema_decay"] = ema_decay_at(opt.ema_decay, step, opt.ema_num_updates)
            if phase_timing:
                ph = runner.phase_times()
                rec.update(ph)
                timer.add_gpu_phases(now, ph)
            rec.setdefault("allreduce_ms", 0.0 if (not sync or num_workers == 1) else None)
            metrics.log(**rec)
        after_step(step, local_step)

    watchdog.stop()
    if zero:
        runner.sync_state()  # whole replicas again: final checksum, eval and the chief's last checkpoint
    if FLAGS.check_consistency_every and sync:
        print("Worker %d: parameter checksum %.17g %.17g" % ((FLAGS.task_index,) + _param_checksum(runner)))
    if transport is not None:
        transport.check("training")  # a timed-out IPC barrier must not pass as a finished run
    training_time = _training_ends(time_begin, eval_time)
    print("Worker %d: %.1f images/sec (%d optimizer steps of %d images)" % (
        FLAGS.task_index, step_rows * (num_workers if sync else 1) * local_step / max(training_time, 1e-9), local_step,
        step_rows * (num_workers if sync else 1)))
    if FLAGS.device_eval:
        batches, recs = eval_pass()
        mean_accuracy = _validate(iter(batches).__next__, len(batches))
        whole = inference.merge_records(recs)
        evaluation = dict(event="evaluation", global_step=step, rows=whole["rows"], correct=whole["correct"],
                          loss=whole["loss_sum"] / max(whole["rows"], 1), mean_accuracy=mean_accuracy)
        if FLAGS.confusion_matrix:
            print(inference.format_confusion(whole["confusion"]))
            evaluation.update(confusion=whole["confusion"].tolist(),
                              per_class_recall=[None if r != r else round(float(r), 6)
                                                for r in inference.per_class_recall(whole["confusion"])])
        metrics.log(**evaluation)
    else:
        mean_accuracy = _validate(eval_batch)
    skipped = runner.skipped_steps() if opt.skip_nonfinite else 0
    if skipped > 0:
        print("Worker %d: --skip_nonfinite skipped %d of %d optimizer steps (aggregated gradient not finite)"
              % (FLAGS.task_index, skipped, local_step))
    metrics.log(event="final", global_step=step, training_time_s=training_time, mean_accuracy=mean_accuracy,
                **({"skipped_steps": skipped} if opt.skip_nonfinite else {}))
    if perf_rows:
        print(performance_table(perf_rows), end="")
    metrics.close()
    if FLAGS.trace_file:
        timer.write_chrome_trace(FLAGS.trace_file.replace("{task}", str(FLAGS.task_index)))
    sv.stop(save=True)
    gsync.close()
    if transport is not None:
        transport.close()
    return _leave(server, server.worker_group if sync and num_workers > 1 else None)


def _param_checksum(runner):
    """(sum, sum of squares) of the parameters in fp64."""
    p = runner.params().detach().double()
    return float(p.sum().item()), float((p * p).sum().item())


def _check_consistency(runner, server, num_workers):
    """Race/desync detector: max |checksum_i - checksum_0| across workers."""
    cs = torch.tensor(_param_checksum(runner), dtype=torch.float64)
    mx, mn = cs.clone(), cs.clone()
    dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=server.worker_group)
    dist.all_reduce(mn, op=dist.ReduceOp.MIN, group=server.worker_group)
    if not torch.equal(mx, mn):
        raise RuntimeError(f"worker parameter desync detected: checksum range {mn.tolist()} .. {mx.tolist()}")


def run_script(task_index_default: int, job_name_default: str, argv=None) -> int:
    define_flags(task_index_default, job_name_default)
    argv = list(sys.argv if argv is None else argv)
    if "--help" in argv or "-h" in argv:
        print(f"usage: {argv[0]} [flags]\n{FLAGS.help_text()}")
        return 0
    FLAGS.parse(argv)
    return main(argv) or 0

