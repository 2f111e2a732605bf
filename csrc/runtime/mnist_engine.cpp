// Native train-step executor for the reference MNIST CNN.
//
// Plays the role of the TF1 graph executor + Session.run for the reference's hot loop
// (the reference's mnist_python_m.py:289-302, mnist_single.py:109-117): it owns every device
// buffer (flat fp32 master params, bf16 shadow, flat grads, Adam slots, activations), sequences
// the fused HIP kernels of csrc/kernels/mnist.hip, overlaps the bucketed RCCL gradient all-reduce
// with the conv backward on a second stream, applies the fused flat optimizer, and can capture the
// whole step (both streams, collectives included) into one hipGraph that is replayed per step.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/custom_class.h>
#include <torch/library.h>

#include <algorithm>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../ema.h"
#include "../grad_accum.h"
#include "../layerwise_kernels.h"
#include "../mnist_infer.h"
#include "../mnist_layout.h"
#include "../optim_launch.h"
#include "../optim_rules.h"
#include "../step_log.h"
#include "../tfd_kernels.h"
#include "comm.h"
#include "hip_util.h"
#include "ipc_comm.h"

namespace tfd {
using namespace mnist;

class MnistEngine : public torch::CustomClassHolder {
  // the update rule (not part of the torch class); LAMB runs on Adam's settings and slots, LARS on Momentum's
  enum class OptKind { Adam, Sgd, Momentum, RmsProp, Adagrad };
  enum class LwKind { None, Lamb, Lars };
 public:
  MnistEngine(int64_t batch, int64_t device, double keep_prob, int64_t seed, int64_t rank)
      : B_(batch), device_(device), keep_prob_(keep_prob), seed_((uint32_t)seed), rank_((uint32_t)rank) {
    // the output-layer gradient blocks stage dlogits [B][10] in LDS: above mnist_max_batch() their
    // launch would be refused (both precisions: set_dtype comes after construction)
    TORCH_CHECK(batch > 0 && batch <= mnist_max_batch(), "MnistEngine: batch ", batch,
                " outside [1, mnist_max_batch() = ", mnist_max_batch(), "]");
    auto f32 = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device);
    auto bf = at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA, device);
    auto u8 = at::TensorOptions().dtype(at::kByte).device(at::kCUDA, device);
    auto i64 = at::TensorOptions().dtype(at::kLong).device(at::kCUDA, device);
    auto i32 = at::TensorOptions().dtype(at::kInt).device(at::kCUDA, device);
    params_ = at::zeros({TOTAL}, f32);
    pbf_ = at::zeros({TOTAL}, bf);
    grad_ = at::zeros({TOTAL}, f32);
    m_ = at::zeros({TOTAL}, f32);
    v_ = at::zeros({TOTAL}, f32);
    gbf_ = at::zeros({TOTAL}, bf);
    step_ = at::zeros({1}, i64);
    tnext_ = at::zeros({1}, i64);
    // {norm, scale} of the last clipped step (set_clip_norm), then ok of the non-finite guard
    // (set_skip_nonfinite) and its device counter of skipped steps
    gnorm_ = at::zeros({3}, f32);
    gnorm_[1] = 1.0;
    gnorm_[2] = 1.0;
    skipped_ = at::zeros({1}, i64);
    // OptMods::one (optim_launch.h); copied from the host: ready whichever stream the first step runs on
    one_ = at::ones({1}, at::kFloat).to(params_.device());
    gpart_ = at::zeros({kGradNormMaxBlocks}, f32);
    fc1_splits_ = mnist_fc1_splits((int)B_);
    wg2_splits_ = mnist_wg2_splits((int)B_);
    p1_ = at::empty({B_, P1H, P1H, C1}, bf);
    idx1_ = at::empty({B_, P1H, P1H, C1}, u8);
    p2_ = at::empty({B_, FEAT}, bf);
    idx2_ = at::empty({B_, FEAT}, u8);
    fc1_slab_ = at::empty({fc1_splits_, B_, HID}, f32);
    hd_ = at::empty({B_, HID}, bf);
    dh_ = at::empty({B_, HID}, bf);
    dlogits_ = at::empty({B_, NCLS}, f32);
    loss_row_ = at::zeros({B_}, f32);
    correct_row_ = at::zeros({B_}, f32);
    dz2_ = at::empty({B_, P1H, P1H, C2}, bf);
    wg2_slab_ = at::empty({wg2_splits_, 801, C2}, f32);
    wg1_slab_ = at::empty({2 * B_, 832}, f32);
    xbuf_ = at::zeros({B_, 784}, f32);
    rows_ = at::full({B_ + 1}, -1, i32);  // prefetched batch rows + step tag (MnistStepArgs::rows)
    xpre_ = at::zeros({B_, 784}, f32);    // prefetched next batch (MnistStepArgs::xpre / ypre)
    ypre_ = at::zeros({B_}, i32);
    ybuf_ = at::zeros({B_}, i32);
    HIP_OK(hipSetDevice((int)device));
    // streams and events belong to `device`, so they are created here and not by member initialisers
    comm_stream_ = HipStream::create();
    opt_stream_ = HipStream::create();
    for (HipEvent* e : {&ev_a_, &ev_b_, &ev_done_, &ev_opt_a_, &ev_start_, &ev_ag_, &ev_p2_, &ev_wag_})
      *e = HipEvent(false);
    for (auto& e : pev_) e = HipEvent(true);  // timing events (phase timer)
  }
  // the graph executables go first; the streams and events they were captured from release themselves
  ~MnistEngine() override {
    for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
  }

  // ---- state accessors (views share storage with the engine) ----
  at::Tensor params() { return params_; }
  at::Tensor params_bf16() { return pbf_; }
  at::Tensor grads() { return grad_; }
  // bf16 gradient buffer: the DP wire format (reduced in place by the bucket all-reduces)
  at::Tensor grads_bf16() { return gbf_; }
  at::Tensor adam_m() { return m_; }
  at::Tensor adam_v() { return v_; }
  // the third slot (centered RMSProp's mg): allocated at the first set_rmsprop(centered = true)
  at::Tensor slot3() {
    TORCH_CHECK(s3_.defined(), "slot3: set_rmsprop(centered = true) first");
    return s3_;
  }
  at::Tensor step_tensor() { return step_; }
  at::Tensor loss_rows() { return loss_row_; }
  at::Tensor correct_rows() { return correct_row_; }
  at::Tensor hidden() {
    if (fp32_) return fhd_;
    if (sfb_active()) return sfdr_.narrow(0, rank_in_comm() * sfb_rs_ + B_ * HID, B_ * HID).view({B_, HID});
    return hd_;
  }
  at::Tensor pool2() {
    if (fp32_) return f2_;
    if (sfb_active()) return sfp2_.narrow(0, rank_in_comm() * B_ * FEAT, B_ * FEAT).view({B_, FEAT});
    return p2_;
  }
  at::Tensor pool1() { return fp32_ ? f1_ : p1_; }
  // read-only views for the tests: each pool's argmax inside its 2x2 window (0..3, row-major; both
  // precisions write the same buffers), the gradient at the logits (1/B folded in) and at the fc1
  // pre-activation
  at::Tensor pool1_argmax() { return idx1_; }
  at::Tensor pool2_argmax() { return idx2_; }
  at::Tensor dlogits() {
    if (!fp32_ && sfb_active())
      return sfdr_.narrow(0, rank_in_comm() * sfb_rs_ + 2 * B_ * HID, 2 * B_ * NCLS).view(at::kFloat).view({B_, NCLS});
    return dlogits_;
  }
  at::Tensor dhidden() {
    if (fp32_) return fdh_;
    if (sfb_active()) return sfdr_.narrow(0, rank_in_comm() * sfb_rs_, B_ * HID).view({B_, HID});
    return dh_;
  }
  at::Tensor feed_x() { return xbuf_; }
  at::Tensor feed_y() { return ybuf_; }
  int64_t batch() { return B_; }
  static int64_t max_batch() { return mnist_max_batch(); }

  // Gradient accumulation: one train_step() is one optimizer step over K micro-batches of B rows
  // (train_step_accum). K = 1 (the default) is off: the step is launch for launch what it was and
  // nothing is allocated. K > 1 allocates, here and never inside a capture, the fp32 accumulator, the
  // device micro-batch counter -- the data cursor, the prefetch tag and the dropout key of the
  // micro-batch kernels, so micro-batch m trains on perm[(m * B + b) % n] and K of them are the rows of
  // one batch of K * B -- and feed buffers of K * B rows (feed_x / feed_y: micro-batch j reads rows
  // [j * B, (j + 1) * B); fetch them again after this call). Sets micro = K * global_step on the current
  // stream; so must whoever writes step_tensor() afterwards (sync_micro_step). loss_rows() /
  // correct_rows() hold the last micro-batch's values; the phase marks between the step's start and end
  // are the last micro-batch's. Graphs captured before a call that changes K are dropped: they point
  // at the buffers of the old K.
  void set_grad_accum(int64_t K) {
    TORCH_CHECK(K >= 1 && K <= 4096, "set_grad_accum: 1 <= K <= 4096, got ", K);
    if (K != accum_) {
      for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
      graphs_.clear();
    }
    if (K > 1 && !acc_.defined()) {
      acc_ = at::empty_like(grad_);  // stored whole by the first micro-batch of every step: never zero-filled
      micro_ = at::zeros({1}, step_.options());
    }
    if (xbuf_.size(0) != K * B_ && (K > 1 || accum_ > 1)) {
      xbuf_ = at::zeros({K * B_, 784}, xbuf_.options());
      ybuf_ = at::zeros({K * B_}, ybuf_.options());
    }
    accum_ = K;
    sync_micro_step();
  }
  int64_t grad_accum() const { return accum_; }
  // the micro-batch counter (K = 1: the step counter itself is the cursor)
  at::Tensor micro_step_tensor() { return micro_.defined() ? micro_ : step_; }
  // micro = K * global_step, on the current stream: after every write of step_tensor()
  void sync_micro_step() {
    if (!micro_.defined()) return;
    micro_.copy_(step_.mul(accum_));
    invalidate_prefetch();
  }

  void set_dataset(at::Tensor data, at::Tensor labels, at::Tensor perm) {
    TORCH_CHECK(data.is_cuda() && data.scalar_type() == at::kFloat && data.dim() == 2 && data.size(1) == 784,
                "dataset must be a [N,784] fp32 GPU tensor");
    TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kInt && labels.numel() == data.size(0),
                "labels must be [N] int32 GPU");
    TORCH_CHECK(perm.is_cuda() && perm.scalar_type() == at::kInt && perm.numel() == data.size(0),
                "perm must be [N] int32 GPU");
    data_ = data.contiguous();
    labels_ = labels.contiguous();
    perm_ = perm.contiguous();
    invalidate_prefetch();
  }
  // the permutation changed (epoch reshuffle): drop the rows prefetched from the old one
  void invalidate_prefetch() { rows_.narrow(0, B_, 1).fill_(-1); }
  // timing-stamp builds (TFD_STAMP): kernels write per-block phase clocks here
  void set_debug_buffer(at::Tensor t) { dbg_ = t; }
  // mode 0 = feed buffers (feed_x/feed_y filled by the host each step), 1 = device dataset + perm
  void set_input_mode(int64_t mode) {
    TORCH_CHECK(mode == 0 || (mode == 1 && data_.defined()), "set_dataset first");
    input_mode_ = mode;
  }
  void set_keep_prob(double kp) { keep_prob_ = kp; }
  void sync_shadow() {
    cast_f32_bf16((const float*)params_.data_ptr(), (uint16_t*)pbf_.data_ptr(), TOTAL, stream());
  }

  void set_adam(double lr, double b1, double b2, double eps) {
    b1_ = b1; b2_ = b2; eps_ = eps;
    set_optimizer(OptKind::Adam, lr);
  }
  void set_momentum(double lr, double momentum, bool nesterov) {
    momentum_ = momentum; nesterov_ = nesterov;
    set_optimizer(momentum > 0 ? OptKind::Momentum : OptKind::Sgd, lr);
  }
  // RMSProp and Adagrad (csrc/optim_rules.h, kernels/optim_rules.hip): one launch over the range, on
  // the unfused step -- the path Momentum takes. Slots: ms / accum in adam_v(), mom in adam_m(), the
  // centered rule's mg in slot3(). The setters fill them with TF's initial values (ms = 1, mom = 0,
  // mg = 0; accum = initial_accumulator_value) by ordinary tensor fills, outside any capture. They
  // compose with set_lr_schedule, set_clip_norm, set_ema, set_skip_nonfinite, set_grad_accum and every DP
  // schedule (ZeRO-1 shards the slots as it shards Adam's). Baked into graphs captured before the call.
  void set_rmsprop(double lr, double decay, double momentum, double eps, bool centered) {
    TORCH_CHECK(decay >= 0 && decay < 1 && momentum >= 0 && eps >= 0, "set_rmsprop: decay in [0, 1), momentum >= 0, eps >= 0");
    rule_decay_ = decay; momentum_ = momentum; rule_eps_ = eps; centered_ = centered;
    nesterov_ = false;
    set_optimizer(OptKind::RmsProp, lr);
    v_.fill_(1.0);
    m_.zero_();
    if (centered) {
      if (!s3_.defined()) s3_ = at::zeros_like(m_);
      else s3_.zero_();
    }
  }
  void set_adagrad(double lr, double initial_accumulator_value) {
    TORCH_CHECK(initial_accumulator_value > 0, "set_adagrad: initial_accumulator_value > 0");
    centered_ = false;
    nesterov_ = false;
    set_optimizer(OptKind::Adagrad, lr);
    v_.fill_(initial_accumulator_value);
  }
  // Layer-wise optimizers (csrc/layerwise.h): every variable's update is scaled by a trust ratio formed
  // from two L2 norms over that variable, taken on the device inside the step (three launches over
  // one block table, kernels/optim_layerwise.hip). LAMB uses the Adam slots (adam_m / adam_v), LARS the
  // momentum slot (adam_m), t = global_step after the update. skip_bias: the four biases take neither
  // the weight decay nor the ratio (LARS's skip_list, LAMB's exclude_from_*). The step is the serial
  // schedule of the clip step; set_clip_norm, set_ema and set_lr_schedule compose with it. set_adam /
  // set_momentum switch back. Baked into graphs captured before the call: capture again.
  void set_lamb(double lr, double b1, double b2, double eps, double weight_decay, bool skip_bias) {
    TORCH_CHECK(weight_decay >= 0, "set_lamb: weight_decay >= 0");
    b1_ = b1; b2_ = b2; eps_ = eps;
    lw_wd_ = weight_decay;
    set_optimizer(OptKind::Adam, lr);
    set_layerwise(LwKind::Lamb, skip_bias);
  }
  void set_lars(double lr, double momentum, double weight_decay, double eeta, double eps, bool skip_bias) {
    TORCH_CHECK(weight_decay >= 0 && eeta > 0 && eps >= 0, "set_lars: weight_decay >= 0, eeta > 0, eps >= 0");
    momentum_ = momentum; nesterov_ = false;
    lw_wd_ = weight_decay; lw_eeta_ = eeta; lw_eps_ = eps;
    set_optimizer(OptKind::Momentum, lr);
    set_layerwise(LwKind::Lars, skip_bias);
  }
  // [8,3] = {|p|, |u| (LAMB) or |g| (LARS), r} of the last layer-wise step, on the device, in the flat
  // layout's order: wc1, bc1, wc2, bc2, wd1, bd1, out, out_b
  at::Tensor layer_norms() {
    TORCH_CHECK(lw_out_.defined(), "layer_norms: set_lamb or set_lars first");
    return lw_out_;
  }
  // Learning rate as a function of global_step (csrc/lr_schedule.h), evaluated by the optimizer
  // kernels from the device step counter: a captured multi-step graph follows it with no host round
  // trip. kind: constant | exponential | piecewise | polynomial | cosine; params = {lr, decay_steps,
  // rate, end, power, alpha, warmup_steps, staircase}. set_adam / set_momentum reset it to constant.
  // Like every optimizer setting it is baked into graphs captured before the call: capture again.
  void set_lr_schedule(std::string kind, std::vector<double> params, std::vector<int64_t> boundaries,
                       std::vector<double> values) {
    try {
      sched_ = make_lr_schedule(kind, params, boundaries, values);
    } catch (const std::invalid_argument& e) {
      TORCH_CHECK(false, e.what());
    }
  }
  // lr the update from global_step = s uses (host evaluation of the same function)
  double lr_at_step(int64_t s) const { return (double)lr_at(sched_, s); }
  // tf.clip_by_global_norm between the gradients and the optimizer, on the device: every step takes
  // norm = ||averaged gradient||_2 (of the buffer the optimizer reads: fp32 grads(), or grads_bf16()
  // when DP all-reduces bf16) and multiplies the gradient by scale = c / max(norm, c), exactly 1 while
  // norm <= c. Non-finite norms get no special handling: inf gives scale 0; a NaN norm leaves scale at 1
  // and the NaN gradients propagate as they do without clipping. c <= 0 turns clipping off (the
  // default: the step is then launch for launch what it was). Like every optimizer setting it is baked
  // into graphs captured before the call: capture again.
  void set_clip_norm(double c) { clip_norm_ = c > 0 ? c : 0.0; }
  double clip_norm() const { return clip_norm_; }
  // {norm, scale} of the last clipped step, on the device ({0, 1} before the first)
  at::Tensor grad_norm() { return gnorm_.narrow(0, 0, 2); }
  // Non-finite guard, off by default. A step whose aggregated gradient is not finite is an identity
  // update: the optimizer kernels return before their first store, so the parameters, the slots, the
  // bf16 shadow and the EMA shadow keep their bits, and a device counter of skipped steps goes up by
  // one. global_step and the micro-step counter advance as on any step -- the data cursor, the dropout
  // key, the schedules, the EMA decay and Adam's t follow them: a skipped step consumes its batch and
  // its t. "Not finite": the fp32 sum of squares of the aggregated gradient (grad_sumsq), finished in
  // fp64 and scaled, is inf or NaN -- any inf / NaN element, and also finite gradients whose norm
  // overflows fp32, which are skipped as well (grad_guard.hip). The step takes the whole-gradient path
  // of set_clip_norm; with the guard on, grad_norm() reports {norm, scale} without clipping too. The
  // counter is a statistic: no state depends on it and it is not checkpointed.
  void set_skip_nonfinite(bool on) { guard_ = on; }
  bool skip_nonfinite() const { return guard_; }
  at::Tensor skipped_steps_tensor() { return skipped_; }
  int64_t skipped_steps() { return skipped_.item<int64_t>(); }
  // whether the last guarded step was applied (true before any)
  bool last_step_ok() { return gnorm_[2].item<float>() != 0.f; }
  // tf.train.ExponentialMovingAverage of the weights (SyncReplicasOptimizer's variable_averages),
  // updated by the optimizer kernels themselves from p' in registers (csrc/ema.h): e' = e - (1 - d_t)
  // (e - p'), d_t = decay or, with num_updates, min(decay, (1 + t) / (10 + t)) from the device step
  // counter, so a captured multi-step graph follows it. Every optimizer launch of every schedule takes
  // its EMA variant; launches, streams and events are what they are without it. decay <= 0 turns it
  // off (the default: nothing is allocated and the step is launch for launch what it was). Switching
  // it on copies the parameters into the shadow (no zero-debias); after writing params() call
  // load_ema(params()) to start the average again. Baked into graphs captured before the call.
  void set_ema(double decay, bool num_updates) {
    TORCH_CHECK(decay == decay && decay < 1.0, "set_ema: decay must be in (0, 1) (<= 0: off), got ", decay);
    if (!(decay > 0)) {
      ema_decay_ = 0.0;
      return;
    }
    if (!ema_.defined()) ema_ = at::empty_like(params_);
    if (!ema_on()) {
      ema_.copy_(params_);
      ema_bf_stale_ = true;
    }
    ema_decay_ = decay;
    ema_nu_ = num_updates;
  }
  double ema_decay() const { return ema_decay_; }
  // d_t of the update that ends at global_step = t (host evaluation of the device function)
  double ema_decay_at_step(int64_t t) const { return (double)ema_decay_at((float)ema_decay_, ema_nu_ ? 1 : 0, t); }
  // the fp32 flat shadow (shares storage with the engine). Like params() it is whole between steps:
  // the deferred fc-region optimizer of the DP step, which writes both, is joined at every step's or
  // graph's end.
  at::Tensor ema_params() {
    TORCH_CHECK(ema_.defined(), "ema_params: set_ema first");
    return ema_;
  }
  void load_ema(at::Tensor t) {
    TORCH_CHECK(ema_.defined(), "load_ema: set_ema first");
    TORCH_CHECK(t.numel() == TOTAL, "load_ema: ", TOTAL, " elements");
    ema_.copy_(t.reshape({TOTAL}));
    ema_bf_stale_ = true;
  }
  void set_comm(c10::intrusive_ptr<RcclComm> comm, bool bf16_grads) {
    comm_ = comm;
    bf16_comm_ = bf16_grads && !fp32_;
  }
  // Peer-to-peer IPC all-reduce for latency-bound buckets (<= small_max elements, e.g. the conv
  // bucket B); without an RCCL communicator it carries every bucket (one-GPU multi-process tests).
  void set_ipc(c10::intrusive_ptr<IpcComm> ipc, int64_t small_max, bool bf16_grads) {
    ipc_ = ipc;
    ipc_small_ = small_max;
    if (!comm_) bf16_comm_ = bf16_grads && !fp32_;
  }
  // Per-path fallback: false = the SFB factor and ZeRO shard all-gathers go through RCCL even when
  // the IPC staging holds them (set when the startup self-check of the IPC gather disagreed with
  // RCCL; parallel/transport.py)
  void set_ipc_gather(bool on) { ipc_gather_ = on; }
  bool ipc_gathers(int64_t shard) const { return ipc_ && ipc_gather_ && ipc_->capacity() * 2 >= shard; }
  int64_t world() const {
    if (comm_) return comm_->world();
    if (ipc_) return ipc_->world();
    return 1;
  }
  // Force the data-parallel schedule (comm stream, bucket casts, captured collectives, 1/N scale)
  // even at world 1: exercises the multi-rank orchestration -- RCCL or IPC -- on a one-GPU box
  // with the exact code an 8-GPU node runs.
  void set_force_dp(bool on) { force_dp_ = on; }
  bool dp() const { return world() > 1 || (force_dp_ && (comm_ || ipc_)); }
  int64_t rank_in_comm() const {
    if (comm_) return comm_->rank();
    if (ipc_) return ipc_->rank();
    return 0;
  }
  // ZeRO-1 for the fc1 weight (98% of the parameters): its gradient is reduce-scattered, each rank
  // runs the optimizer on its 1/N shard (fp32 master + m + v), and the updated bf16 shadow is
  // all-gathered at the start of the next step, overlapping the conv forward. The re-expression of
  // the reference's round-robin parameter sharding across PS tasks.
  void set_zero(bool on) {
    if (!on) { zero_ = false; return; }
    const int64_t W = world();
    // world 1 only as the forced-DP rehearsal (one shard = the whole fc1 weight): the sharded
    // schedule -- reduce-scatter / sharded optimizer / weight all-gather over the real RCCL or IPC
    // communicator -- runs on a one-GPU box exactly as an N-GPU node runs it
    TORCH_CHECK(W > 1 || (force_dp_ && (comm_ || ipc_)), "set_zero: needs a communicator with world > 1 "
                "(or set_force_dp at world 1)");
    TORCH_CHECK((OFF_BD1 - OFF_WD1) % (W * 64) == 0, "set_zero: fc1 weight not divisible into ", W, " shards");
    zshard_ = (OFF_BD1 - OFF_WD1) / W;
    zero_ = true;
  }
  bool zero() const { return zero_; }
  // DP fc-region gradients by sufficient-factor broadcasting (mnist_fc_grad_sfb): all-gather the
  // fc factors (p2 after the conv forward, dh / hd / dlogits after the head) and compute the summed
  // fc gradients locally instead of all-reducing them. Needs the transport attached first.
  void set_fc_sfb(bool on) {
    if (!on) { sfb_ = false; return; }
    TORCH_CHECK(comm_ || ipc_, "set_fc_sfb: attach a communicator first");
    const int64_t W = world();
    sfb_rs_ = mnist_sfb_slot_elems((int)B_);
    auto bf = at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA, device_);
    if (!sfp2_.defined() || sfp2_.numel() != W * B_ * FEAT) {
      sfp2_ = at::zeros({W * B_ * FEAT}, bf);
      sfdr_ = at::zeros({W * sfb_rs_}, bf);
    }
    sfb_ = true;
  }
  bool fc_sfb() const { return sfb_active(); }
  // SFB schedule: run the conv slab reduce inside the SFB GEMM's launch (one kernel boundary and the
  // reduce's own latency less; the conv bucket's all-reduce moves behind the fc-region optimizer)
  void set_sfb_merge_reduce(bool on) { merge_tail_ = on; }
  bool sfb_merge_reduce() const { return merge_tail_; }
  // bf16 elements of the larger of the two per-rank gather shards (IPC staging must hold it)
  int64_t sfb_shard_elems() const { return std::max<int64_t>(B_ * FEAT, mnist_sfb_slot_elems((int)B_)); }
  void set_fused_tail(int64_t on) { fuse_tail_ = on != 0; }
  // one GPU, fused tail: keep the fc-region gradients in bf16 (as DP all-reduces them)
  void set_local_bf16_grads(int64_t on) { local_bf16_grads_ = on != 0; }
  // Make every rank's state whole again after ZeRO-1 steps (before eval / checkpoint / broadcast):
  // each rank updated the fp32 master, m and v of its own fc1 shard only, so all four are
  // all-gathered -- the bf16 shadow (what the forward reads) and the fp32 master + Adam slots (what
  // params() / a checkpoint read).
  void sync_params() {
    if (!zero_) return;
    hipStream_t s = stream();
    ag_w(s);
    const int64_t r = rank_in_comm();
    std::vector<at::Tensor*> whole = {&params_, &m_, &v_};
    if (opt_ == OptKind::RmsProp && centered_) whole.push_back(&s3_);
    for (at::Tensor* t : whole) {
      float* base = (float*)t->data_ptr() + OFF_WD1;
      if (comm_) comm_->all_gather_raw(base + r * zshard_, base, (size_t)zshard_, ncclFloat32, s);
      else ipc_->all_gather_raw(base, 4, zshard_, s);
    }
  }

  // ---- compute precision ----
  // "bf16" (default): bf16 MFMA operands / activations, fp32 accumulation, master and optimizer.
  // "fp32": the reference's precision -- every operand and activation fp32, GEMMs on the fp32
  // matrix core (csrc/kernels/mnist_f32.hip); the gradient wire format becomes fp32 too.
  void set_dtype(const std::string& dt) {
    TORCH_CHECK(dt == "bf16" || dt == "fp32", "dtype must be bf16 or fp32");
    const bool f = dt == "fp32";
    if (f && !f1_.defined()) {
      auto f32 = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device_);
      f1_ = at::empty({B_, P1H, P1H, C1}, f32);
      f2_ = at::empty({B_, FEAT}, f32);
      fhd_ = at::empty({B_, HID}, f32);
      fdh_ = at::empty({B_, HID}, f32);
      fdz2_ = at::empty({B_, P1H, P1H, C2}, f32);
      fslab_ = at::empty({mnist_f32_fc1_splits(), B_, HID}, f32);
      fwg2_ = at::empty({mnist_f32_wg2_splits((int)B_), 801, C2}, f32);
    }
    if (fp32_ && !f) sync_shadow();  // the fp32 optimizer tail leaves the bf16 shadow stale
    fp32_ = f;
    if (f) bf16_comm_ = false;
  }
  std::string dtype() const { return fp32_ ? "fp32" : "bf16"; }

  // ---- per-phase GPU timing ----
  // With timing on, train_step records HIP timing events at its phase boundaries -- also inside a
  // captured graph (event-record nodes) -- and phase_times() returns the last step's
  //   [forward, fc backward, conv backward, optimizer, allreduce (sum of the bucket collectives on
  //    the comm stream; 0 on one GPU), exposed comm wait, step] in milliseconds.
  void set_phase_timing(bool on) { timing_ = on; }
  at::Tensor phase_times() {
    auto out = at::zeros({7}, at::TensorOptions().dtype(at::kFloat));
    if (!timing_ || !timed_) return out;
    HIP_OK(hipEventSynchronize(pev_[P_OPT]));
    float* o = out.data_ptr<float>();
    auto el = [&](int a, int b) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pev_[a], pev_[b]) == hipSuccess) return ms;
      (void)hipGetLastError();  // not sticky: a pair that cannot be timed reports -1
      return -1.f;
    };
    o[0] = el(P_START, P_FWD);
    o[1] = el(P_FWD, P_BFC);
    o[2] = el(P_BFC, P_BCONV);
    o[3] = el(P_BCONV, P_OPT);
    if (timed_dp_) {
      o[4] = el(P_CA0, P_CA1) + el(P_CB0, P_CB1);
      o[5] = el(P_BCONV, P_CB1);
    }
    o[6] = el(P_START, P_OPT);
    return out;
  }

  // ---- device step log (csrc/step_log.h) ----
  // A ring of `capacity` per-step records -- {loss, correct, lr, grad_norm, clip_scale, ok, rows} and the
  // step number t -- written inside the step by one small launch behind the head kernel of every training
  // (micro-)batch and, with clipping or the guard, one behind the norm / guard finish: the record of
  // update t (global_step after it) lives in slot (t - 1) % capacity, so a replayed n-step graph leaves
  // every step's values behind. 0 turns it off (the default: nothing is allocated and the step is launch
  // for launch what it was). Observation only: no kernel of the step reads the log. evaluate() and
  // capture_grads do not log. Like phase timing it takes effect for graphs captured afterwards; a call
  // that changes the capacity allocates a fresh ring (no slot written) and drops the captured graphs.
  void set_step_log(int64_t capacity) {
    TORCH_CHECK(capacity >= 0 && capacity <= (1 << 20), "set_step_log: 0 (off) <= capacity <= 2^20, got ", capacity);
    if (capacity == slog_cap_) return;
    for (auto& kv : graphs_) hipGraphExecDestroy(kv.second);
    graphs_.clear();
    slog_cap_ = capacity;
    if (capacity == 0) {
      slog_t_ = slog_rec_ = slog_acc_ = at::Tensor();
      return;
    }
    // host tensors copied over: ready when the call returns, whichever stream the first step runs on.
    // t = 0 marks a slot no step has written (a record's t is >= 1)
    slog_t_ = at::zeros({capacity}, at::kLong).to(params_.device());
    slog_rec_ = at::zeros({capacity, kStepLogFields}, at::kFloat).to(params_.device());
    slog_acc_ = at::zeros({2}, at::kDouble).to(params_.device());
  }
  int64_t step_log_capacity() const { return slog_cap_; }
  // {t int64 [capacity], records fp32 [capacity][8]}, on the device (share storage with the engine)
  std::vector<at::Tensor> step_log() {
    TORCH_CHECK(slog_cap_ > 0, "step_log: set_step_log(capacity > 0) first");
    return {slog_t_, slog_rec_};
  }
  // Cost probe: `iters` launches of the loss-mode kernel alone over this engine's rows, timed with HIP
  // events; returns ms per launch. Rewrites the record of the next update with the same values.
  double step_log_probe(int64_t iters) {
    TORCH_CHECK(slog_cap_ > 0 && iters >= 1, "step_log_probe: set_step_log first, iters >= 1");
    hipStream_t s = stream();
    const int64_t* c = (const int64_t*)step_.data_ptr();
    log_loss(c, SL_WHOLE, s, 1);  // warm
    HipEvent e0(true), e1(true);
    HIP_OK(hipEventRecord(e0, s));
    for (int64_t i = 0; i < iters; ++i) log_loss(c, SL_WHOLE, s, 1);
    HIP_OK(hipEventRecord(e1, s));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms / (double)iters;
  }

  // ---- step pieces (current HIP stream) ----
  void forward(bool train) {
    if (fp32_) mnist_f32_forward(args_f32(), train, stream());
    else mnist_forward(args(), train, stream());
  }
  // fp32 mode: backward_a runs the whole backward (fc + conv), backward_b the slab reduce
  void backward_a() {
    if (fp32_) mnist_f32_backward(args_f32(), stream());
    else mnist_backward_a(args(), stream());
  }
  // backward_b ends with the conv-grad reduce kernel, which also bumps global_step (see
  // MnistStepArgs::step_bump): apply_optimizer() after it therefore uses t = global_step.
  void backward_b() {
    MnistStepArgs a = args();
    a.step_bump = (int64_t*)step_.data_ptr();
    if (fp32_) {
      a.wg2_slab = (float*)fwg2_.data_ptr();
      a.wg2_splits = mnist_f32_wg2_splits((int)B_);
      mnist_conv_grad_reduce(a, stream());
      return;
    }
    mnist_backward_b(a, stream());
    mnist_conv_grad_reduce(a, stream());
  }
  void apply_optimizer(double grad_scale) {
    apply_optimizer_range(0, TOTAL, grad_scale, 0, stream());
  }
  // Optimizer over the flat range [beg, end) on stream s; t = global_step + t_offset. The one place that
  // chooses between the layer-wise optimizers, the rules, Adam and SGD; optim_launch.h picks the variant from
  // mods(). gscale: the step's clip factor on the device, ok: the non-finite guard's device ok; null without.
  void apply_optimizer_range(int64_t beg, int64_t end, double grad_scale, int t_offset, hipStream_t s,
                             const int64_t* tsrc = nullptr, const float* gscale = nullptr, const float* ok = nullptr) {
    if (!tsrc) tsrc = (const int64_t*)step_.data_ptr();
    const bool bf_grads = bf16_comm_ && dp();
    const OptMods m = mods(beg, gscale, ok);
    if (layerwise()) {
      TORCH_CHECK(beg == 0 && end == TOTAL, "a layer-wise optimizer updates the whole flat buffer: a range has no "
                  "per-variable norm");
      apply_layerwise(bf_grads, grad_scale, t_offset, tsrc, m, s);
    } else if (is_rule()) {
      apply_rule(beg, end - beg, bf_grads, grad_scale, t_offset, tsrc, m, s);
    } else if (opt_ == OptKind::Adam) {
      adam_launch(adam_args(beg, end - beg, bf_grads, grad_scale, t_offset, tsrc), m, s);
    } else {
      sgd_launch(sgd_args(beg, end - beg, bf_grads, grad_scale, t_offset, tsrc), m, s);
    }
  }
  // Adam over up to 3 ranges of the flat buffers in one launch (o: buffer bases)
  void apply_adam_ranges(const AdamArgs& o, int nr, const int64_t* beg, const int64_t* n, hipStream_t s) {
    adam_launch_ranges(o, mods(0, nullptr, nullptr), nr, beg, n, s);
  }

  // Full synchronous data-parallel step (the reference's SyncReplicasOptimizer global step with
  // replicas_to_aggregate == num_workers: averaged grads, one ApplyAdam, global_step += 1).
  // One GPU: fused forward/backward and ONE optimizer kernel (it also reduces the conv slabs).
  // DP (train_step_dp): three streams, the fc-region optimizer deferred into the next step.
  void train_step() { train_step_impl(true); }

  void train_step_impl(bool join_end) {
    // checked before anything is launched: the sharded schedules read the bf16 shadow, which the
    // fp32 step leaves stale
    TORCH_CHECK(!(zero_ && fp32_), "ZeRO-1 is a bf16-path option: set_zero(False) or set_dtype('bf16')");
    // a sharded gradient has no global norm without a scalar collective inside the graph
    TORCH_CHECK(!(clip_norm_ > 0 && (zero_ || sfb_active())), "set_clip_norm conflicts with ",
                zero_ ? "ZeRO-1 (set_zero)" : "sufficient-factor fc gradients (set_fc_sfb)",
                ": the global norm needs the whole aggregated gradient on every rank; use the all-reduce schedule");
    // a sharded gradient has no per-variable norm either
    TORCH_CHECK(!(layerwise() && (zero_ || sfb_active())), lw_ == LwKind::Lamb ? "set_lamb" : "set_lars", " conflicts with ",
                zero_ ? "ZeRO-1 (set_zero)" : "sufficient-factor fc gradients (set_fc_sfb)",
                ": the per-variable norms need the whole aggregated gradient on every rank; use the all-reduce schedule");
    // nor a whole-gradient sum of squares to call finite
    TORCH_CHECK(!(guard_ && (zero_ || sfb_active())), "set_skip_nonfinite conflicts with ",
                zero_ ? "ZeRO-1 (set_zero)" : "sufficient-factor fc gradients (set_fc_sfb)",
                ": the guard reads the whole aggregated gradient on every rank; use the all-reduce schedule");
    // each rank updates only its fc1 shard, so it would own only that shard of the averages
    TORCH_CHECK(!(ema_on() && zero_), "set_ema conflicts with ZeRO-1 (set_zero): each rank would hold only its fc1 "
                "shard of the moving averages; use a schedule without ZeRO");
    // the sharded schedules fuse gradient production with the collectives: no summed gradient to hold back
    TORCH_CHECK(!(accum_ > 1 && (zero_ || sfb_active())), "set_grad_accum conflicts with ",
                zero_ ? "ZeRO-1 (set_zero)" : "sufficient-factor fc gradients (set_fc_sfb)",
                ": the micro-batch gradients are summed whole before the one collective; use the all-reduce schedule");
    if (zero_ && !sfb_active()) {
      train_step_zero();
      return;
    }
    hipStream_t s = stream();
    const bool dp = this->dp();
    timed_ = timing_;
    timed_dp_ = timing_ && dp;
    if (accum_ > 1) {
      train_step_accum(dp);
      return;
    }
    if (clip_norm_ > 0 || layerwise() || guard_) {
      train_step_clip(dp);
      return;
    }
    if (fp32_) {
      train_step_f32(dp);
      return;
    }
    if (dp) {
      if (sfb_active()) {
        train_step_sfb_serial(join_end);
      } else {
        train_step_dp(join_end);
      }
      return;
    }
    mark(P_START, s);
    MnistStepArgs a = args();
    // one GPU: nothing to overlap with. With Adam ONE kernel ends the step: it reduces the conv
    // weight-gradient slabs itself and bumps the step (its t was written by the head kernel).
    const bool fused = opt_ == OptKind::Adam && fuse_tail_;
    if (fused) a.t_out = (int64_t*)tnext_.data_ptr();
    // bf16 fc-region gradients (the DP wire format): the fc backward writes 2 B and Adam reads
    // 2 B per gradient instead of 4 + 4 (13 MB less HBM traffic per step)
    const bool gbf_local = fused && local_bf16_grads_;
    if (gbf_local) a.gbf_a = (uint16_t*)gbf_.data_ptr();
    const MnistAdamArgs o = fused_adam_args((uint16_t*)pbf_.data_ptr(), gbf_local);
    mnist_forward_conv(a, s);
    tag("conv_fwd", s);
    mnist_forward_fc(a, true, s);
    tag("fc_fwd", s);
    log_loss(a.step, SL_WHOLE, s);
    mark(P_FWD, s);
    mnist_backward_a(a, s);
    tag("fc_bwd", s);
    mark(P_BFC, s);
    a.step_bump = (int64_t*)step_.data_ptr();
    mnist_backward_b(a, s);
    tag("conv_bwd", s);
    if (fused) {
      mark(P_BCONV, s);
      if (ema_on()) mnist_adam_fused_ema(a, ema_args(o), s, true);
      else mnist_adam_fused(a, o, s, true);
      tag("opt", s);
    } else {
      mnist_conv_grad_reduce(a, s);
      tag("slab_reduce", s);
      mark(P_BCONV, s);
      apply_optimizer_range(0, TOTAL, 1.0, 0, s);
      tag("opt", s);
    }
    mark(P_OPT, s);
  }

  // DP step, three streams (main s, comm c, optimizer o):
  //   s: conv fwd -> [wait o: previous step's fc optimizer] -> fc fwd + head -> fc bwd (bucket A as
  //      bf16 in gbf) -> conv bwd -> conv-slab reduce (bucket B as bf16 in gbf, step bump)
  //      -> [wait c: B reduced] -> optimizer on B (conv region)
  //   c: [wait A] all-reduce A -> [wait B] all-reduce B
  //   o: [wait A reduced] optimizer on A (fc region; t from the head kernel, so the step bump on s
  //      does not race it)
  // The fc optimizer overlaps the conv backward, bucket B's collective, the conv optimizer AND the
  // next step's conv forward (which needs only conv params): the main stream waits for it just
  // before the next fc forward. Captured multi-step graphs keep that cross-step overlap; the last
  // step of a graph (and every eager step) joins o back into s at its end.
  void train_step_dp(bool join_end) {
    hipStream_t s = stream();
    const double scale = 1.0 / (double)world();
    const bool bf = bf16_comm_;
    MnistStepArgs a = args();
    set_dp_outputs(a, bf);
    mark(P_START, s);
    mnist_forward_conv(a, s);
    tag("conv_fwd", s);
    if (pending_opt_a_) {
      wait(s, ev_opt_a_, "fc_fwd<-opt_fc");
      pending_opt_a_ = false;
    }
    mnist_forward_fc(a, true, s);
    tag("fc_fwd", s);
    log_loss(a.step, SL_WHOLE, s);
    mark(P_FWD, s);
    mnist_backward_a(a, s, 0);
    tag("fc_bwd", s);
    mark(P_BFC, s);
    hand_off(s, ev_a_, comm_stream_, "ar_fc<-fc_bwd");
    mark(P_CA0, comm_stream_);
    reduce_bucket(BUCKET_SPLIT, TOTAL, bf);
    tag("ar_fc", comm_stream_);
    mark(P_CA1, comm_stream_);
    hand_off(comm_stream_, ev_ag_, opt_stream_, "opt_fc<-ar_fc");
    apply_optimizer_range(BUCKET_SPLIT, TOTAL, scale, 0, opt_stream_, (const int64_t*)tnext_.data_ptr());
    tag("opt_fc", opt_stream_);
    HIP_OK(hipEventRecord(ev_opt_a_, opt_stream_));
    mnist_backward_b(a, s);
    tag("conv_bwd", s);
    mnist_conv_grad_reduce(a, s);
    tag("slab_reduce", s);
    all_reduce_conv(s, bf);
    wait(s, ev_done_, "opt_conv<-ar_conv");
    apply_optimizer_range(0, BUCKET_SPLIT, scale, 0, s);
    tag("opt_conv", s);
    mark(P_OPT, s);
    if (join_end) wait(s, ev_opt_a_, "end<-opt_fc");
    else pending_opt_a_ = true;
  }

  // DP step with sufficient-factor fc gradients (set_fc_sfb): every compute kernel on the main
  // stream in one order, only the collectives on the comm stream. The round-2 overlapped schedule
  // (SFB GEMM + fc optimizer on a second stream beside the conv backward and the next conv forward;
  // removed in round 3, A/B in profiles/mnist_dp_schedule_ab_r2.log) measured 124 us/step in the world-1 rehearsal against 74 for the fused one-GPU step: these
  // kernels each fill the GPU, so running two of them at once slowed both (conv2 wgrad 10 -> 19 us),
  // as the one-GPU overlap A/Bs showed (profiles/ab_fc_adam_overlap_r2.log).
  //   s: conv fwd -> fc fwd -> head -> fc1 dX -> conv wgrad / dgrad -> conv slab reduce (+ next
  //      batch, step bump) -> [wait dh gather] SFB fc GEMM -> [wait conv bucket] ONE optimizer
  //   c: [p2] gather p2 (beside fc fwd + head) -> [head] gather dh|hd|dlogits (beside dX + conv
  //      backward) -> [slabs reduced] conv bucket all-reduce (beside the SFB GEMM)
  //   ZeRO-1: the GEMM forms only this rank's fc1 shard rows, the optimizer runs on conv + shard +
  //   tail, and the updated bf16 shards are all-gathered on c beside the next conv forward.
  void train_step_sfb_serial(bool join_end) {
    hipStream_t s = stream();
    const double scale = 1.0 / (double)world();
    const bool bf = bf16_comm_;
    const bool shard = zero_;
    const int64_t rk = rank_in_comm();
    MnistStepArgs a = args();
    if (shard) {
      const int64_t rows = zshard_ / HID;
      mnist_sfb_tile_rows((int)(rk * rows), (int)((rk + 1) * rows), &a.sfb_by_lo, &a.sfb_by_hi);
    }
    set_dp_outputs(a, bf);
    mark(P_START, s);
    // last step's fc1 bf16 shards -> every rank, beside the conv fwd
    if (shard && pending_wag_ && !wag_issued_) gather_weights(s, "wag<-opt");
    mnist_forward_conv(a, s);
    tag("conv_fwd", s);
    hand_off(s, ev_p2_, comm_stream_, "gather_p2<-conv_fwd");
    mark(P_CA0, comm_stream_);
    gather_sfb(true, comm_stream_);
    tag("gather_p2", comm_stream_);
    if (shard && pending_wag_) {
      wait(s, ev_wag_, "fc_fwd<-wag");
      pending_wag_ = wag_issued_ = false;
    }
    mnist_forward_fc(a, true, s);
    tag("fc_fwd", s);
    mark(P_FWD, s);
    hand_off(s, ev_a_, comm_stream_, "gather_dr<-fc_fwd");
    log_loss(a.step, SL_WHOLE, s);  // behind the hand-off: the factor gather does not wait for it
    gather_sfb(false, comm_stream_);
    tag("gather_dr", comm_stream_);
    mark(P_CA1, comm_stream_);
    HIP_OK(hipEventRecord(ev_ag_, comm_stream_));
    mnist_backward_a(a, s, 2);  // fc1 dX from this rank's own rows
    tag("fc1_dx", s);
    mark(P_BFC, s);
    mnist_backward_b(a, s);
    tag("conv_bwd", s);
    if (merge_tail_) {
      // ONE launch for the slab reduce and the SFB GEMM (their blocks side by side); the conv
      // bucket's all-reduce then runs beside the fc-region optimizer instead of beside the GEMM
      wait(s, ev_ag_, "sfb_gemm<-gather_dr");
      mnist_fc_grad_sfb(a, s, true);
      tag("sfb_gemm", s);
      tag_alias("slab_reduce");
      all_reduce_conv(s, bf);
    } else {
      mnist_conv_grad_reduce(a, s);
      tag("slab_reduce", s);
      all_reduce_conv(s, bf);
      wait(s, ev_ag_, "sfb_gemm<-gather_dr");
      mnist_fc_grad_sfb(a, s);  // beside the conv bucket's all-reduce
      tag("sfb_gemm", s);
    }
    const int64_t* t = (const int64_t*)tnext_.data_ptr();
    // With real peers the conv bucket's all-reduce can outlast the SFB GEMM (at 8 ranks the ZeRO
    // GEMM is ~4 us): the fc-region optimizer (its gradients are local) then runs first and covers
    // it, and only the small conv region waits for the collective. At world 1 (the rehearsal) the
    // collective is instant and one launch is cheaper.
    const bool split_opt = world() > 1;
    if (!split_opt) wait(s, ev_done_, "opt<-ar_conv");
    if (shard) {
      const int64_t beg[3] = {0, OFF_WD1 + rk * zshard_, OFF_BD1};
      const int64_t end[3] = {BUCKET_SPLIT, OFF_WD1 + (rk + 1) * zshard_, TOTAL};
      if (opt_ == OptKind::Adam && BUCKET_SPLIT % 4 == 0 && zshard_ % 4 == 0) {  // one launch over the ranges
        const int64_t n[3] = {end[0] - beg[0], end[1] - beg[1], end[2] - beg[2]};
        const AdamArgs o = adam_args(0, 0, bf16_comm_, scale, 0, t);  // buffer bases; n comes per range
        if (split_opt) {
          apply_adam_ranges(o, 2, beg + 1, n + 1, s);
          tag("opt_fc", s);
          // the updated shard can leave now: the gather queues behind the conv bucket's all-reduce on
          // the comm stream and runs beside the conv-region Adam and the next conv forward
          gather_weights(s, "wag<-opt_fc");
          wag_issued_ = true;
          wait(s, ev_done_, "opt_conv<-ar_conv");
          apply_adam_ranges(o, 1, beg, n, s);
          tag("opt_conv", s);
        } else {
          apply_adam_ranges(o, 3, beg, n, s);
          tag("opt", s);
        }
      } else {
        for (int k = 1; k < 3; ++k) apply_optimizer_range(beg[k], end[k], scale, 0, s, t);
        tag("opt_fc", s);
        if (split_opt) wait(s, ev_done_, "opt_conv<-ar_conv");
        apply_optimizer_range(beg[0], end[0], scale, 0, s, t);
        tag("opt_conv", s);
      }
      pending_wag_ = true;
      if (join_end) {  // the caller reads whole weights after this step: gather the shards now
        if (!wag_issued_) gather_weights(s, "wag<-opt");
        wait(s, ev_wag_, "end<-wag");
        pending_wag_ = wag_issued_ = false;
      }
    } else if (split_opt) {
      apply_optimizer_range(BUCKET_SPLIT, TOTAL, scale, 0, s, t);
      tag("opt_fc", s);
      wait(s, ev_done_, "opt_conv<-ar_conv");
      apply_optimizer_range(0, BUCKET_SPLIT, scale, 0, s, t);
      tag("opt_conv", s);
    } else {
      apply_optimizer_range(0, TOTAL, scale, 0, s, t);
      tag("opt", s);
    }
    mark(P_OPT, s);
  }

  // fp32 step: forward, backward (fc grads + conv slabs), slab reduce + step bump, [fp32
  // all-reduce of the whole buffer], optimizer (t = bumped step).
  void train_step_f32(bool dp) {
    hipStream_t s = stream();
    MnistF32Args f = args_f32();
    // one GPU + Adam: ONE tail kernel reduces the conv slabs, runs Adam over every region and bumps
    // the step (t from the head), as the bf16 step does
    const bool fused = !dp && opt_ == OptKind::Adam && fuse_tail_;
    if (fused) f.t_out = (int64_t*)tnext_.data_ptr();
    mark(P_START, s);
    mnist_f32_forward(f, true, s);
    log_loss(f.step, SL_WHOLE, s);
    mark(P_FWD, s);
    mnist_f32_backward(f, s);
    mark(P_BFC, s);
    MnistStepArgs r = args();
    r.wg2_slab = f.wg2_slab;
    r.wg2_splits = f.wg2_splits;
    r.xpre = nullptr;  // the fp32 kernels read their batch rows through perm/step: no prefetch gather
    if (fused) {
      // no bf16 shadow: nothing in fp32 mode reads it (set_dtype("bf16") re-derives it), and its
      // 6.5 MB of writes are 1 us of the bandwidth-bound optimizer tail
      mark(P_BCONV, s);
      if (ema_on()) mnist_adam_fused_ema(r, ema_args(fused_adam_args(nullptr, false)), s, true);
      else mnist_adam_fused(r, fused_adam_args(nullptr, false), s, true);
      mark(P_OPT, s);
      return;
    }
    r.step_bump = (int64_t*)step_.data_ptr();
    mnist_conv_grad_reduce(r, s);
    mark(P_BCONV, s);
    if (dp) all_reduce_whole(s, "f32:ar<-slab_reduce", "f32:opt<-ar", false);
    apply_optimizer_range(0, TOTAL, 1.0 / (double)world(), 0, s);
    mark(P_OPT, s);
  }

  // Step with global-norm clipping (set_clip_norm), the non-finite guard (set_skip_nonfinite) and / or a
  // layer-wise optimizer (set_lamb, set_lars):
  // one serial schedule for both dtypes, the shape of the unfused one-GPU step --
  //   s: forward -> backward a -> backward b -> conv-slab reduce (step bump) -> [DP: wait c]
  //      -> [clip: norm stage 1 -> norm stage 2] -> ONE optimizer over [0, TOTAL), t = global_step
  //         (layer-wise: its three stages, which need the whole aggregated gradient as the clip does)
  //   c (DP): [wait fc bwd] all-reduce A -> [wait slab reduce] all-reduce B  (fp32 dtype: one bucket)
  // The norm is taken of the aggregated gradient, in the buffer the optimizer reads (gbf_ with a bf16
  // wire), so N ranks at batch B stay equal to one at N*B. The fused one-GPU tail cannot host the clip:
  // its conv gradients are summed inside the optimizer kernel, so they do not exist when the norm is
  // needed; and the deferred fc-region optimizer of train_step_dp would need the norm before the conv
  // gradients exist.
  void train_step_clip(bool dp) {
    hipStream_t s = stream();
    const double scale = 1.0 / (double)world();
    const bool bf = bf16_comm_ && dp;
    int64_t* step = (int64_t*)step_.data_ptr();
    if (pending_opt_a_) {  // an unclipped DP graph left its fc-region optimizer running
      wait(s, ev_opt_a_, "fc_fwd<-opt_fc");
      pending_opt_a_ = false;
    }
    mark(P_START, s);
    MnistStepArgs a = args();
    if (fp32_) {
      MnistF32Args f = args_f32();
      mnist_f32_forward(f, true, s);
      tag("fwd", s);
      log_loss(f.step, SL_WHOLE, s);
      mark(P_FWD, s);
      mnist_f32_backward(f, s);
      tag("bwd", s);
      mark(P_BFC, s);
      a.wg2_slab = f.wg2_slab;
      a.wg2_splits = f.wg2_splits;
      a.xpre = nullptr;  // as train_step_f32: no prefetch gather
      a.step_bump = step;
      mnist_conv_grad_reduce(a, s);
      tag("slab_reduce", s);
      mark(P_BCONV, s);
      if (dp) all_reduce_whole(s, "ar<-slab_reduce", "grad_norm<-ar", true);
    } else {
      if (dp) set_dp_outputs(a, bf);
      else a.step_bump = step;
      mnist_forward_conv(a, s);
      tag("conv_fwd", s);
      mnist_forward_fc(a, true, s);
      tag("fc_fwd", s);
      log_loss(a.step, SL_WHOLE, s);
      mark(P_FWD, s);
      mnist_backward_a(a, s, 0);
      tag("fc_bwd", s);
      mark(P_BFC, s);
      if (dp) {
        hand_off(s, ev_a_, comm_stream_, "ar_fc<-fc_bwd");
        mark(P_CA0, comm_stream_);
        reduce_bucket(BUCKET_SPLIT, TOTAL, bf);
        tag("ar_fc", comm_stream_);
        mark(P_CA1, comm_stream_);
      }
      mnist_backward_b(a, s);
      tag("conv_bwd", s);
      mnist_conv_grad_reduce(a, s);
      tag("slab_reduce", s);
      if (dp) {
        all_reduce_conv(s, bf);  // behind bucket A's on the comm stream: ev_done_ covers both
        wait(s, ev_done_, "grad_norm<-ar_conv");
      } else {
        mark(P_BCONV, s);
      }
    }
    whole_gradient_tail(scale, s);
  }

  // The end of the steps that hold the whole aggregated gradient in one flat buffer (train_step_clip,
  // train_step_accum) -- grad_, or gbf_ with a bf16 wire (bf) -- after the step bump: [clip: norm stage
  // 1 -> norm stage 2] -> ONE optimizer over [0, TOTAL), t = global_step (layer-wise: its three stages).
  // With the guard, stage 2 is the guard finish ({norm, scale, ok}, the skipped-step counter; scale
  // exactly 1 without clipping) and the optimizer its guarded instantiation, which stores nothing when
  // ok == 0. In DP the buffer is the all-reduced one, so every rank decides alike: whether a sum is
  // finite does not depend on its order.
  void whole_gradient_tail(double scale, hipStream_t s) {
    const bool bf = bf16_comm_ && dp();  // what both callers hold, and what apply_optimizer_range derives
    float* pair = (float*)gnorm_.data_ptr();
    float* part = (float*)gpart_.data_ptr();
    if (guard_ || clip_norm_ > 0)
      grad_sumsq((const float*)grad_.data_ptr(), bf ? (const uint16_t*)gbf_.data_ptr() : nullptr, TOTAL, part, s);
    if (guard_) {
      grad_guard_finish(part, grad_norm_blocks(TOTAL), (float)scale,
                        clip_norm_ > 0 ? (float)clip_norm_ : std::numeric_limits<float>::infinity(), pair,
                        (int64_t*)skipped_.data_ptr(), s);
      tag("grad_guard", s);
    } else if (clip_norm_ > 0) {
      grad_norm_finish(part, grad_norm_blocks(TOTAL), (float)scale, (float)clip_norm_, pair, s);
      tag("grad_norm", s);
    }
    // after the step bump (both callers): the triple goes into the record of update global_step
    if (guard_ || clip_norm_ > 0) log_norm(s);
    // the step's clip factor and the guard's ok on the device; null without
    apply_optimizer_range(0, TOTAL, scale, 0, s, nullptr, guard_ || clip_norm_ > 0 ? pair + 1 : nullptr,
                          guard_ ? pair + 2 : nullptr);
    tag("opt", s);
    mark(P_OPT, s);
  }

  // One optimizer step over K = grad_accum() micro-batches (set_grad_accum), both dtypes, one GPU and
  // the all-reduce DP schedule:
  //   s: K x [forward -> fc backward -> conv backward -> conv-slab reduce (micro bump, next micro-batch's
  //      gather) -> grad_accum over [0, TOTAL): store / add / emit] -> [DP: wait c] -> the tail of
  //      train_step_clip (whole_gradient_tail) at scale 1 / (K * world)
  //   c (DP): [wait the emit] ONE all-reduce per bucket, of the summed gradient
  // The micro-batch kernels are those of the unfused path and write un-rounded fp32 into grad_ (per
  // micro-batch rounding to bf16 is what accumulation must avoid); they read the micro counter where a
  // plain step reads global_step (MnistStepArgs::step / step_bump), so the data cursor, the prefetch
  // tag and the dropout key advance per micro-batch. The emit writes the sum where the collective or
  // the optimizer reads it -- grad_, or bf16 into gbf_ with a bf16 wire -- and bumps global_step, which
  // schedules, EMA decay and Adam's t follow.
  void train_step_accum(bool dp) {
    hipStream_t s = stream();
    const int64_t K = accum_;
    const double scale = 1.0 / (double)(K * world());
    const bool bf = bf16_comm_ && dp;
    int64_t* micro = (int64_t*)micro_.data_ptr();
    if (pending_opt_a_) {  // an earlier DP graph left its fc-region optimizer running
      wait(s, ev_opt_a_, "fc_fwd<-opt_fc");
      pending_opt_a_ = false;
    }
    mark(P_START, s);
    for (int64_t j = 0; j < K; ++j) {
      const bool last = j == K - 1;
      const int log_mode = last ? SL_EMIT : (j == 0 ? SL_STORE : SL_ADD);
      MnistStepArgs a = args();
      a.step = micro;
      a.step_bump = micro;
      if (input_mode_ == 0) {  // fed: this micro-batch's rows of the K * B fed
        a.data += j * B_ * 784;
        a.labels += j * B_;
      }
      if (fp32_) {
        MnistF32Args f = args_f32(a);
        mnist_f32_forward(f, true, s);
        tag("fwd", s);
        log_loss(micro, log_mode, s);
        if (last) mark(P_FWD, s);
        mnist_f32_backward(f, s);
        tag("bwd", s);
        if (last) mark(P_BFC, s);
        a.wg2_slab = f.wg2_slab;
        a.wg2_splits = f.wg2_splits;
        a.xpre = nullptr;  // as train_step_f32: no prefetch gather
      } else {
        mnist_forward_conv(a, s);
        tag("conv_fwd", s);
        mnist_forward_fc(a, true, s);
        tag("fc_fwd", s);
        log_loss(micro, log_mode, s);
        if (last) mark(P_FWD, s);
        mnist_backward_a(a, s, 0);
        tag("fc_bwd", s);
        if (last) mark(P_BFC, s);
        mnist_backward_b(a, s);
        tag("conv_bwd", s);
      }
      mnist_conv_grad_reduce(a, s);
      tag("slab_reduce", s);
      GradAccumArgs g{};
      g.acc = (float*)acc_.data_ptr();
      g.g = (const float*)grad_.data_ptr();
      g.n = TOTAL;
      g.mode = last ? GA_EMIT : (j == 0 ? GA_STORE : GA_ADD);
      if (last) {
        if (bf) g.outbf = (uint16_t*)gbf_.data_ptr();
        else g.out = (float*)grad_.data_ptr();
        g.bump = (int64_t*)step_.data_ptr();
      }
      tfd::grad_accum(g, s);
      tag("accum", s);
    }
    if (!dp) {
      mark(P_BCONV, s);
    } else if (fp32_) {
      mark(P_BCONV, s);
      all_reduce_whole(s, "ar<-accum", "grad_norm<-ar", true);
    } else {
      hand_off(s, ev_a_, comm_stream_, "ar_fc<-accum");
      mark(P_CA0, comm_stream_);
      reduce_bucket(BUCKET_SPLIT, TOTAL, bf);
      tag("ar_fc", comm_stream_);
      mark(P_CA1, comm_stream_);
      all_reduce_conv(s, bf);  // behind bucket A's on the comm stream: ev_done_ covers both
      wait(s, ev_done_, "grad_norm<-ar_conv");
    }
    whole_gradient_tail(scale, s);
  }

  void train_step_zero() {
    timed_ = false;
    hipStream_t s = stream();
    const double scale = 1.0 / (double)world();
    const int64_t r = rank_in_comm();
    MnistStepArgs a = args();
    // all-gather last step's updated fc1 shadow shards, overlapping the conv forward
    hand_off(s, ev_start_, comm_stream_, "zero:wag<-prev_opt");
    ag_w(comm_stream_);
    HIP_OK(hipEventRecord(ev_ag_, comm_stream_));
    mnist_forward_conv(a, s);
    wait(s, ev_ag_, "zero:fc_fwd<-wag");
    mnist_forward_fc(a, true, s);
    log_loss(a.step, SL_WHOLE, s);
    // bf16 wire format for both buckets, produced by the kernels themselves -- the same rounding
    // points as train_step_dp (the conv bucket used to be summed from fp32 and rounded after the
    // sum here, so ZeRO and replicated DP differed by bf16 rounding of the conv gradients)
    const bool pre_b = fused_bf16_a();
    if (pre_b) {
      a.gbf_a = (uint16_t*)gbf_.data_ptr();
      a.gbf_b = (uint16_t*)gbf_.data_ptr();
    }
    mnist_backward_a(a, s);
    hand_off(s, ev_a_, comm_stream_, "zero:rs_fc<-fc_bwd");
    rs_w(comm_stream_);
    reduce_bucket(OFF_BD1, TOTAL, in_gbf(OFF_BD1));
    apply_optimizer_range(OFF_WD1 + r * zshard_, OFF_WD1 + (r + 1) * zshard_, scale, 1, comm_stream_);
    apply_optimizer_range(OFF_BD1, TOTAL, scale, 1, comm_stream_);
    HIP_OK(hipEventRecord(ev_opt_a_, comm_stream_));
    a.step_bump = (int64_t*)step_.data_ptr();
    mnist_backward_b(a, s);
    wait(s, ev_opt_a_, "zero:slab_reduce<-opt_fc");
    mnist_conv_grad_reduce(a, s);
    hand_off(s, ev_b_, comm_stream_, "zero:ar_conv<-slab_reduce");
    reduce_bucket(0, BUCKET_SPLIT, pre_b);
    hand_off(comm_stream_, ev_done_, s, "zero:opt_conv<-ar_conv");
    apply_optimizer_range(0, BUCKET_SPLIT, scale, 0, s);
  }

  // Backup-worker path (SyncReplicas with replicas_to_aggregate < workers): sum-all-reduce of
  // weight * local grads over the whole flat buffer (no optimizer). weight is 1 for the chosen
  // replicas and 0 for the dropped stragglers; apply_optimizer(1/R) follows.
  void reduce_grads(double weight) {
    hipStream_t s = stream();
    if (weight != 1.0) scale_f32((float*)grad_.data_ptr(), TOTAL, (float)weight, s);
    if (!dp()) return;
    hand_off(s, ev_a_, comm_stream_, "reduce_grads:ar<-grads");
    reduce_bucket(0, TOTAL, false);
    hand_off(comm_stream_, ev_done_, s, "reduce_grads:end<-ar");
  }

  // Evaluate on an explicit batch (x [n,784] fp32, y [n] int32) in chunks of <= B.
  // Returns a 2-element fp32 GPU tensor {sum of per-example loss, number correct}.
  // use_ema: the forward reads the moving averages (set_ema) in place of the parameters -- the fp32
  // shadow or, in bf16, a bf16 image of it, cast here when a step or load_ema has made it stale (the
  // step does not write it).
  at::Tensor evaluate(at::Tensor x, at::Tensor y, bool use_ema) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.size(1) == 784, "x: [n,784] fp32 GPU");
    TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kInt, "y: [n] int32 GPU");
    TORCH_CHECK(!use_ema || ema_on(), "evaluate(use_ema): set_ema first");
    if (use_ema && !fp32_) {
      if (!ema_bf_.defined()) ema_bf_ = at::empty_like(pbf_);
      if (ema_bf_stale_) cast_f32_bf16((const float*)ema_.data_ptr(), (uint16_t*)ema_bf_.data_ptr(), TOTAL, stream());
      ema_bf_stale_ = false;
    }
    x = x.contiguous();
    y = y.contiguous();
    const int64_t n = x.size(0);
    auto out = at::zeros({2}, x.options());
    for (int64_t o = 0; o < n; o += B_) {
      const int nb = (int)std::min<int64_t>(B_, n - o);
      if (fp32_) {
        MnistF32Args f = args_f32();
        f.B = nb;
        f.data = (const float*)x.data_ptr() + o * 784;
        f.labels = (const int*)y.data_ptr() + o;
        f.perm = nullptr;
        if (use_ema) f.p32 = (const float*)ema_.data_ptr();
        mnist_f32_forward(f, false, stream());
      } else {
        MnistStepArgs a = args();
        a.B = nb;
        a.data = (const float*)x.data_ptr() + o * 784;
        a.labels = (const int*)y.data_ptr() + o;
        a.perm = nullptr;
        if (use_ema) {
          a.p32 = (const float*)ema_.data_ptr();
          a.pbf = (const uint16_t*)ema_bf_.data_ptr();
        }
        mnist_forward(a, false, stream());
      }
      out[0] += loss_row_.narrow(0, 0, nb).sum();
      out[1] += correct_row_.narrow(0, 0, nb).sum();
    }
    return out;
  }

  // ---- device inference (csrc/mnist_infer.h) ----
  // The forward up to fc1 as evaluate() runs it, then the inference head, which stores the logits and
  // classes into buffers of its own: loss_rows(), correct_rows(), dlogits(), the prefetch buffers and
  // every piece of training state keep their bits.
  //
  // predict: x [n,784] fp32, y an empty tensor or [n] int32, both on the engine's device and
  // contiguous; rows in chunks of <= B. Returns (logits [n,10] fp32, classes [n] int32, loss_rows [n],
  // correct_rows [n]); the last two are empty without labels. use_ema as in evaluate().
  std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> predict(at::Tensor x, at::Tensor y, bool use_ema) {
    check_rows("predict: x", x, at::kFloat, 2);
    TORCH_CHECK(x.size(1) == 784, "predict: x must be [n,784], got [", x.size(0), ",", x.size(1), "]");
    const int64_t n = x.size(0);
    const bool labelled = y.numel() > 0;
    if (labelled) {
      check_rows("predict: y", y, at::kInt, 1);
      TORCH_CHECK(y.size(0) == n, "predict: y has ", y.size(0), " labels for ", n, " rows");
    }
    TORCH_CHECK(!use_ema || ema_on(), "predict(use_ema): set_ema first");
    auto logits = at::empty({n, NCLS}, x.options());
    auto classes = at::empty({n}, x.options().dtype(at::kInt));
    auto loss = at::empty({labelled ? n : 0}, x.options());
    auto correct = at::empty({labelled ? n : 0}, x.options());
    if (n == 0) return {logits, classes, loss, correct};
    refresh_ema_image(use_ema, stream());
    for (int64_t o = 0; o < n; o += B_) {
      const int nb = (int)std::min<int64_t>(B_, n - o);
      InferHeadArgs h = infer_forward((const float*)x.data_ptr() + o * 784, nb, use_ema, stream());
      h.labels = labelled ? (const int*)y.data_ptr() + o : nullptr;
      h.logits = (float*)logits.data_ptr() + o * NCLS;
      h.classes = (int*)classes.data_ptr() + o;
      h.loss_row = labelled ? (float*)loss.data_ptr() + o : nullptr;
      h.correct_row = labelled ? (float*)correct.data_ptr() + o : nullptr;
      infer_head(h, !fp32_, stream());
    }
    return {logits, classes, loss, correct};
  }

  // A device-resident evaluation split, uploaded once: images [N,784] fp32, labels [N] int32 in
  // [0, 10) (checked here: one synchronisation). Graphs captured over an earlier split are dropped.
  void set_eval_dataset(at::Tensor images, at::Tensor labels) {
    check_rows("set_eval_dataset: images", images, at::kFloat, 2);
    check_rows("set_eval_dataset: labels", labels, at::kInt, 1);
    TORCH_CHECK(images.size(1) == 784 && labels.size(0) == images.size(0), "set_eval_dataset: images [N,784], labels [N]");
    if (labels.numel() > 0) {
      const int64_t lo = labels.min().item<int64_t>(), hi = labels.max().item<int64_t>();
      TORCH_CHECK(lo >= 0 && hi < NCLS, "set_eval_dataset: labels must be in [0, ", NCLS, "), got [", lo, ", ", hi, "]");
    }
    for (auto& kv : eval_recs_) drop_graph(kv.first);
    eval_recs_.clear();
    eval_x_ = images;
    eval_y_ = labels;
    if (!inf_logits_.defined()) {
      inf_logits_ = at::empty({B_, NCLS}, loss_row_.options());
      inf_classes_ = at::empty({B_}, ybuf_.options());
      inf_loss_ = at::empty({B_}, loss_row_.options());
      inf_correct_ = at::empty({B_}, loss_row_.options());
    }
  }
  int64_t eval_dataset_rows() const { return eval_x_.defined() ? eval_x_.size(0) : 0; }

  // Rows [first, first + count) of the evaluation split in groups of `group` rows, each group in
  // chunks of <= B: one record per group (mnist_infer.h), fp64 [ceil(count / group)][104] on the device.
  at::Tensor evaluate_dataset(int64_t first, int64_t count, int64_t group, bool use_ema) {
    check_eval_range("evaluate_dataset", first, count, group, use_ema);
    auto rec = at::empty({(count + group - 1) / group, kEvalRecFields}, eval_x_.options().dtype(at::kDouble));
    if (count == 0) return rec;
    refresh_ema_image(use_ema, stream());
    eval_launches(first, count, group, use_ema, (double*)rec.data_ptr(), stream());
    return rec;
  }
  // The same launches as ONE hipGraph, replayed with replay(name, 1); the records are eval_records(name),
  // allocated here, outside the capture. With use_ema in bf16 the graph's first node casts the fp32
  // shadow to the bf16 image the forward reads, so a replay always sees the current averages. The
  // first chunk's forward runs once eagerly before the capture: the launchers raise their kernels'
  // dynamic-LDS limits at their first launch, which belongs outside a capture.
  void capture_eval(const std::string& name, int64_t first, int64_t count, int64_t group, bool use_ema) {
    check_eval_range("capture_eval", first, count, group, use_ema);
    TORCH_CHECK(count > 0, "capture_eval: count > 0");
    hipStream_t s = capture_stream();
    drop_graph(name);
    auto rec = at::empty({(count + group - 1) / group, kEvalRecFields}, eval_x_.options().dtype(at::kDouble));
    if (use_ema && !fp32_ && !ema_bf_.defined()) ema_bf_ = at::empty_like(pbf_);
    (void)infer_forward((const float*)eval_x_.data_ptr() + first * 784, (int)std::min(std::min(B_, group), count), false, s);
    StreamCapture cap(s);
    if (use_ema && !fp32_) cast_f32_bf16((const float*)ema_.data_ptr(), (uint16_t*)ema_bf_.data_ptr(), TOTAL, s);
    eval_launches(first, count, group, use_ema, (double*)rec.data_ptr(), s);
    store_graph(name, cap);
    eval_recs_[name] = rec;
  }
  at::Tensor eval_records(const std::string& name) {
    auto it = eval_recs_.find(name);
    TORCH_CHECK(it != eval_recs_.end(), "eval_records: no evaluation graph named ", name);
    return it->second;
  }

  // ---- hipGraph capture / replay of the whole step ----
  void capture_train_step(const std::string& name) { capture_train_steps(name, 1); }
  // n consecutive steps in ONE graph: the step counter, the dataset cursor and the dropout key all
  // live on the device, so step i+1 of the graph is exactly the next training step. One launch per
  // n steps removes the host launch and the graph-to-graph boundary from n - 1 of them.
  void capture_train_steps(const std::string& name, int64_t n) {
    TORCH_CHECK(n >= 1 && n <= 1000, "capture_train_steps: 1 <= n <= 1000");
    hipStream_t s = capture_stream();
    drop_graph(name);
    StreamCapture cap(s);
    for (int64_t i = 0; i < n; ++i) train_step_impl(i == n - 1);
    store_graph(name, cap);
  }
  // forward + backward (fc gradients, conv slab reduce, step bump) as one graph, no optimizer: the
  // compute part of a parameter-server worker step (the update runs on the PS task's GPU,
  // csrc/runtime/gpu_ps.cpp). Replayed with replay(name, 1) after the batch is fed.
  void capture_grads(const std::string& name) {
    TORCH_CHECK(accum_ == 1, "capture_grads is one batch's forward and backward: set_grad_accum(1) first (grad_accum() = ",
                accum_, ")");
    hipStream_t s = capture_stream();
    drop_graph(name);
    timed_ = false;
    StreamCapture cap(s);
    forward(true);
    backward_a();
    backward_b();
    store_graph(name, cap);
  }
  void replay(const std::string& name, int64_t times) {
    auto it = graphs_.find(name);
    TORCH_CHECK(it != graphs_.end(), "no graph named ", name);
    hipStream_t s = stream();
    ema_bf_stale_ = true;
    for (int64_t i = 0; i < times; ++i) HIP_OK(hipGraphLaunch(it->second, s));
  }
  void drop_graph(const std::string& name) {
    auto it = graphs_.find(name);
    if (it != graphs_.end()) {
      hipGraphExecDestroy(it->second);
      graphs_.erase(it);
    }
  }

  // Dependency structure of the captured step graph (tests/test_graph_topology_gpu.py): captures n
  // consecutive training steps exactly as capture_train_steps does -- every stream, collective and
  // cross-stream event edge -- but instead of instantiating the graph returns its topology as text:
  //   "node <i> <hipGraphNodeType>", "edge <from> <to>", "tag <label>@<step> <node> <node> ..."
  // where a tag lists the nodes one operation of the schedule added (tag() calls in the train-step
  // functions). The test checks that every collective depends on the kernel that produced its
  // operand and that its consumers depend on it (read-after-write and write-after-read across steps).
  std::vector<std::string> capture_topology(int64_t n) {
    TORCH_CHECK(n >= 1 && n <= 8, "capture_topology: 1 <= n <= 8");
    topo_seen_.clear();
    topo_tags_.clear();
    StreamCapture cap(capture_stream());
    try {
      topo_ = true;
      for (int64_t i = 0; i < n; ++i) {
        topo_step_ = i;
        train_step_impl(i == n - 1);
      }
      topo_ = false;
    } catch (...) {
      topo_ = false;
      throw;
    }
    hipGraph_t g = cap.end();
    std::vector<std::string> out;
    size_t nn = 0, ne = 0;
    HIP_OK(hipGraphGetNodes(g, nullptr, &nn));
    std::vector<hipGraphNode_t> nodes(nn);
    HIP_OK(hipGraphGetNodes(g, nodes.data(), &nn));
    std::map<hipGraphNode_t, size_t> idx;
    for (size_t i = 0; i < nn; ++i) {
      idx[nodes[i]] = i;
      hipGraphNodeType ty = hipGraphNodeTypeEmpty;
      HIP_OK(hipGraphNodeGetType(nodes[i], &ty));
      out.push_back("node " + std::to_string(i) + " " + std::to_string((int)ty));
    }
    HIP_OK(hipGraphGetEdges(g, nullptr, nullptr, &ne));
    std::vector<hipGraphNode_t> from(ne), to(ne);
    if (ne) HIP_OK(hipGraphGetEdges(g, from.data(), to.data(), &ne));
    for (size_t e = 0; e < ne; ++e)
      out.push_back("edge " + std::to_string(idx.at(from[e])) + " " + std::to_string(idx.at(to[e])));
    for (auto& kv : topo_tags_) {
      std::string line = "tag " + kv.first;
      for (auto nd : kv.second) {
        auto it = idx.find(nd);
        if (it != idx.end()) line += " " + std::to_string(it->second);
      }
      out.push_back(line);
    }
    topo_tags_.clear();
    topo_seen_.clear();
    return out;
  }
  // Fault injection for the topology test: skip the cross-stream wait named `name` in later
  // captures ("" restores every wait). A graph captured this way is wrong by construction.
  void set_debug_drop_wait(const std::string& name) { drop_wait_ = name; }

  // Cost probe of the sufficient-factor fc-gradient kernel at world W on THIS GPU (one GPU cannot
  // run a W-rank job): factor buffers of W ranks (this rank's slot = its real factors, the others
  // copies of it) and `iters` launches of mnist_fc_grad_sfb timed with HIP events; returns ms per
  // launch. Writes the fc gradient region of grads_bf16() -- a diagnostic, not a training step.
  double sfb_probe(int64_t W, int64_t iters) {
    TORCH_CHECK(W >= 1 && W <= 64 && iters >= 1, "sfb_probe: 1 <= W <= 64");
    hipStream_t s = stream();
    const int64_t rs = mnist_sfb_slot_elems((int)B_);
    auto bf = at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA, device_);
    at::Tensor p2 = p2_.reshape({1, -1}).repeat({W, 1}).contiguous();
    at::Tensor dr = at::zeros({W, rs}, bf);
    auto slot0 = dr.select(0, 0);
    slot0.narrow(0, 0, B_ * HID).copy_(dh_.reshape({-1}));
    slot0.narrow(0, B_ * HID, B_ * HID).copy_(hd_.reshape({-1}));
    slot0.narrow(0, 2 * B_ * HID, 2 * B_ * NCLS).copy_(dlogits_.reshape({-1}).view(at::kBFloat16));
    dr.copy_(slot0.unsqueeze(0).expand({W, rs}));
    MnistStepArgs a = args();
    a.gbf_a = (uint16_t*)gbf_.data_ptr();
    a.sfb_world = (int)W;
    a.sfb_p2 = (const uint16_t*)p2.data_ptr();
    a.sfb_dr = (const uint16_t*)dr.data_ptr();
    a.sfb_rs = rs;
    mnist_fc_grad_sfb(a, s);  // warm (kernel attributes)
    HipEvent e0(true), e1(true);
    HIP_OK(hipEventRecord(e0, s));
    for (int64_t i = 0; i < iters; ++i) mnist_fc_grad_sfb(a, s);
    HIP_OK(hipEventRecord(e1, s));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms / (double)iters;
  }

 private:
  hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }
  enum { P_START, P_FWD, P_BFC, P_BCONV, P_OPT, P_CA0, P_CA1, P_CB0, P_CB1, P_N };
  void mark(int k, hipStream_t st) {
    if (timing_) HIP_OK(hipEventRecord(pev_[k], st));
  }
  // The stream a capture runs on. StreamCapture (hip_util.h) issues the hipStreamBeginCapture.
  hipStream_t capture_stream() {
    hipStream_t s = stream();
    TORCH_CHECK(s != nullptr, "capture needs a non-default stream (use torch.cuda.stream(...))");
    return s;
  }
  // ends the capture and keeps its instantiated graph under `name` for replay()
  void store_graph(const std::string& name, StreamCapture& cap) {
    hipGraphExec_t ex = nullptr;
    HIP_OK(hipGraphInstantiate(&ex, cap.end(), nullptr, nullptr, 0));
    graphs_[name] = ex;
  }
  // A cross-stream dependency of the schedule: `st` waits for `ev`. `name` ("consumer<-producer")
  // identifies the edge for the topology test's fault injection (set_debug_drop_wait). Every wait of
  // the engine goes through here.
  void wait(hipStream_t st, hipEvent_t ev, const char* name) {
    if (!drop_wait_.empty() && drop_wait_ == name) return;
    HIP_OK(hipStreamWaitEvent(st, ev, 0));
  }
  // `to` goes on only after everything queued on `from` so far: record `ev` there, wait for it here
  void hand_off(hipStream_t from, hipEvent_t ev, hipStream_t to, const char* name) {
    HIP_OK(hipEventRecord(ev, from));
    wait(to, ev, name);
  }
  // ZeRO + SFB: the updated fc1 bf16 shards go to every rank on the comm stream, behind what `s` has
  // queued so far (`name` names that wait). The consumer waits for ev_wag_ later, where it needs them.
  void gather_weights(hipStream_t s, const char* name) {
    hand_off(s, ev_start_, comm_stream_, name);
    ag_w(comm_stream_);
    tag("wag", comm_stream_);
    HIP_OK(hipEventRecord(ev_wag_, comm_stream_));
  }
  // bf16 DP steps: the conv bucket's all-reduce on the comm stream, behind the slab reduce on `s`.
  // The consumer waits for ev_done_ later, where it needs the reduced bucket.
  void all_reduce_conv(hipStream_t s, bool pre) {
    mark(P_BCONV, s);
    hand_off(s, ev_b_, comm_stream_, "ar_conv<-slab_reduce");
    mark(P_CB0, comm_stream_);
    reduce_bucket(0, BUCKET_SPLIT, pre);
    tag("ar_conv", comm_stream_);
    mark(P_CB1, comm_stream_);
    HIP_OK(hipEventRecord(ev_done_, comm_stream_));
  }
  // fp32 DP steps: ONE all-reduce of the whole fp32 buffer on the comm stream, behind what `s` has queued
  // (edge `in`); `s` goes on behind it (edge `out`). One bucket, so bucket B's marks time nothing.
  void all_reduce_whole(hipStream_t s, const char* in, const char* out, bool tagged) {
    hand_off(s, ev_b_, comm_stream_, in);
    mark(P_CA0, comm_stream_);
    reduce_bucket(0, TOTAL, false);
    if (tagged) tag("ar", comm_stream_);
    mark(P_CA1, comm_stream_);
    mark(P_CB0, comm_stream_);
    mark(P_CB1, comm_stream_);
    hand_off(comm_stream_, ev_done_, s, out);
  }

  // ---- device step log: the two launches (no-ops with the log off) ----
  StepLogArgs log_args(int mode, const int64_t* counter) {
    StepLogArgs g{};
    g.t = (int64_t*)slog_t_.data_ptr();
    g.rec = (float*)slog_rec_.data_ptr();
    g.capacity = slog_cap_;
    g.counter = counter;
    g.mode = mode;
    return g;
  }
  // behind the head kernel on its stream; counter: what the head read (global_step, or the micro
  // counter under accumulation), not yet bumped. acc_mode: SL_WHOLE, or the micro-batch's store / add / emit
  void log_loss(const int64_t* counter, int acc_mode, hipStream_t s, int64_t K = 0) {
    if (!slog_cap_) return;
    StepLogArgs g = log_args(SL_LOSS, counter);
    g.acc_mode = acc_mode;
    g.accum = K ? K : (acc_mode == SL_WHOLE ? 1 : accum_);
    g.loss_row = (const float*)loss_row_.data_ptr();
    g.correct_row = (const float*)correct_row_.data_ptr();
    g.B = (int)B_;
    g.acc = (double*)slog_acc_.data_ptr();
    g.sched = sched_;
    tfd::step_log(g, s);
    tag("step_log", s);
  }
  // behind the norm / guard finish on its stream, after the step bump
  void log_norm(hipStream_t s) {
    if (!slog_cap_) return;
    StepLogArgs g = log_args(SL_NORM, (const int64_t*)step_.data_ptr());
    g.triple = (const float*)gnorm_.data_ptr();
    tfd::step_log(g, s);
    tag("step_log_norm", s);
  }

  // ---- argument structs of the optimizer kernels: each is filled in one place ----
  // Range [beg, beg + n) of the flat buffers; bf_grads: the gradients are bf16 in gbf_
  AdamArgs adam_args(int64_t beg, int64_t n, bool bf_grads, double grad_scale, int t_offset, const int64_t* t) {
    return AdamArgs{(float*)params_.data_ptr() + beg, (float*)m_.data_ptr() + beg, (float*)v_.data_ptr() + beg,
                    (const float*)grad_.data_ptr() + beg, (uint16_t*)pbf_.data_ptr() + beg,
                    bf_grads ? (const uint16_t*)gbf_.data_ptr() + beg : nullptr, n, sched_, (float)b1_,
                    (float)b2_, (float)eps_, t, t_offset, (float)grad_scale};
  }
  SgdArgs sgd_args(int64_t beg, int64_t n, bool bf_grads, double grad_scale, int t_offset, const int64_t* t) {
    return SgdArgs{(float*)params_.data_ptr() + beg, opt_ == OptKind::Momentum ? (float*)m_.data_ptr() + beg : nullptr,
                   (const float*)grad_.data_ptr() + beg, (uint16_t*)pbf_.data_ptr() + beg,
                   bf_grads ? (const uint16_t*)gbf_.data_ptr() + beg : nullptr, n, sched_, (float)momentum_, 0.f,
                   (float)grad_scale, nesterov_ ? 1 : 0, t, t_offset};
  }
  // one-GPU fused tail (slab reduce + Adam over every region + step bump). pbf: the bf16 shadow to
  // write, null for none; bf_grads: the fc-region gradients are bf16 in gbf_
  MnistAdamArgs fused_adam_args(uint16_t* pbf, bool bf_grads) {
    return MnistAdamArgs{(float*)params_.data_ptr(), (float*)m_.data_ptr(), (float*)v_.data_ptr(), pbf, sched_,
                         (float)b1_, (float)b2_, (float)eps_, (const int64_t*)tnext_.data_ptr(),
                         (int64_t*)step_.data_ptr(), bf_grads ? (const uint16_t*)gbf_.data_ptr() : nullptr};
  }
  // what every optimizer setter ends with: the rule, no layer-wise form, a constant rate
  void set_optimizer(OptKind kind, double lr) { opt_ = kind; lw_ = LwKind::None; sched_ = lr_constant((float)lr); }
  bool layerwise() const { return lw_ != LwKind::None; }
  // ---- layer-wise optimizers ----
  // the variable table of the flat layout and its block table, built once, on the device
  void set_layerwise(LwKind kind, bool skip_bias) {
    const int w = LW_DECAY | LW_ADAPT, b = skip_bias ? 0 : w;
    const LwSegment segs[8] = {{OFF_WC1, KTAPS * C1, w}, {OFF_BC1, C1, b}, {OFF_WC2, KTAPS * C1 * C2, w}, {OFF_BC2, C2, b},
                               {OFF_WD1, (int64_t)FEAT * HID, w}, {OFF_BD1, HID, b}, {OFF_OUT, HID * NCLS, w},
                               {OFF_BOUT, NCLS, b}};
    LwTable t;
    try {
      t = lw_build_table(segs, 8, kLwChunk, TOTAL);
    } catch (const std::invalid_argument& e) {
      TORCH_CHECK(false, e.what());
    }
    auto to_dev = [&](const void* src, size_t bytes) {
      return at::from_blob(const_cast<void*>(src), {(int64_t)bytes}, at::TensorOptions().dtype(at::kByte))
          .to(params_.device());
    };
    // written in place once they exist (the sizes depend on the layout alone): a graph captured
    // earlier keeps pointing at live tables
    if (lw_out_.defined()) {
      lw_blocks_.copy_(to_dev(t.blocks.data(), t.blocks.size() * sizeof(LwBlock)));
      lw_segs_.copy_(to_dev(t.segs.data(), t.segs.size() * sizeof(LwSegBlocks)));
    } else {
      lw_blocks_ = to_dev(t.blocks.data(), t.blocks.size() * sizeof(LwBlock));
      lw_segs_ = to_dev(t.segs.data(), t.segs.size() * sizeof(LwSegBlocks));
      lw_nblocks_ = (int)t.blocks.size();
      // host tensors copied over: ready when the call returns, whichever stream the first step runs on
      lw_part_ = at::empty({lw_nblocks_, 2}, params_.options());  // every entry is stored by every stage 1
      lw_out_ = at::zeros({8, 3}, at::kFloat).to(params_.device());
    }
    lw_ = kind;
  }
  // stages 1, 2, 3 over [0, TOTAL); m: the step's modifiers (mods(0, ...))
  void apply_layerwise(bool bf_grads, double grad_scale, int t_offset, const int64_t* t, const OptMods& m, hipStream_t s) {
    const bool lamb = lw_ == LwKind::Lamb;
    LayerwiseArgs a{};
    a.p = (float*)params_.data_ptr();
    a.s1 = (float*)m_.data_ptr();
    a.s2 = lamb ? (float*)v_.data_ptr() : nullptr;
    a.g = bf_grads ? nullptr : (const float*)grad_.data_ptr();
    a.gbf = bf_grads ? (const uint16_t*)gbf_.data_ptr() : nullptr;
    a.pbf = (uint16_t*)pbf_.data_ptr();
    a.blocks = (const LwBlock*)lw_blocks_.data_ptr();
    a.segs = (const LwSegBlocks*)lw_segs_.data_ptr();
    a.nblocks = lw_nblocks_;
    a.nsegs = 8;
    a.partials = (float*)lw_part_.data_ptr();
    a.out = (float*)lw_out_.data_ptr();
    a.sched = sched_;
    a.beta1 = (float)b1_;
    a.beta2 = (float)b2_;
    a.momentum = (float)momentum_;
    a.eeta = (float)lw_eeta_;
    a.eps = (float)(lamb ? eps_ : lw_eps_);
    a.weight_decay = (float)lw_wd_;
    a.step = t;
    a.t_offset = t_offset;
    a.grad_scale = (float)grad_scale;
    apply_mods(a, m);
    if (lamb) lamb_apply(a, s);
    else lars_apply(a, s);
  }
  // RMSProp / Adagrad over [beg, beg + n); m: the range's modifiers (mods(beg, ...))
  bool is_rule() const { return opt_ == OptKind::RmsProp || opt_ == OptKind::Adagrad; }
  void apply_rule(int64_t beg, int64_t n, bool bf_grads, double grad_scale, int t_offset, const int64_t* t,
                  const OptMods& m, hipStream_t s) {
    const bool rms = opt_ == OptKind::RmsProp;
    RuleArgs a{};
    a.p = (float*)params_.data_ptr() + beg;
    a.s1 = (float*)v_.data_ptr() + beg;
    a.s2 = rms ? (float*)m_.data_ptr() + beg : nullptr;
    a.s3 = rms && centered_ ? (float*)s3_.data_ptr() + beg : nullptr;
    a.g = bf_grads ? nullptr : (const float*)grad_.data_ptr() + beg;
    a.gbf = bf_grads ? (const uint16_t*)gbf_.data_ptr() + beg : nullptr;
    a.pbf = (uint16_t*)pbf_.data_ptr() + beg;
    a.n = n;
    a.sched = sched_;
    a.decay = (float)rule_decay_;
    a.momentum = (float)momentum_;
    a.eps = (float)rule_eps_;
    a.step = t;
    a.t_offset = t_offset;
    a.grad_scale = (float)grad_scale;
    apply_mods(a, m);
    if (rms) rmsprop_apply(a, centered_, s);
    else adagrad_apply(a, s);
  }
  // What a step adds to the bare update over a range that starts at beg (optim_launch.h). The only reader of
  // the EMA settings and one_ for a flat launch; with the shadow it marks the shadow's bf16 image stale: an
  // EMA launch is about to move the shadow.
  bool ema_on() const { return ema_decay_ > 0; }
  OptMods mods(int64_t beg, const float* gscale, const float* ok) {
    OptMods m{gscale, ok};
    m.one = (const float*)one_.data_ptr();
    if (ema_on()) {
      ema_bf_stale_ = true;
      m.ema = (float*)ema_.data_ptr() + beg;
      m.ema_decay = (float)ema_decay_;
      m.ema_num_updates = ema_nu_ ? 1 : 0;
    }
    return m;
  }
  // the fused one-GPU tail's EMA wrapper
  MnistAdamEmaArgs ema_args(const MnistAdamArgs& o) {
    ema_bf_stale_ = true;
    return MnistAdamEmaArgs{o, (float*)ema_.data_ptr(), (float)ema_decay_, ema_nu_ ? 1 : 0};
  }
  // bf16 DP steps: the head kernel writes the optimizer's t, the slab reduce bumps the step, and with
  // a bf16 wire format (bf) both buckets' gradients come out of the kernels as bf16 in gbf_
  void set_dp_outputs(MnistStepArgs& a, bool bf) {
    a.t_out = (int64_t*)tnext_.data_ptr();
    a.step_bump = (int64_t*)step_.data_ptr();
    if (bf) a.gbf_a = a.gbf_b = (uint16_t*)gbf_.data_ptr();
  }

  // capture_topology: the last operation's nodes under a second label (one launch doing two jobs)
  void tag_alias(const char* label) {
    if (!topo_ || topo_tags_.empty()) return;
    auto nodes = topo_tags_.back().second;
    topo_tags_.emplace_back(std::string(label) + "@" + std::to_string(topo_step_), std::move(nodes));
  }
  // capture_topology: the graph nodes this operation added (everything new since the last tag; the
  // host issues operations one after another, so the difference is exactly this operation's nodes)
  void tag(const char* label, hipStream_t st) {
    if (!topo_) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t g = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    HIP_OK(hipStreamGetCaptureInfo_v2(st, &cs, &id, &g, &deps, &nd));
    TORCH_CHECK(cs == hipStreamCaptureStatusActive && g, "tag: stream not capturing");
    size_t n = 0;
    HIP_OK(hipGraphGetNodes(g, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    HIP_OK(hipGraphGetNodes(g, nodes.data(), &n));
    std::vector<hipGraphNode_t> fresh;
    for (auto nd_ : nodes)
      if (topo_seen_.insert(nd_).second) fresh.push_back(nd_);
    if (fresh.empty()) {
      // An operation that captured no node -- a world-1 in-place RCCL collective is a no-op -- gets
      // a marker: an empty kernel at the operation's place in its stream, with the dependencies the
      // collective would have had and the same successors. The checker then orders the schedule's
      // cross-stream waits around every RCCL collective too, not only around the IPC ones.
      noop_launch(1, st);
      HIP_OK(hipGraphGetNodes(g, nullptr, &n));
      nodes.resize(n);
      HIP_OK(hipGraphGetNodes(g, nodes.data(), &n));
      for (auto nd_ : nodes)
        if (topo_seen_.insert(nd_).second) fresh.push_back(nd_);
    }
    topo_tags_.emplace_back(std::string(label) + "@" + std::to_string(topo_step_), std::move(fresh));
  }

  // ZeRO helpers (fc1 weight region W = [OFF_WD1, OFF_BD1))
  void rs_w(hipStream_t st) {
    reduce_scatter_grads(OFF_WD1, zshard_, in_gbf(OFF_WD1), st);
  }
  // The updated bf16 fc1 shards -> every rank. At 8 ranks the 0.8 MB shard exactly fills the IPC
  // staging sized for the SFB p2 gather.
  void ag_w(hipStream_t st) {
    all_gather_bf16((uint16_t*)pbf_.data_ptr() + OFF_WD1, zshard_, st, "ZeRO weight gather");
  }

  bool sfb_active() const { return sfb_ && !fp32_ && dp() && sfp2_.defined(); }
  // in-place all-gather of one SFB factor array ([W][S], this rank's shard at r*S)
  void gather_sfb(bool p2part, hipStream_t st) {
    all_gather_bf16((uint16_t*)(p2part ? sfp2_ : sfdr_).data_ptr(), p2part ? B_ * FEAT : sfb_rs_, st, "SFB gather");
  }

  // bucket A's gradients come out of the fc backward as bf16 in gbf_ (MnistStepArgs::gbf_a)
  bool fused_bf16_a() const { return bf16_comm_ && dp(); }
  bool in_gbf(int64_t beg) const { return fused_bf16_a() && beg >= BUCKET_SPLIT; }

  // pre: the bucket's gradients are already bf16 in gbf_ (written by the producing kernel)
  void reduce_bucket(int64_t beg, int64_t end, bool pre) { all_reduce_grads(beg, end - beg, pre, comm_stream_); }

  // ---- collectives: the one place each chooses between the IPC and the RCCL transport ----
  // In-place all-gather of a bf16 array [W][S] with this rank's shard at r*S: the IPC one-shot gather
  // (one kernel reading every peer at once over all xGMI links) when its staging holds a shard, else
  // RCCL's. sync_params' fp32 gathers prefer RCCL and keep their own code.
  void all_gather_bf16(uint16_t* base, int64_t S, hipStream_t st, const char* what) {
    if (ipc_gathers(S)) ipc_->all_gather_raw(base, 2, S, st);
    else if (comm_) comm_->all_gather_raw(base + rank_in_comm() * S, base, (size_t)S, ncclBfloat16, st);
    else TORCH_CHECK(false, what, ": no communicator holds a ", S, "-element shard");
  }
  // Operands of a gradient collective on the flat range starting at beg. IPC reads the gradients
  // where the kernels wrote them (pre: as bf16 in gbf_, else fp32 in grad_), sums in fp32 in rank
  // order and writes where the optimizer reads: the wire format, bf16 in gbf_ or fp32 in grad_.
  // RCCL reduces in place in the wire format, so fp32 gradients are cast to it first.
  const void* grad_src(int64_t beg, bool pre) const {
    if (pre) return (const uint16_t*)gbf_.data_ptr() + beg;
    return (const float*)grad_.data_ptr() + beg;
  }
  void* grad_wire(int64_t beg) const {
    if (bf16_comm_) return (uint16_t*)gbf_.data_ptr() + beg;
    return (float*)grad_.data_ptr() + beg;
  }
  void* rccl_wire(int64_t beg, int64_t n, bool pre, hipStream_t st) {
    if (bf16_comm_ && !pre) cast_f32_bf16((const float*)grad_.data_ptr() + beg, (uint16_t*)grad_wire(beg), n, st);
    return grad_wire(beg);
  }
  ncclDataType_t wire_type() const { return bf16_comm_ ? ncclBfloat16 : ncclFloat32; }
  // Sum all-reduce of n gradients at beg: IPC without RCCL or for a latency-bound bucket
  // (<= ipc_small_ elements), else RCCL
  void all_reduce_grads(int64_t beg, int64_t n, bool pre, hipStream_t st) {
    if (ipc_ && (!comm_ || n <= ipc_small_)) {
      ipc_->all_reduce_raw(grad_src(beg, pre), pre, grad_wire(beg), bf16_comm_, n, 1.0, st);
      return;
    }
    TORCH_CHECK(comm_, "no communicator for a ", n, "-element bucket");
    comm_->all_reduce_raw(rccl_wire(beg, n, pre, st), (size_t)n, wire_type(), ncclSum, st);
  }
  // Sum reduce-scatter of world() * S gradients at beg into this rank's shard of them: RCCL when
  // present, else IPC
  void reduce_scatter_grads(int64_t beg, int64_t S, bool pre, hipStream_t st) {
    void* shard = grad_wire(beg + rank_in_comm() * S);
    if (comm_) {
      comm_->reduce_scatter_raw(rccl_wire(beg, world() * S, pre, st), shard, (size_t)S, wire_type(), ncclSum, st);
    } else {
      ipc_->reduce_scatter_raw(grad_src(beg, pre), pre, shard, bf16_comm_, S, 1.0, st);
    }
  }

  // ---- device inference ----
  // an operand of predict / set_eval_dataset, checked before the first launch: on the engine's device,
  // of the dtype and rank asked, contiguous
  void check_rows(const char* what, const at::Tensor& t, at::ScalarType dt, int64_t dim) const {
    TORCH_CHECK(t.is_cuda() && t.get_device() == device_, what, " must be on cuda:", device_);
    TORCH_CHECK(t.scalar_type() == dt, what, " must be ", dt, ", got ", t.scalar_type());
    TORCH_CHECK(t.dim() == dim, what, " must have ", dim, " dimension(s), got ", t.dim());
    TORCH_CHECK(t.is_contiguous(), what, " must be contiguous");
  }
  void check_eval_range(const char* what, int64_t first, int64_t count, int64_t group, bool use_ema) const {
    TORCH_CHECK(eval_x_.defined(), what, ": set_eval_dataset first");
    TORCH_CHECK(first >= 0 && count >= 0 && first + count <= eval_x_.size(0), what, ": rows [", first, ", ", first + count,
                ") outside the evaluation split of ", eval_x_.size(0), " rows");
    TORCH_CHECK(group >= 1, what, ": group >= 1, got ", group);
    TORCH_CHECK(!use_ema || ema_on(), what, "(use_ema): set_ema first");
  }
  // evaluate(use_ema)'s staleness rule for the bf16 image of the shadow
  void refresh_ema_image(bool use_ema, hipStream_t s) {
    if (!use_ema || fp32_) return;
    if (!ema_bf_.defined()) ema_bf_ = at::empty_like(pbf_);
    if (ema_bf_stale_) cast_f32_bf16((const float*)ema_.data_ptr(), (uint16_t*)ema_bf_.data_ptr(), TOTAL, s);
    ema_bf_stale_ = false;
  }
  // conv1, conv2 and fc1 over nb <= B fed rows at x, as evaluate() runs them; returns the inference
  // head's view of the slabs and the parameters (the caller sets the labels and the outputs)
  InferHeadArgs infer_forward(const float* x, int nb, bool use_ema, hipStream_t s) {
    InferHeadArgs h{};
    h.rows = nb;
    h.split_rows = nb;
    h.p32 = (const float*)(use_ema ? ema_ : params_).data_ptr();
    MnistStepArgs a = args();
    a.B = nb;
    a.data = x;
    a.labels = nullptr;
    a.perm = nullptr;
    if (use_ema) {
      a.p32 = h.p32;
      if (!fp32_) a.pbf = (const uint16_t*)ema_bf_.data_ptr();
    }
    if (fp32_) {
      MnistF32Args f = args_f32(a);
      mnist_f32_forward_nohead(f, s);
      h.fc1_slab = f.fc1_slab;
      h.splits = f.fc1_splits;
    } else {
      mnist_forward_nohead(a, s);
      h.fc1_slab = a.fc1_slab;
      h.splits = a.fc1_splits;
    }
    return h;
  }
  void eval_launches(int64_t first, int64_t count, int64_t group, bool use_ema, double* rec, hipStream_t s) {
    const float* x = (const float*)eval_x_.data_ptr();
    const int* y = (const int*)eval_y_.data_ptr();
    for (int64_t g0 = 0, gi = 0; g0 < count; g0 += group, ++gi) {
      const int64_t gn = std::min(group, count - g0);
      for (int64_t o = 0; o < gn; o += B_) {
        const int nb = (int)std::min<int64_t>(B_, gn - o);
        const int64_t r = first + g0 + o;
        InferHeadArgs h = infer_forward(x + r * 784, nb, use_ema, s);
        h.labels = y + r;
        h.logits = (float*)inf_logits_.data_ptr();
        h.classes = (int*)inf_classes_.data_ptr();
        h.loss_row = (float*)inf_loss_.data_ptr();
        h.correct_row = (float*)inf_correct_.data_ptr();
        infer_head(h, !fp32_, s);
        EvalReduceArgs e{nb, h.labels, h.classes, h.loss_row, h.correct_row, rec + gi * kEvalRecFields,
                         o == 0 ? EVAL_STORE : EVAL_ADD};
        eval_reduce(e, s);
      }
    }
  }

  MnistF32Args args_f32() { return args_f32(args()); }
  // the fp32 kernels' view of a step's arguments
  MnistF32Args args_f32(const MnistStepArgs& a) {
    TORCH_CHECK(f1_.defined(), "set_dtype('fp32') first");
    MnistF32Args f{};
    f.B = a.B;
    f.data = a.data;
    f.labels = a.labels;
    f.perm = a.perm;
    f.n_data = a.n_data;
    f.step = a.step;
    f.p32 = a.p32;
    f.grad = a.grad;
    f.p1 = (float*)f1_.data_ptr();
    f.idx1 = a.idx1;
    f.p2 = (float*)f2_.data_ptr();
    f.idx2 = a.idx2;
    f.fc1_slab = (float*)fslab_.data_ptr();
    f.hd = (float*)fhd_.data_ptr();
    f.dh = (float*)fdh_.data_ptr();
    f.dlogits = a.dlogits;
    f.loss_row = a.loss_row;
    f.correct_row = a.correct_row;
    f.dz2 = (float*)fdz2_.data_ptr();
    f.wg2_slab = (float*)fwg2_.data_ptr();
    f.wg1_slab = a.wg1_slab;
    f.fc1_splits = mnist_f32_fc1_splits();
    f.wg2_splits = mnist_f32_wg2_splits((int)B_);
    f.keep_prob = a.keep_prob;
    f.seed = a.seed;
    f.rank = a.rank;
    return f;
  }

  MnistStepArgs args() {
    MnistStepArgs a{};
    a.B = (int)B_;
    if (input_mode_ == 1) {
      a.data = (const float*)data_.data_ptr();
      a.labels = (const int*)labels_.data_ptr();
      a.perm = (const int*)perm_.data_ptr();
      a.n_data = (int)data_.size(0);
    } else {
      a.data = (const float*)xbuf_.data_ptr();
      a.labels = (const int*)ybuf_.data_ptr();
      a.perm = nullptr;
      a.n_data = (int)B_;
    }
    a.step = (const int64_t*)step_.data_ptr();
    a.p32 = (const float*)params_.data_ptr();
    a.pbf = (const uint16_t*)pbf_.data_ptr();
    a.grad = (float*)grad_.data_ptr();
    a.p1 = (uint16_t*)p1_.data_ptr();
    a.idx1 = (uint8_t*)idx1_.data_ptr();
    a.p2 = (uint16_t*)p2_.data_ptr();
    a.idx2 = (uint8_t*)idx2_.data_ptr();
    a.fc1_slab = (float*)fc1_slab_.data_ptr();
    a.hd = (uint16_t*)hd_.data_ptr();
    a.dh = (uint16_t*)dh_.data_ptr();
    a.dlogits = (float*)dlogits_.data_ptr();
    a.loss_row = (float*)loss_row_.data_ptr();
    a.correct_row = (float*)correct_row_.data_ptr();
    a.dz2 = (uint16_t*)dz2_.data_ptr();
    a.wg2_slab = (float*)wg2_slab_.data_ptr();
    a.wg1_slab = (float*)wg1_slab_.data_ptr();
    a.fc1_splits = fc1_splits_;
    a.wg2_splits = wg2_splits_;
    a.keep_prob = (float)keep_prob_;
    a.seed = seed_;
    a.rank = rank_;
    a.rows = input_mode_ == 1 ? (int*)rows_.data_ptr() : nullptr;
    a.xpre = input_mode_ == 1 ? (float*)xpre_.data_ptr() : nullptr;
    a.ypre = input_mode_ == 1 ? (int*)ypre_.data_ptr() : nullptr;
    a.dbg = dbg_.defined() ? (int64_t*)dbg_.data_ptr() : nullptr;
    if (sfb_active()) {
      const int64_t r = rank_in_comm();
      uint16_t* slot = (uint16_t*)sfdr_.data_ptr() + r * sfb_rs_;
      a.p2 = (uint16_t*)sfp2_.data_ptr() + r * B_ * FEAT;
      a.dh = slot;
      a.hd = slot + B_ * HID;
      a.dlogits = reinterpret_cast<float*>(slot + 2 * B_ * HID);
      a.sfb_world = (int)world();
      a.sfb_p2 = (const uint16_t*)sfp2_.data_ptr();
      a.sfb_dr = (const uint16_t*)sfdr_.data_ptr();
      a.sfb_rs = sfb_rs_;
    }
    a.sfb_by_lo = 0;
    a.sfb_by_hi = -1;  // all tile rows (train_step_sfb narrows it under ZeRO)
    return a;
  }

  int64_t B_, device_;
  double keep_prob_;
  uint32_t seed_, rank_;
  int fc1_splits_, wg2_splits_;
  int64_t input_mode_ = 0;
  OptKind opt_ = OptKind::Adam;
  // RMSProp / Adagrad (set_rmsprop / set_adagrad): the rule's scalars and the centered rule's third slot
  double rule_decay_ = 0.9, rule_eps_ = 1e-10;
  bool centered_ = false;
  at::Tensor s3_;
  LwKind lw_ = LwKind::None;  // layer-wise optimizer (set_lamb / set_lars); its tables and outputs
  int lw_nblocks_ = 0;
  double lw_wd_ = 0.0, lw_eeta_ = 0.0, lw_eps_ = 0.0;
  at::Tensor lw_blocks_, lw_segs_, lw_part_, lw_out_;
  double b1_ = 0.9, b2_ = 0.999, eps_ = 1e-8, momentum_ = 0.0;
  LrSchedule sched_ = lr_constant(0.01f);
  bool nesterov_ = false;
  bool bf16_comm_ = true;
  c10::intrusive_ptr<RcclComm> comm_;
  c10::intrusive_ptr<IpcComm> ipc_;
  int64_t ipc_small_ = 0;
  bool ipc_gather_ = true;
  at::Tensor params_, pbf_, grad_, m_, v_, gbf_, step_, tnext_;
  at::Tensor p1_, idx1_, p2_, idx2_, fc1_slab_, hd_, dh_, dlogits_, loss_row_, correct_row_, dz2_, wg2_slab_,
      wg1_slab_, xbuf_, ybuf_;
  at::Tensor data_, labels_, perm_, rows_, xpre_, ypre_, dbg_;
  at::Tensor f1_, f2_, fhd_, fdh_, fdz2_, fslab_, fwg2_;  // fp32-mode activations / slabs
  bool fp32_ = false;
  HipStream comm_stream_;
  HipEvent ev_a_, ev_b_, ev_done_;
  HipStream opt_stream_;  // train_step_dp: the fc-region optimizer
  HipEvent ev_opt_a_, ev_start_, ev_ag_;
  bool zero_ = false;
  bool merge_tail_ = false;
  bool pending_wag_ = false;  // serialized ZeRO: this step's shards not yet all-gathered
  bool wag_issued_ = false;   // ... their all-gather already queued on the comm stream (ev_wag_)
  bool force_dp_ = false;
  int64_t zshard_ = 0;
  bool pending_opt_a_ = false;  // DP: the main stream still has to wait for the fc optimizer
  // sufficient-factor fc gradients (set_fc_sfb): gathered factors, slot stride, events
  bool sfb_ = false;
  at::Tensor sfp2_, sfdr_;
  int64_t sfb_rs_ = 0;
  HipEvent ev_p2_, ev_wag_;
  // one GPU + Adam: the optimizer kernel also reduces the conv gradient slabs and bumps the step
  bool fuse_tail_ = true;
  bool local_bf16_grads_ = false;
  // global-norm clipping (set_clip_norm): 0 = off; {norm, scale} and stage 1's per-block partials
  double clip_norm_ = 0.0;
  at::Tensor gnorm_, gpart_;
  // non-finite guard (set_skip_nonfinite): ok is gnorm_[2]; the device counter of skipped steps
  bool guard_ = false;
  at::Tensor skipped_;
  // gradient accumulation (set_grad_accum): micro-batches per optimizer step (1 = off), the fp32
  // accumulator and the device micro-batch counter
  int64_t accum_ = 1;
  at::Tensor acc_, micro_;
  // device step log (set_step_log): capacity (0 = off), the ring {t, records} and, under accumulation,
  // the two fp64 sums carried from micro-batch to micro-batch
  int64_t slog_cap_ = 0;
  at::Tensor slog_t_, slog_rec_, slog_acc_;
  // moving average of the weights (set_ema): 0 = off; the fp32 shadow, its bf16 image for
  // evaluate(use_ema) (cast when stale); one_: the device 1.0f of OptMods::one
  double ema_decay_ = 0.0;
  bool ema_nu_ = false;
  at::Tensor ema_, ema_bf_, one_;
  bool ema_bf_stale_ = true;
  // device inference: the evaluation split (set_eval_dataset), the inference head's own per-chunk
  // outputs, and the record array of every captured evaluation graph
  at::Tensor eval_x_, eval_y_, inf_logits_, inf_classes_, inf_loss_, inf_correct_;
  std::map<std::string, at::Tensor> eval_recs_;
  std::map<std::string, hipGraphExec_t> graphs_;
  // capture_topology: nodes added by each tagged operation (label@step -> node handles)
  bool topo_ = false;
  int64_t topo_step_ = 0;
  std::set<hipGraphNode_t> topo_seen_;
  std::vector<std::pair<std::string, std::vector<hipGraphNode_t>>> topo_tags_;
  std::string drop_wait_;  // fault injection for the topology test: this named wait is skipped
  HipEvent pev_[P_N];
  bool timing_ = false, timed_ = false, timed_dp_ = false;
};

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  // the largest batch an MnistEngine accepts (csrc/tfd_kernels.h)
  m.def("mnist_max_batch() -> int", []() -> int64_t { return mnist_max_batch(); });
  m.class_<RcclComm>("RcclComm")
      .def(torch::init<at::Tensor, int64_t, int64_t, int64_t>())
      .def_static("unique_id", &RcclComm::unique_id)
      .def_static("reap", &RcclComm::reap)
      .def_static("retired_count", &RcclComm::retired_count)
      .def("graph_refs", &RcclComm::graph_refs)
      .def("world", &RcclComm::world)
      .def("rank", &RcclComm::rank)
      .def("all_reduce", &RcclComm::all_reduce)
      .def("reduce_scatter", &RcclComm::reduce_scatter)
      .def("all_gather", &RcclComm::all_gather)
      .def("broadcast", &RcclComm::broadcast)
      .def("send", &RcclComm::send)
      .def("recv", &RcclComm::recv)
      .def("abort", &RcclComm::abort);
  m.class_<MnistEngine>("MnistEngine")
      .def(torch::init<int64_t, int64_t, double, int64_t, int64_t>())
      .def("params", &MnistEngine::params)
      .def("params_bf16", &MnistEngine::params_bf16)
      .def("grads", &MnistEngine::grads)
      .def("grads_bf16", &MnistEngine::grads_bf16)
      .def("adam_m", &MnistEngine::adam_m)
      .def("adam_v", &MnistEngine::adam_v)
      .def("slot3", &MnistEngine::slot3)
      .def("step_tensor", &MnistEngine::step_tensor)
      .def("loss_rows", &MnistEngine::loss_rows)
      .def("correct_rows", &MnistEngine::correct_rows)
      .def("hidden", &MnistEngine::hidden)
      .def("pool1", &MnistEngine::pool1)
      .def("pool2", &MnistEngine::pool2)
      .def("pool1_argmax", &MnistEngine::pool1_argmax)
      .def("pool2_argmax", &MnistEngine::pool2_argmax)
      .def("dlogits", &MnistEngine::dlogits)
      .def("dhidden", &MnistEngine::dhidden)
      .def_static("max_batch", &MnistEngine::max_batch)
      .def("feed_x", &MnistEngine::feed_x)
      .def("feed_y", &MnistEngine::feed_y)
      .def("batch", &MnistEngine::batch)
      .def("set_grad_accum", &MnistEngine::set_grad_accum)
      .def("grad_accum", &MnistEngine::grad_accum)
      .def("micro_step_tensor", &MnistEngine::micro_step_tensor)
      .def("sync_micro_step", &MnistEngine::sync_micro_step)
      .def("set_step_log", &MnistEngine::set_step_log)
      .def("step_log_capacity", &MnistEngine::step_log_capacity)
      .def("step_log", &MnistEngine::step_log)
      .def("step_log_probe", &MnistEngine::step_log_probe)
      .def("set_dataset", &MnistEngine::set_dataset)
      .def("invalidate_prefetch", &MnistEngine::invalidate_prefetch)
      .def("set_debug_buffer", &MnistEngine::set_debug_buffer)
      .def("set_input_mode", &MnistEngine::set_input_mode)
      .def("set_keep_prob", &MnistEngine::set_keep_prob)
      .def("sync_shadow", &MnistEngine::sync_shadow)
      .def("set_adam", &MnistEngine::set_adam)
      .def("set_momentum", &MnistEngine::set_momentum)
      .def("set_rmsprop", &MnistEngine::set_rmsprop)
      .def("set_adagrad", &MnistEngine::set_adagrad)
      .def("set_lamb", &MnistEngine::set_lamb)
      .def("set_lars", &MnistEngine::set_lars)
      .def("layer_norms", &MnistEngine::layer_norms)
      .def("set_lr_schedule", &MnistEngine::set_lr_schedule)
      .def("lr_at_step", &MnistEngine::lr_at_step)
      .def("set_clip_norm", &MnistEngine::set_clip_norm)
      .def("clip_norm", &MnistEngine::clip_norm)
      .def("grad_norm", &MnistEngine::grad_norm)
      .def("set_skip_nonfinite", &MnistEngine::set_skip_nonfinite)
      .def("skip_nonfinite", &MnistEngine::skip_nonfinite)
      .def("skipped_steps", &MnistEngine::skipped_steps)
      .def("skipped_steps_tensor", &MnistEngine::skipped_steps_tensor)
      .def("last_step_ok", &MnistEngine::last_step_ok)
      .def("set_ema", &MnistEngine::set_ema)
      .def("ema_decay", &MnistEngine::ema_decay)
      .def("ema_decay_at_step", &MnistEngine::ema_decay_at_step)
      .def("ema_params", &MnistEngine::ema_params)
      .def("load_ema", &MnistEngine::load_ema)
      .def("set_comm", &MnistEngine::set_comm)
      .def("set_ipc", &MnistEngine::set_ipc)
      .def("set_ipc_gather", &MnistEngine::set_ipc_gather)
      .def("set_zero", &MnistEngine::set_zero)
      .def("set_sfb_merge_reduce", &MnistEngine::set_sfb_merge_reduce)
      .def("sfb_merge_reduce", &MnistEngine::sfb_merge_reduce)
      .def("set_fc_sfb", &MnistEngine::set_fc_sfb)
      .def("fc_sfb", &MnistEngine::fc_sfb)
      .def("sfb_shard_elems", &MnistEngine::sfb_shard_elems)
      .def("sfb_probe", &MnistEngine::sfb_probe)
      .def("set_force_dp", &MnistEngine::set_force_dp)
      .def("dp", &MnistEngine::dp)
      .def("set_fused_tail", &MnistEngine::set_fused_tail)
      .def("set_local_bf16_grads", &MnistEngine::set_local_bf16_grads)
      .def("capture_topology", &MnistEngine::capture_topology)
      .def("set_debug_drop_wait", &MnistEngine::set_debug_drop_wait)
      .def("set_dtype", &MnistEngine::set_dtype)
      .def("dtype", &MnistEngine::dtype)
      .def("set_phase_timing", &MnistEngine::set_phase_timing)
      .def("phase_times", &MnistEngine::phase_times)
      .def("zero", &MnistEngine::zero)
      .def("sync_params", &MnistEngine::sync_params)
      .def("world", &MnistEngine::world)
      .def("forward", &MnistEngine::forward)
      .def("backward_a", &MnistEngine::backward_a)
      .def("backward_b", &MnistEngine::backward_b)
      .def("apply_optimizer", &MnistEngine::apply_optimizer)
      .def("reduce_grads", &MnistEngine::reduce_grads)
      .def("train_step", &MnistEngine::train_step)
      .def("evaluate", &MnistEngine::evaluate, "", {torch::arg("x"), torch::arg("y"), torch::arg("use_ema") = false})
      .def("predict", &MnistEngine::predict, "", {torch::arg("x"), torch::arg("y"), torch::arg("use_ema") = false})
      .def("set_eval_dataset", &MnistEngine::set_eval_dataset)
      .def("eval_dataset_rows", &MnistEngine::eval_dataset_rows)
      .def("evaluate_dataset", &MnistEngine::evaluate_dataset, "",
           {torch::arg("first"), torch::arg("count"), torch::arg("group"), torch::arg("use_ema") = false})
      .def("capture_eval", &MnistEngine::capture_eval, "",
           {torch::arg("name"), torch::arg("first"), torch::arg("count"), torch::arg("group"), torch::arg("use_ema") = false})
      .def("eval_records", &MnistEngine::eval_records)
      .def("capture_train_step", &MnistEngine::capture_train_step)
      .def("capture_train_steps", &MnistEngine::capture_train_steps)
      .def("capture_grads", &MnistEngine::capture_grads)
      .def("replay", &MnistEngine::replay)
      .def("drop_graph", &MnistEngine::drop_graph);
}

}  // namespace tfd
