// Torch custom-op registration for the native library (namespace `tfd`, see torch.ops.tfd.*).
// Ops run on the caller's current HIP stream so they compose with torch stream/graph semantics.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "../grad_accum.h"
#include "flat_op_args.h"  // with optim_launch.h

namespace tfd {
uint32_t crc32c_extend(uint32_t init, const void* data, size_t n);

namespace {
using namespace flat_op;  // cur, flat_schedule, step_ptr, on_device_of, ema_shadow, flat_mods

int64_t crc32c_op(const at::Tensor& bytes, int64_t init) {
  TORCH_CHECK(!bytes.is_cuda() && bytes.is_contiguous(), "crc32c: contiguous CPU tensor");
  return (int64_t)crc32c_extend((uint32_t)init, bytes.data_ptr(), (size_t)bytes.nbytes());
}

// The buffers of the flat Adam / Momentum ops, checked as rule_args checks them (rules_ops.cpp): every buffer is
// contiguous, of p's size and on p's device, the slots fp32, g fp32 or bf16, pbf bf16. An out-of-bounds store of
// an optimizer is the worst kind there is, so nothing reaches a launcher unchecked.
void check_params(const at::Tensor& p, const char* who) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous() && p.numel() >= 1, who,
              ": p is a contiguous fp32 GPU tensor of at least one element");
}
float* slot_ptr(const at::Tensor& s, const at::Tensor& p, const char* who, const char* name) {
  TORCH_CHECK(on_device_of(s, p) && s.scalar_type() == at::kFloat && s.is_contiguous() && s.numel() == p.numel(), who, ": ",
              name, " is a contiguous fp32 tensor of p's size on p's device");
  return (float*)s.data_ptr();
}
// g as {fp32 pointer, bf16 pointer}: exactly one is set
struct GradPtr { const float* f; const uint16_t* b; };
GradPtr grad_ptr(const at::Tensor& g, const at::Tensor& p, const char* who) {
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(on_device_of(g, p) && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous() && g.numel() == p.numel(), who,
              ": g is a contiguous fp32 or bf16 tensor of p's size on p's device");
  return GradPtr{gb ? nullptr : (const float*)g.data_ptr(), gb ? (const uint16_t*)g.data_ptr() : nullptr};
}
uint16_t* shadow_ptr(const c10::optional<at::Tensor>& pbf, const at::Tensor& p, const char* who) {
  TORCH_CHECK(!pbf || (on_device_of(*pbf, p) && pbf->scalar_type() == at::kBFloat16 && pbf->is_contiguous() &&
                       pbf->numel() == p.numel()),
              who, ": pbf is a contiguous bf16 tensor of p's size on p's device");
  return pbf ? (uint16_t*)pbf->data_ptr() : nullptr;
}
// Adam's kernels read float4 of the fp32 buffers and uint2 of the bf16 ones
void check_aligned(const void* ptr, size_t bytes, const char* who, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ptr) % bytes == 0, who, ": ", name, " is not ", bytes,
              "-byte aligned (the kernel reads it as ", bytes == 16 ? "float4" : "uint2", ")");
}
// the launchers' own checks (ranges, the guard of the ranges form) as torch errors
template <class F>
void launch(F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    TORCH_CHECK(false, e.what());
  }
}

// what adam_flat and adam_ranges_flat share: every check both make, the kernel's arguments and the modifiers
struct AdamCall { AdamArgs a; OptMods m; };
AdamCall adam_flat_args(const char* who, at::Tensor& p, const at::Tensor& m, const at::Tensor& v, const at::Tensor& g,
                        const c10::optional<at::Tensor>& pbf, double lr, double b1, double b2, double eps,
                        const c10::optional<at::Tensor>& step, double grad_scale, int64_t t_offset, const std::string& lr_kind,
                        const std::vector<double>& lr_params, const std::vector<int64_t>& lr_boundaries,
                        const std::vector<double>& lr_values, const c10::optional<at::Tensor>& gscale,
                        const c10::optional<at::Tensor>& ema, double ema_decay, bool ema_num_updates,
                        const c10::optional<at::Tensor>& guard) {
  check_params(p, who);
  float* mp = slot_ptr(m, p, who, "m");
  float* vp = slot_ptr(v, p, who, "v");
  const GradPtr gp = grad_ptr(g, p, who);
  uint16_t* pb = shadow_ptr(pbf, p, who);
  const int64_t* step_p = step_ptr(step, p, who);
  const LrSchedule sc = flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values);
  TORCH_CHECK(sc.kind == LR_CONSTANT || step, who, ": a schedule needs the device step tensor");
  TORCH_CHECK(!ema_num_updates || !ema || step, who, ": ema_num_updates needs the device step tensor");
  const OptMods mods = flat_mods(who, p, gscale, ema, ema_decay, ema_num_updates, guard);
  check_aligned(p.data_ptr(), 16, who, "p");
  check_aligned(mp, 16, who, "m");
  check_aligned(vp, 16, who, "v");
  if (gp.f) check_aligned(gp.f, 16, who, "g");
  if (gp.b) check_aligned(gp.b, 8, who, "g");
  if (pb) check_aligned(pb, 8, who, "pbf");
  if (mods.ema) check_aligned(mods.ema, 16, who, "ema");
  return AdamCall{AdamArgs{(float*)p.data_ptr(), mp, vp, gp.f, pb, gp.b, p.numel(), sc, (float)b1, (float)b2, (float)eps,
                           step_p, (int)t_offset, (float)grad_scale},
                  mods};
}

// Adam's t = *step + t_offset (no step: t_offset); the schedule is evaluated on the device at s = t - 1
void adam_flat(at::Tensor p, at::Tensor m, at::Tensor v, at::Tensor g, c10::optional<at::Tensor> pbf, double lr,
               double b1, double b2, double eps, c10::optional<at::Tensor> step, double grad_scale, int64_t t_offset,
               std::string lr_kind, std::vector<double> lr_params, std::vector<int64_t> lr_boundaries,
               std::vector<double> lr_values, c10::optional<at::Tensor> gscale, c10::optional<at::Tensor> ema,
               double ema_decay, bool ema_num_updates, c10::optional<at::Tensor> guard) {
  const AdamCall c = adam_flat_args("adam_flat", p, m, v, g, pbf, lr, b1, b2, eps, step, grad_scale, t_offset, lr_kind,
                                    lr_params, lr_boundaries, lr_values, gscale, ema, ema_decay, ema_num_updates, guard);
  launch([&] { adam_launch(c.a, c.m, cur()); });
}

// The ranges form (adam_ranges_kernel: the ZeRO-1 optimizer's one launch over conv bucket + fc1 shard + tail) on
// its own, for the tests: adam_flat's arguments, and up to 3 ranges [beg[k], beg[k] + n[k]) of the buffers, in
// order and disjoint. Elements outside the ranges are not touched. The launcher refuses an unaligned range
// (every beg and every n but the last a multiple of 4), a range count outside 1..3 and a guard.
void adam_ranges_flat(at::Tensor p, at::Tensor m, at::Tensor v, at::Tensor g, c10::optional<at::Tensor> pbf,
                      std::vector<int64_t> beg, std::vector<int64_t> n, double lr, double b1, double b2, double eps,
                      c10::optional<at::Tensor> step, double grad_scale, int64_t t_offset, std::string lr_kind,
                      std::vector<double> lr_params, std::vector<int64_t> lr_boundaries, std::vector<double> lr_values,
                      c10::optional<at::Tensor> gscale, c10::optional<at::Tensor> ema, double ema_decay,
                      bool ema_num_updates, c10::optional<at::Tensor> guard) {
  const char* who = "adam_ranges_flat";
  const AdamCall c = adam_flat_args(who, p, m, v, g, pbf, lr, b1, b2, eps, step, grad_scale, t_offset, lr_kind, lr_params,
                                    lr_boundaries, lr_values, gscale, ema, ema_decay, ema_num_updates, guard);
  TORCH_CHECK(beg.size() == n.size(), who, ": one n per beg, got ", beg.size(), " and ", n.size());
  int64_t end = 0;
  for (size_t k = 0; k < beg.size(); ++k) {
    TORCH_CHECK(beg[k] >= end && n[k] >= 0 && n[k] <= p.numel() - beg[k], who, ": range ", k, " = [", beg[k], ", ", beg[k],
                " + ", n[k], ") is not inside the buffers behind its predecessor");
    end = beg[k] + n[k];
  }
  launch([&] { adam_launch_ranges(c.a, c.m, (int)beg.size(), beg.data(), n.data(), cur()); });
}

// what momentum_flat and momentum_ema_flat share: the checks both make and the kernel's arguments
SgdArgs sgd_flat_args(const char* who, at::Tensor& p, const c10::optional<at::Tensor>& mom, const at::Tensor& g,
                      const c10::optional<at::Tensor>& pbf, double lr, double momentum, double weight_decay, bool nesterov,
                      double grad_scale, const c10::optional<at::Tensor>& step, int64_t t_offset, const std::string& lr_kind,
                      const std::vector<double>& lr_params, const std::vector<int64_t>& lr_boundaries,
                      const std::vector<double>& lr_values) {
  check_params(p, who);
  float* mp = mom ? slot_ptr(*mom, p, who, "mom") : nullptr;
  const GradPtr gp = grad_ptr(g, p, who);
  uint16_t* pb = shadow_ptr(pbf, p, who);
  const int64_t* step_p = step_ptr(step, p, who);
  const LrSchedule sc = flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values);
  TORCH_CHECK(sc.kind == LR_CONSTANT || step, who, ": a schedule needs the device step tensor");
  return SgdArgs{(float*)p.data_ptr(), mp, gp.f, pb, gp.b, p.numel(), sc, (float)momentum, (float)weight_decay,
                 (float)grad_scale, nesterov ? 1 : 0, step_p, (int)t_offset};
}

void momentum_flat(at::Tensor p, c10::optional<at::Tensor> mom, at::Tensor g, c10::optional<at::Tensor> pbf,
                   double lr, double momentum, double weight_decay, bool nesterov, double grad_scale,
                   c10::optional<at::Tensor> step, int64_t t_offset, std::string lr_kind, std::vector<double> lr_params,
                   std::vector<int64_t> lr_boundaries, std::vector<double> lr_values,
                   c10::optional<at::Tensor> gscale, c10::optional<at::Tensor> guard) {
  const char* who = "momentum_flat";
  const SgdArgs a = sgd_flat_args(who, p, mom, g, pbf, lr, momentum, weight_decay, nesterov, grad_scale, step, t_offset,
                                  lr_kind, lr_params, lr_boundaries, lr_values);
  const OptMods mods = flat_mods(who, p, gscale, c10::nullopt, 0.0, false, guard);
  launch([&] { sgd_launch(a, mods, cur()); });
}

// momentum_flat with the moving average of the weights updated by the same launch (csrc/ema.h): the
// same arguments, then the shadow, its decay and whether the decay follows the step. An op of its own;
// momentum_flat itself is what it was.
void momentum_ema_flat(at::Tensor p, c10::optional<at::Tensor> mom, at::Tensor g, c10::optional<at::Tensor> pbf,
                       double lr, double momentum, double weight_decay, bool nesterov, double grad_scale,
                       c10::optional<at::Tensor> step, int64_t t_offset, std::string lr_kind,
                       std::vector<double> lr_params, std::vector<int64_t> lr_boundaries, std::vector<double> lr_values,
                       c10::optional<at::Tensor> gscale, at::Tensor ema, double ema_decay, bool ema_num_updates,
                       c10::optional<at::Tensor> guard) {
  const char* who = "momentum_ema_flat";
  const SgdArgs a = sgd_flat_args(who, p, mom, g, pbf, lr, momentum, weight_decay, nesterov, grad_scale, step, t_offset,
                                  lr_kind, lr_params, lr_boundaries, lr_values);
  TORCH_CHECK(!ema_num_updates || step, who, ": ema_num_updates needs the device step tensor");
  const OptMods mods = flat_mods(who, p, gscale, ema, ema_decay, ema_num_updates, guard);
  launch([&] { sgd_launch(a, mods, cur()); });
}

// The shadow update as a pass of its own, from parameters already updated: e' = e - (1 - d_t)(e - p),
// t = *step + t_offset (no step: t_offset). The same device helper as the fused variants.
void ema_flat(at::Tensor e, at::Tensor p, double decay, bool num_updates, c10::optional<at::Tensor> step,
              int64_t t_offset) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous(), "ema_flat: fp32 GPU params");
  TORCH_CHECK(!step || (step->scalar_type() == at::kLong && step->is_cuda()), "ema_flat: int64 GPU step");
  ema_apply(ema_shadow(e, p, decay, "ema_flat"), (const float*)p.data_ptr(), p.numel(), (float)decay, num_updates ? 1 : 0,
            step ? (const int64_t*)step->data_ptr() : nullptr, (int)t_offset, cur());
}

// {norm, scale} of tf.clip_by_global_norm over a flat fp32 or bf16 buffer, on the device:
// norm = grad_scale * sqrt(sum g^2), scale = clip_norm / max(norm, clip_norm) (grad_norm.hip)
at::Tensor grad_global_norm(const at::Tensor& g, double clip_norm, double grad_scale) {
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(g.is_cuda() && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous() && g.numel() >= 1,
              "grad_global_norm: a contiguous fp32 or bf16 GPU tensor of at least one element");
  auto out = at::empty({2}, g.options().dtype(at::kFloat));
  auto part = at::empty({kGradNormMaxBlocks}, out.options());
  grad_sumsq(gb ? nullptr : (const float*)g.data_ptr(), gb ? (const uint16_t*)g.data_ptr() : nullptr, g.numel(),
             (float*)part.data_ptr(), cur());
  grad_norm_finish((const float*)part.data_ptr(), grad_norm_blocks(g.numel()), (float)grad_scale, (float)clip_norm,
                   (float*)out.data_ptr(), cur());
  return out;
}

// {norm, scale, ok} of the non-finite guard over a flat fp32 or bf16 buffer (grad_guard.hip): norm and
// scale as grad_global_norm gives them (clip_norm = inf: no clipping, scale 1), ok = 1 if the norm is
// finite, else ok = 0 and scale = 0. Not finite means an inf / NaN element or a norm that overflows
// fp32. Adds 1 - ok to the int64 device counter `skipped`.
at::Tensor grad_guard(const at::Tensor& g, double grad_scale, double clip_norm, at::Tensor skipped) {
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(g.is_cuda() && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous() && g.numel() >= 1,
              "grad_guard: a contiguous fp32 or bf16 GPU tensor of at least one element");
  TORCH_CHECK(skipped.is_cuda() && skipped.scalar_type() == at::kLong && skipped.numel() == 1 &&
                  skipped.get_device() == g.get_device(),
              "grad_guard: skipped is one int64 element on g's device");
  TORCH_CHECK(clip_norm > 0.0, "grad_guard: clip_norm must be positive (inf: no clipping), got ", clip_norm);
  auto out = at::empty({3}, g.options().dtype(at::kFloat));
  auto part = at::empty({kGradNormMaxBlocks}, out.options());
  grad_sumsq(gb ? nullptr : (const float*)g.data_ptr(), gb ? (const uint16_t*)g.data_ptr() : nullptr, g.numel(),
             (float*)part.data_ptr(), cur());
  grad_guard_finish((const float*)part.data_ptr(), grad_norm_blocks(g.numel()), (float)grad_scale, (float)clip_norm,
                    (float*)out.data_ptr(), (int64_t*)skipped.data_ptr(), cur());
  return out;
}

// Gradient accumulation over micro-batches (csrc/grad_accum.h), one flat pass: first (no out) acc = g;
// no out: acc += g; out given: out = acc + g (acc untouched; out fp32 or bf16, and it may be g). g is
// fp32 or bf16. blocks / loads: 0 = the kernel's defaults (grad_accum_tuned: the probe's A/B).
void grad_accum_tuned(at::Tensor acc, const at::Tensor& g, c10::optional<at::Tensor> out, bool first, int64_t blocks,
                      int64_t loads) {
  const char* who = "grad_accum_flat";
  const int64_t n = acc.numel();
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.is_contiguous(), who, ": acc is a contiguous fp32 GPU tensor");
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(g.is_cuda() && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous(), who,
              ": g is a contiguous fp32 or bf16 GPU tensor");
  TORCH_CHECK(n >= 1 && g.numel() == n, who, ": acc and g hold the same number (>= 1) of elements, got ", n, " and ",
              g.numel());
  TORCH_CHECK(!(first && out), who, ": first (acc = g) takes no out");
  const bool ob = out && out->scalar_type() == at::kBFloat16;
  if (out)
    TORCH_CHECK(out->is_cuda() && (ob || out->scalar_type() == at::kFloat) && out->is_contiguous() && out->numel() == n,
                who, ": out is a contiguous fp32 or bf16 GPU tensor of acc's size");
  TORCH_CHECK(blocks >= 0 && blocks <= 65536 && (loads == 0 || loads == 1 || loads == 2 || loads == 4), who,
              ": blocks in [0, 65536], loads 0, 1, 2 or 4");
  GradAccumArgs a{};
  a.acc = (float*)acc.data_ptr();
  a.g = gb ? nullptr : (const float*)g.data_ptr();
  a.gbf = gb ? (const uint16_t*)g.data_ptr() : nullptr;
  a.out = out && !ob ? (float*)out->data_ptr() : nullptr;
  a.outbf = ob ? (uint16_t*)out->data_ptr() : nullptr;
  a.n = n;
  a.mode = out ? GA_EMIT : (first ? GA_STORE : GA_ADD);
  grad_accum(a, cur(), (int)blocks, (int)loads);
}
void grad_accum_flat(at::Tensor acc, const at::Tensor& g, c10::optional<at::Tensor> out, bool first) {
  grad_accum_tuned(acc, g, out, first, 0, 0);
}

void roofline_stream(at::Tensor p, at::Tensor m, at::Tensor v, const at::Tensor& g, at::Tensor pbf,
                     c10::optional<at::Tensor> x, int64_t blocks, int64_t unroll) {
  const int64_t n = p.numel();
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous() && n % 4 == 0, "roofline_stream: p");
  TORCH_CHECK(m.numel() == n && v.numel() == n && g.numel() == n && pbf.numel() == n, "roofline_stream: sizes");
  TORCH_CHECK(g.scalar_type() == at::kBFloat16 && pbf.scalar_type() == at::kBFloat16, "roofline_stream: bf16 g / pbf");
  const int64_t nx = x ? x->numel() : 0;
  TORCH_CHECK(nx % 4 == 0 && nx <= n && (!x || x->scalar_type() == at::kFloat), "roofline_stream: x");
  stream_floor((float*)p.data_ptr(), (float*)m.data_ptr(), (float*)v.data_ptr(), (const uint16_t*)g.data_ptr(),
               (uint16_t*)pbf.data_ptr(), x ? (const float*)x->data_ptr() : nullptr, n / 4, nx / 4, (int)blocks,
               (int)unroll, cur());
}

// the device lr_at() over a vector of steps (the numerical probe of the schedule tests)
at::Tensor lr_schedule_eval_op(const at::Tensor& steps, std::string kind, std::vector<double> params,
                               std::vector<int64_t> boundaries, std::vector<double> values) {
  TORCH_CHECK(steps.is_cuda() && steps.scalar_type() == at::kLong && steps.dim() == 1, "lr_schedule_eval: [n] int64 GPU steps");
  const LrSchedule sc = flat_schedule(params.empty() ? 0.0 : params[0], kind, params, boundaries, values);
  auto sc_steps = steps.contiguous();
  auto out = at::empty({sc_steps.numel()}, sc_steps.options().dtype(at::kFloat));
  lr_schedule_eval(sc, (const int64_t*)sc_steps.data_ptr(), (float*)out.data_ptr(), sc_steps.numel(), cur());
  return out;
}

void noop_op(int64_t blocks) { noop_launch((int)blocks, cur()); }

void kernarg_probe_op(const at::Tensor& src, at::Tensor dst, int64_t blocks, bool preload) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda() && src.scalar_type() == at::kFloat && dst.scalar_type() == at::kFloat &&
                  src.is_contiguous() && dst.is_contiguous(), "kernarg_probe: contiguous fp32 GPU tensors");
  TORCH_CHECK(blocks > 0 && src.numel() >= blocks * 64 && dst.numel() >= blocks * 64, "kernarg_probe: blocks x 64 elements");
  kernarg_probe((const float*)src.data_ptr(), (float*)dst.data_ptr(), (int)blocks, preload, cur());
}

at::Tensor to_bf16(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat, "to_bf16: fp32 GPU");
  auto xc = x.contiguous();
  auto y = at::empty(xc.sizes(), xc.options().dtype(at::kBFloat16));
  cast_f32_bf16((const float*)xc.data_ptr(), (uint16_t*)y.data_ptr(), xc.numel(), cur());
  return y;
}
}  // namespace

TORCH_LIBRARY(tfd, m) {
  m.def("crc32c(Tensor bytes, int init=0) -> int");
  m.impl("crc32c", c10::DispatchKey::CPU, &crc32c_op);
  m.def("adam_flat(Tensor(a!) p, Tensor(b!) m, Tensor(c!) v, Tensor g, Tensor(d!)? pbf, float lr, float b1, float b2, "
        "float eps, Tensor? step, float grad_scale=1.0, int t_offset=1, str lr_kind=\"constant\", "
        "float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[], Tensor? gscale=None, "
        "Tensor(f!)? ema=None, float ema_decay=0.0, bool ema_num_updates=False, Tensor? guard=None) -> ()");
  m.impl("adam_flat", c10::DispatchKey::CUDA, &adam_flat);
  m.def("adam_ranges_flat(Tensor(a!) p, Tensor(b!) m, Tensor(c!) v, Tensor g, Tensor(d!)? pbf, int[] beg, int[] n, "
        "float lr, float b1, float b2, float eps, Tensor? step, float grad_scale=1.0, int t_offset=1, "
        "str lr_kind=\"constant\", float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[], "
        "Tensor? gscale=None, Tensor(f!)? ema=None, float ema_decay=0.0, bool ema_num_updates=False, "
        "Tensor? guard=None) -> ()");
  m.impl("adam_ranges_flat", c10::DispatchKey::CUDA, &adam_ranges_flat);
  m.def("momentum_flat(Tensor(a!) p, Tensor(b!)? mom, Tensor g, Tensor(d!)? pbf, float lr, float momentum, "
        "float weight_decay, bool nesterov, float grad_scale=1.0, Tensor? step=None, int t_offset=1, "
        "str lr_kind=\"constant\", float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[], "
        "Tensor? gscale=None, Tensor? guard=None) -> ()");
  m.impl("momentum_flat", c10::DispatchKey::CUDA, &momentum_flat);
  m.def("momentum_ema_flat(Tensor(a!) p, Tensor(b!)? mom, Tensor g, Tensor(d!)? pbf, float lr, float momentum, "
        "float weight_decay, bool nesterov, float grad_scale=1.0, Tensor? step=None, int t_offset=1, "
        "str lr_kind=\"constant\", float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[], "
        "Tensor? gscale=None, *, Tensor(f!) ema, float ema_decay, bool ema_num_updates=False, "
        "Tensor? guard=None) -> ()");
  m.impl("momentum_ema_flat", c10::DispatchKey::CUDA, &momentum_ema_flat);
  m.def("ema_flat(Tensor(a!) e, Tensor p, float decay, bool num_updates=False, Tensor? step=None, int t_offset=0) -> ()");
  m.impl("ema_flat", c10::DispatchKey::CUDA, &ema_flat);
  m.def("grad_global_norm(Tensor g, float clip_norm, float grad_scale=1.0) -> Tensor");
  m.impl("grad_global_norm", c10::DispatchKey::CUDA, &grad_global_norm);
  m.def("grad_guard(Tensor g, float grad_scale, float clip_norm, Tensor(a!) skipped) -> Tensor");
  m.impl("grad_guard", c10::DispatchKey::CUDA, &grad_guard);
  m.def("grad_accum_flat(Tensor(a!) acc, Tensor g, Tensor(b!)? out=None, bool first=False) -> ()");
  m.impl("grad_accum_flat", c10::DispatchKey::CUDA, &grad_accum_flat);
  m.def("grad_accum_tuned(Tensor(a!) acc, Tensor g, Tensor(b!)? out, bool first, int blocks, int loads) -> ()");
  m.impl("grad_accum_tuned", c10::DispatchKey::CUDA, &grad_accum_tuned);
  m.def("roofline_stream(Tensor(a!) p, Tensor(b!) m, Tensor(c!) v, Tensor g, Tensor(d!) pbf, Tensor? x, int blocks, "
        "int unroll) -> ()");
  m.impl("roofline_stream", c10::DispatchKey::CUDA, &roofline_stream);
  m.def("lr_schedule_eval(Tensor steps, str kind, float[] params, int[] boundaries=[], float[] values=[]) -> Tensor");
  m.impl("lr_schedule_eval", c10::DispatchKey::CUDA, &lr_schedule_eval_op);
  m.def("noop(int blocks) -> ()");
  m.impl("noop", c10::DispatchKey::CompositeExplicitAutograd, &noop_op);
  m.def("kernarg_probe(Tensor src, Tensor(a!) dst, int blocks, bool preload) -> ()");
  m.impl("kernarg_probe", c10::DispatchKey::CUDA, &kernarg_probe_op);
  m.def("to_bf16(Tensor x) -> Tensor");
  m.impl("to_bf16", c10::DispatchKey::CUDA, &to_bf16);
}

}  // namespace tfd
