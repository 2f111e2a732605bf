// Torch ops of the layer-wise optimizers (csrc/layerwise.h, csrc/kernels/optim_layerwise.hip):
// tfd::lamb_flat, tfd::lars_flat, tfd::layer_norms. A fragment of the `tfd` library, as conv_ops.cpp is.
// Ops run on the caller's current HIP stream. The trailing arguments are read by flat_op_args.h.
#include "../layerwise_kernels.h"
#include "flat_op_args.h"

namespace tfd {
namespace {
using namespace flat_op;  // cur, flat_schedule, flat_mods

// ---- layer-wise optimizers (csrc/layerwise.h, kernels/optim_layerwise.hip) ----
// The block table of a segment table `segs` (int64 CPU [S,3] rows of begin, length, flags) over
// buffers of `numel` elements, on x's device, with the partials and the [S,3] output the stages write.
struct LayerwisePlan {
  at::Tensor blocks, seg_blocks, partials, out;
  int nblocks, nsegs;
};
LayerwisePlan layerwise_plan(const at::Tensor& segs, int64_t numel, const at::Tensor& x, const char* who) {
  TORCH_CHECK(!segs.is_cuda() && segs.scalar_type() == at::kLong && segs.dim() == 2 && segs.size(1) == 3 && segs.size(0) >= 1,
              who, ": segs is an int64 CPU tensor [S,3] of (begin, length, flags)");
  const at::Tensor sc = segs.contiguous();
  const int64_t* row = (const int64_t*)sc.data_ptr();
  std::vector<LwSegment> sv((size_t)sc.size(0));
  for (size_t i = 0; i < sv.size(); ++i) {
    TORCH_CHECK(row[3 * i + 2] >= 0 && row[3 * i + 2] <= (LW_DECAY | LW_ADAPT), who, ": segment ", i, " has unknown flags");
    sv[i] = LwSegment{row[3 * i], row[3 * i + 1], (int)row[3 * i + 2]};
  }
  LwTable t;
  try {
    t = lw_build_table(sv.data(), sv.size(), kLwChunk, numel);
  } catch (const std::invalid_argument& e) {
    TORCH_CHECK(false, who, ": ", e.what());
  }
  auto to_dev = [&](const void* src, size_t bytes) {
    return at::from_blob(const_cast<void*>(src), {(int64_t)bytes}, at::TensorOptions().dtype(at::kByte)).to(x.device());
  };
  LayerwisePlan pl;
  pl.nblocks = (int)t.blocks.size();
  pl.nsegs = (int)t.segs.size();
  pl.blocks = to_dev(t.blocks.data(), t.blocks.size() * sizeof(LwBlock));
  pl.seg_blocks = to_dev(t.segs.data(), t.segs.size() * sizeof(LwSegBlocks));
  pl.partials = at::empty({pl.nblocks, 2}, x.options().dtype(at::kFloat));
  pl.out = at::empty({pl.nsegs, 3}, x.options().dtype(at::kFloat));
  return pl;
}
void layerwise_plan_args(LayerwiseArgs& a, const LayerwisePlan& pl) {
  a.blocks = (const LwBlock*)pl.blocks.data_ptr();
  a.segs = (const LwSegBlocks*)pl.seg_blocks.data_ptr();
  a.nblocks = pl.nblocks;
  a.nsegs = pl.nsegs;
  a.partials = (float*)pl.partials.data_ptr();
  a.out = (float*)pl.out.data_ptr();
}
// what lamb_flat and lars_flat share: the buffers' checks and every argument but the optimizer's own
LayerwiseArgs layerwise_args(const char* who, at::Tensor& p, at::Tensor& s1, const at::Tensor& g,
                             const c10::optional<at::Tensor>& pbf, const c10::optional<at::Tensor>& step, int64_t t_offset,
                             double grad_scale, const LrSchedule& sc, const c10::optional<at::Tensor>& gscale,
                             const c10::optional<at::Tensor>& ema, double ema_decay, bool ema_num_updates,
                             const c10::optional<at::Tensor>& guard) {
  const int64_t n = p.numel();
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous(), who, ": fp32 GPU params");
  TORCH_CHECK(s1.is_cuda() && s1.scalar_type() == at::kFloat && s1.is_contiguous() && s1.numel() == n, who,
              ": slots are contiguous fp32 GPU tensors of p's size");
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(g.is_cuda() && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous() && g.numel() == n, who,
              ": g is a contiguous fp32 or bf16 GPU tensor of p's size");
  TORCH_CHECK(!pbf || (pbf->is_cuda() && pbf->scalar_type() == at::kBFloat16 && pbf->is_contiguous() && pbf->numel() == n),
              who, ": pbf is a contiguous bf16 GPU tensor of p's size");
  TORCH_CHECK(!step || (step->scalar_type() == at::kLong && step->is_cuda() && step->numel() == 1), who, ": int64 GPU step");
  TORCH_CHECK(sc.kind == LR_CONSTANT || step, who, ": a schedule needs the device step tensor");
  TORCH_CHECK(!ema_num_updates || !ema || step, who, ": ema_num_updates needs the device step tensor");
  LayerwiseArgs a{};
  a.p = (float*)p.data_ptr();
  a.s1 = (float*)s1.data_ptr();
  a.g = gb ? nullptr : (const float*)g.data_ptr();
  a.gbf = gb ? (const uint16_t*)g.data_ptr() : nullptr;
  a.pbf = pbf ? (uint16_t*)pbf->data_ptr() : nullptr;
  a.sched = sc;
  a.step = step ? (const int64_t*)step->data_ptr() : nullptr;
  a.t_offset = (int)t_offset;
  a.grad_scale = (float)grad_scale;
  apply_mods(a, flat_mods(who, p, gscale, ema, ema_decay, ema_num_updates, guard, true));
  return a;
}

// LAMB over the variables of `segs`; returns [S,3] = {|p|, |u|, r} per variable (fp32, on the device).
// guard (here and in lars_flat): with its ok == 0 nothing is stored to p, the slots, pbf or ema, and the
// [S,3] result is unspecified.
at::Tensor lamb_flat(at::Tensor p, at::Tensor m, at::Tensor v, at::Tensor g, c10::optional<at::Tensor> pbf, at::Tensor segs,
                     double lr, double b1, double b2, double eps, double weight_decay, c10::optional<at::Tensor> step,
                     int64_t t_offset, double grad_scale, std::string lr_kind, std::vector<double> lr_params,
                     std::vector<int64_t> lr_boundaries, std::vector<double> lr_values, c10::optional<at::Tensor> gscale,
                     c10::optional<at::Tensor> ema, double ema_decay, bool ema_num_updates,
                     c10::optional<at::Tensor> guard) {
  const char* who = "lamb_flat";
  LayerwiseArgs a = layerwise_args(who, p, m, g, pbf, step, t_offset, grad_scale,
                                   flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values), gscale, ema, ema_decay,
                                   ema_num_updates, guard);
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == at::kFloat && v.is_contiguous() && v.numel() == p.numel(), who,
              ": slots are contiguous fp32 GPU tensors of p's size");
  const LayerwisePlan pl = layerwise_plan(segs, p.numel(), p, who);
  layerwise_plan_args(a, pl);
  a.s2 = (float*)v.data_ptr();
  a.beta1 = (float)b1;
  a.beta2 = (float)b2;
  a.eps = (float)eps;
  a.weight_decay = (float)weight_decay;
  lamb_apply(a, cur());
  return pl.out;
}

// LARS (momentum form, the rate folded into the accumulator); returns [S,3] = {|p|, |g|, r}
at::Tensor lars_flat(at::Tensor p, at::Tensor accum, at::Tensor g, c10::optional<at::Tensor> pbf, at::Tensor segs, double lr,
                     double momentum, double weight_decay, double eeta, double eps, c10::optional<at::Tensor> step,
                     int64_t t_offset, double grad_scale, std::string lr_kind, std::vector<double> lr_params,
                     std::vector<int64_t> lr_boundaries, std::vector<double> lr_values, c10::optional<at::Tensor> gscale,
                     c10::optional<at::Tensor> ema, double ema_decay, bool ema_num_updates,
                     c10::optional<at::Tensor> guard) {
  const char* who = "lars_flat";
  LayerwiseArgs a = layerwise_args(who, p, accum, g, pbf, step, t_offset, grad_scale,
                                   flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values), gscale, ema, ema_decay,
                                   ema_num_updates, guard);
  const LayerwisePlan pl = layerwise_plan(segs, p.numel(), p, who);
  layerwise_plan_args(a, pl);
  a.momentum = (float)momentum;
  a.eeta = (float)eeta;
  a.eps = (float)eps;
  a.weight_decay = (float)weight_decay;
  lars_apply(a, cur());
  return pl.out;
}

// the per-variable L2 norms of one fp32 or bf16 buffer: stages 1 and 2 alone (tests and probes)
at::Tensor layer_norms(const at::Tensor& x, at::Tensor segs) {
  const char* who = "layer_norms";
  const bool xb = x.scalar_type() == at::kBFloat16;
  TORCH_CHECK(x.is_cuda() && (xb || x.scalar_type() == at::kFloat) && x.is_contiguous() && x.numel() >= 1, who,
              ": a contiguous fp32 or bf16 GPU tensor of at least one element");
  const LayerwisePlan pl = layerwise_plan(segs, x.numel(), x, who);
  LayerwiseArgs a{};
  layerwise_plan_args(a, pl);
  a.g = xb ? nullptr : (const float*)x.data_ptr();
  a.gbf = xb ? (const uint16_t*)x.data_ptr() : nullptr;
  layer_norms_apply(a, cur());
  return pl.out.select(1, 0).contiguous();
}
int64_t layerwise_chunk() { return kLwChunk; }
}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("lamb_flat(Tensor(a!) p, Tensor(b!) m, Tensor(c!) v, Tensor g, Tensor(d!)? pbf, Tensor segs, float lr, float beta1, "
        "float beta2, float eps, float weight_decay, Tensor? step=None, int t_offset=1, float grad_scale=1.0, "
        "str lr_kind=\"constant\", float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[], "
        "Tensor? gscale=None, Tensor(f!)? ema=None, float ema_decay=0.0, bool ema_num_updates=False, "
        "Tensor? guard=None) -> Tensor");
  m.impl("lamb_flat", c10::DispatchKey::CUDA, &lamb_flat);
  m.def("lars_flat(Tensor(a!) p, Tensor(b!) accum, Tensor g, Tensor(d!)? pbf, Tensor segs, float lr, float momentum, "
        "float weight_decay, float eeta, float eps, Tensor? step=None, int t_offset=1, float grad_scale=1.0, "
        "str lr_kind=\"constant\", float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[], "
        "Tensor? gscale=None, Tensor(f!)? ema=None, float ema_decay=0.0, bool ema_num_updates=False, "
        "Tensor? guard=None) -> Tensor");
  m.impl("lars_flat", c10::DispatchKey::CUDA, &lars_flat);
  m.def("layer_norms(Tensor x, Tensor segs) -> Tensor");
  m.impl("layer_norms", c10::DispatchKey::CUDA, &layer_norms);
  m.def("layerwise_chunk() -> int");
  m.impl("layerwise_chunk", c10::DispatchKey::CompositeExplicitAutograd, &layerwise_chunk);
}

}  // namespace tfd
