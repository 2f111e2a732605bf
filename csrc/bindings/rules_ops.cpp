// Torch ops of RMSProp and Adagrad (csrc/optim_rules.h, csrc/kernels/optim_rules.hip): tfd::rmsprop_flat,
// tfd::adagrad_flat. A fragment of the `tfd` library, as layerwise_ops.cpp is. Ops run on the caller's
// current HIP stream. The trailing arguments are read by flat_op_args.h.
#include "../optim_rules.h"
#include "flat_op_args.h"

namespace tfd {
namespace {
using namespace flat_op;  // cur, flat_schedule, step_ptr, flat_mods

float* slot_ptr(const at::Tensor& s, const at::Tensor& p, const char* who, const char* name) {
  TORCH_CHECK(s.is_cuda() && s.get_device() == p.get_device() && s.scalar_type() == at::kFloat && s.is_contiguous() &&
                  s.numel() == p.numel(),
              who, ": ", name, " is a contiguous fp32 tensor of p's size on p's device");
  return (float*)s.data_ptr();
}

// what the two ops share: the buffers' checks and every argument but the rule's own
RuleArgs rule_args(const char* who, at::Tensor& p, const at::Tensor& g, const c10::optional<at::Tensor>& pbf,
                   const c10::optional<at::Tensor>& step, int64_t t_offset, double grad_scale, const LrSchedule& sc,
                   const c10::optional<at::Tensor>& gscale, const c10::optional<at::Tensor>& ema, double ema_decay,
                   bool ema_num_updates, const c10::optional<at::Tensor>& guard) {
  const int64_t n = p.numel();
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous() && n >= 1, who,
              ": p is a contiguous fp32 GPU tensor of at least one element");
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(g.is_cuda() && g.get_device() == p.get_device() && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous() &&
                  g.numel() == n,
              who, ": g is a contiguous fp32 or bf16 tensor of p's size on p's device");
  TORCH_CHECK(!pbf || (pbf->is_cuda() && pbf->get_device() == p.get_device() && pbf->scalar_type() == at::kBFloat16 &&
                       pbf->is_contiguous() && pbf->numel() == n),
              who, ": pbf is a contiguous bf16 tensor of p's size on p's device");
  const int64_t* step_p = step_ptr(step, p, who);
  TORCH_CHECK(sc.kind == LR_CONSTANT || step, who, ": a schedule needs the device step tensor");
  TORCH_CHECK(!ema_num_updates || !ema || step, who, ": ema_num_updates needs the device step tensor");
  RuleArgs a{};
  a.p = (float*)p.data_ptr();
  a.g = gb ? nullptr : (const float*)g.data_ptr();
  a.gbf = gb ? (const uint16_t*)g.data_ptr() : nullptr;
  a.pbf = pbf ? (uint16_t*)pbf->data_ptr() : nullptr;
  a.n = n;
  a.sched = sc;
  a.step = step_p;
  a.t_offset = (int)t_offset;
  a.grad_scale = (float)grad_scale;
  apply_mods(a, flat_mods(who, p, gscale, ema, ema_decay, ema_num_updates, guard, true));
  return a;
}
// the launchers' own checks (alignment) as torch errors
template <class F>
void launch(F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    TORCH_CHECK(false, e.what());
  }
}

// mg given = the centered rule (ApplyCenteredRMSProp); without it the plain one. mom is stored by every call,
// and read only when momentum != 0 (optim_rules.h). guard (here and in adagrad_flat): with its ok == 0 nothing
// is stored to p, the slots, pbf or ema.
void rmsprop_flat(at::Tensor p, at::Tensor ms, at::Tensor mom, at::Tensor g, c10::optional<at::Tensor> pbf, double lr,
                  double decay, double momentum, double epsilon, c10::optional<at::Tensor> mg,
                  c10::optional<at::Tensor> step, int64_t t_offset, double grad_scale, c10::optional<at::Tensor> gscale,
                  c10::optional<at::Tensor> ema, double ema_decay, bool ema_num_updates, c10::optional<at::Tensor> guard,
                  std::string lr_kind, std::vector<double> lr_params, std::vector<int64_t> lr_boundaries,
                  std::vector<double> lr_values) {
  const char* who = "rmsprop_flat";
  const bool centered = mg.has_value();  // the centered rule is the one with the mg slot
  RuleArgs a = rule_args(who, p, g, pbf, step, t_offset, grad_scale,
                         flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values), gscale, ema, ema_decay,
                         ema_num_updates, guard);
  a.s1 = slot_ptr(ms, p, who, "ms");
  a.s2 = slot_ptr(mom, p, who, "mom");
  if (centered) a.s3 = slot_ptr(*mg, p, who, "mg");
  a.decay = (float)decay;
  a.momentum = (float)momentum;
  a.eps = (float)epsilon;
  launch([&] { rmsprop_apply(a, centered, cur()); });
}

void adagrad_flat(at::Tensor p, at::Tensor accum, at::Tensor g, c10::optional<at::Tensor> pbf, double lr,
                  c10::optional<at::Tensor> step, int64_t t_offset, double grad_scale, c10::optional<at::Tensor> gscale,
                  c10::optional<at::Tensor> ema, double ema_decay, bool ema_num_updates, c10::optional<at::Tensor> guard,
                  std::string lr_kind, std::vector<double> lr_params, std::vector<int64_t> lr_boundaries,
                  std::vector<double> lr_values) {
  const char* who = "adagrad_flat";
  RuleArgs a = rule_args(who, p, g, pbf, step, t_offset, grad_scale,
                         flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values), gscale, ema, ema_decay,
                         ema_num_updates, guard);
  a.s1 = slot_ptr(accum, p, who, "accum");
  launch([&] { adagrad_apply(a, cur()); });
}
// the largest grid x block x 4 of the launchers: above it a buffer takes a second grid-stride pass
int64_t rules_grid_elems() { return (int64_t)rules_max_blocks() * rules_threads() * 4; }
}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("rmsprop_flat(Tensor(a!) p, Tensor(b!) ms, Tensor(c!) mom, Tensor g, Tensor(d!)? pbf, float lr, float decay, "
        "float momentum, float epsilon, Tensor(e!)? mg=None, *, Tensor? step=None, int t_offset=1, "
        "float grad_scale=1.0, Tensor? gscale=None, Tensor(f!)? ema=None, float ema_decay=0.0, "
        "bool ema_num_updates=False, Tensor? guard=None, str lr_kind=\"constant\", float[] lr_params=[], "
        "int[] lr_boundaries=[], float[] lr_values=[]) -> ()");
  m.impl("rmsprop_flat", c10::DispatchKey::CUDA, &rmsprop_flat);
  m.def("adagrad_flat(Tensor(a!) p, Tensor(b!) accum, Tensor g, Tensor(d!)? pbf, float lr, *, Tensor? step=None, "
        "int t_offset=1, float grad_scale=1.0, Tensor? gscale=None, Tensor(f!)? ema=None, float ema_decay=0.0, "
        "bool ema_num_updates=False, Tensor? guard=None, str lr_kind=\"constant\", float[] lr_params=[], "
        "int[] lr_boundaries=[], float[] lr_values=[]) -> ()");
  m.impl("adagrad_flat", c10::DispatchKey::CUDA, &adagrad_flat);
  m.def("rules_grid_elems() -> int");
  m.impl("rules_grid_elems", c10::DispatchKey::CompositeExplicitAutograd, &rules_grid_elems);
}

}  // namespace tfd
