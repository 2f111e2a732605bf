// What the flat optimizer ops share when they read their trailing arguments (ops.cpp, layerwise_ops.cpp,
// rules_ops.cpp): the schedule keywords, the device clip factor, the non-finite guard's ok, the EMA shadow and the
// device 1.0f that stands in for the clip factor when the caller clips nothing -- and flat_mods, which reads them
// into the OptMods of optim_launch.h. Host-only, header-only; every tensor is checked to live on p's device.
#pragma once
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../lr_schedule.h"
#include "../optim_launch.h"

namespace tfd {
namespace flat_op {

inline hipStream_t cur() { return c10::hip::getCurrentHIPStream().stream(); }

// the trailing schedule arguments, as adam_flat takes them: no lr_params = constant at `lr`
inline LrSchedule flat_schedule(double lr, const std::string& kind, const std::vector<double>& params,
                                const std::vector<int64_t>& boundaries, const std::vector<double>& values) {
  if (kind == "constant" && params.empty()) return lr_constant((float)lr);
  TORCH_CHECK(params.empty() || (float)params[0] == (float)lr, "lr (", lr, ") and lr_params[0] (", params[0], ") disagree");
  try {
    return make_lr_schedule(kind, params.empty() ? std::vector<double>{lr} : params, boundaries, values);
  } catch (const std::invalid_argument& e) {
    TORCH_CHECK(false, e.what());
  }
}
inline bool on_device_of(const at::Tensor& t, const at::Tensor& p) { return t.is_cuda() && t.get_device() == p.get_device(); }
// gscale: the device clip factor, one fp32 element
inline const float* clip_factor(const at::Tensor& t, const at::Tensor& p, const char* who) {
  TORCH_CHECK(on_device_of(t, p) && t.scalar_type() == at::kFloat && t.numel() == 1, who,
              ": gscale is one fp32 element on p's device");
  return (const float*)t.data_ptr();
}
// guard: the non-finite guard's device ok, the [3] result of grad_guard or a one-element view of its ok
inline const float* guard_ok(const at::Tensor& t, const at::Tensor& p, const char* who) {
  TORCH_CHECK(on_device_of(t, p) && t.scalar_type() == at::kFloat && t.is_contiguous() && (t.numel() == 3 || t.numel() == 1),
              who, ": guard is grad_guard's fp32 [3] result or its ok element, on p's device");
  return (const float*)t.data_ptr() + (t.numel() == 3 ? 2 : 0);
}
inline float* ema_shadow(const at::Tensor& e, const at::Tensor& p, double decay, const char* who) {
  TORCH_CHECK(on_device_of(e, p) && e.scalar_type() == at::kFloat && e.is_contiguous() && e.numel() == p.numel(), who,
              ": ema is a contiguous fp32 tensor of p's size on p's device");
  TORCH_CHECK(decay > 0.0 && decay < 1.0, who, ": ema_decay must be in (0, 1), got ", decay);
  return (float*)e.data_ptr();
}
inline const int64_t* step_ptr(const c10::optional<at::Tensor>& step, const at::Tensor& p, const char* who) {
  TORCH_CHECK(!step || (step->scalar_type() == at::kLong && on_device_of(*step, p) && step->numel() == 1), who,
              ": step is one int64 element on p's device");
  return step ? (const int64_t*)step->data_ptr() : nullptr;
}
// the clip factor when the caller clips nothing: one fp32 1.0 per device, made once (copied from the
// host, so it is ready when the call returns). One cache for every op that includes this header.
inline const float* unit_scale(const at::Tensor& like) {
  static at::Tensor one[64];
  const int d = like.get_device();
  TORCH_CHECK(d >= 0 && d < 64, "device index");
  if (!one[d].defined()) one[d] = at::ones({1}, at::kFloat).to(like.device());
  return (const float*)one[d].data_ptr();
}
// The trailing gscale / ema / guard of a flat op as the modifiers of its update. always_clip: the op's kernel
// reads a clip factor in every variant (RuleArgs, LayerwiseArgs). The device 1.0f is made at the first call
// that needs it, so an op that needs none allocates nothing (it may be inside a capture).
inline OptMods flat_mods(const char* who, const at::Tensor& p, const c10::optional<at::Tensor>& gscale,
                         const c10::optional<at::Tensor>& ema, double ema_decay, bool ema_num_updates,
                         const c10::optional<at::Tensor>& guard, bool always_clip = false) {
  OptMods m;
  if (gscale) m.gscale = clip_factor(*gscale, p, who);
  if (ema) {
    m.ema = ema_shadow(*ema, p, ema_decay, who);
    m.ema_decay = (float)ema_decay;
    m.ema_num_updates = ema_num_updates ? 1 : 0;
  }
  if (guard) m.ok = guard_ok(*guard, p, who);
  if (!m.gscale && (always_clip || opt_variant(m) != OptVariant::Plain)) m.one = unit_scale(p);
  return m;
}

}  // namespace flat_op
}  // namespace tfd
