// Which instantiation of a flat optimizer kernel a step launches: the one place on the host that knows. The
// device side is optim_kernels.h: the kernels are templates over their argument struct, and the wrappers of
// tfd_kernels.h select the clip, EMA and guard instantiations, each in a code object of its own. A new modifier
// of the update is added in this header and nowhere else on the host. Host-only: no .hip file includes it.
//
//   guard  ema   clip   variant    launcher                               code object
//   no     no    no     Plain      adam_apply / sgd_apply                 optim.hip, optim_sched.hip
//   no     no    yes    Clip       adam_apply_clip / sgd_apply_clip       optim_clip.hip
//   no     yes   any    Ema        adam_apply_ema / sgd_apply_ema         optim_ema.hip
//   yes    no    any    Guard      *_apply_guard(GuardArgs<ClipArgs>)     optim_guard.hip
//   yes    yes   any    EmaGuard   *_apply_guard(GuardArgs<EmaArgs>)      optim_guard.hip
// "any": the variant reads a clip factor either way; without clipping, OptMods::one (x * 1.0f is exact).
#pragma once
#include <stdexcept>

#include "tfd_kernels.h"

namespace tfd {

// What a step adds to the bare update; every field is optional.
struct OptMods {
  const float* gscale = nullptr;  // device clip factor
  const float* ok = nullptr;      // the non-finite guard's device flag
  float* ema = nullptr;           // the shadow, already offset to the range's start
  float ema_decay = 0.f;
  int ema_num_updates = 0;
  const float* one = nullptr;     // a device 1.0f: the clip factor of a variant that reads one without clipping
};

enum class OptVariant { Plain, Clip, Ema, Guard, EmaGuard };
constexpr OptVariant opt_variant(bool clip, bool ema, bool guard) {
  return guard ? (ema ? OptVariant::EmaGuard : OptVariant::Guard)
               : ema ? OptVariant::Ema : clip ? OptVariant::Clip : OptVariant::Plain;
}
inline OptVariant opt_variant(const OptMods& m) { return opt_variant(m.gscale != nullptr, m.ema != nullptr, m.ok != nullptr); }
// the ranges form (ZeRO-1) has no guarded instantiation, and ZeRO-1 refuses the guard
inline OptVariant opt_ranges_variant(const OptMods& m) {
  if (m.ok) throw std::runtime_error("adam_launch_ranges: no guarded ranges kernel exists (the non-finite guard needs the whole gradient)");
  return opt_variant(m);
}

// the clip factor a variant reads: the step's, or the device 1.0f
inline const float* opt_clip_factor(const OptMods& m) {
  if (m.gscale) return m.gscale;
  if (!m.one) throw std::runtime_error("optimizer launch: the variant reads a clip factor, and neither gscale nor the device 1.0f was given");
  return m.one;
}
inline AdamClipArgs opt_clip_args(const AdamArgs& a, const OptMods& m) { return AdamClipArgs{a, opt_clip_factor(m)}; }
inline SgdClipArgs opt_clip_args(const SgdArgs& a, const OptMods& m) { return SgdClipArgs{a, opt_clip_factor(m)}; }
inline AdamEmaArgs opt_ema_args(const AdamArgs& a, const OptMods& m) {
  return AdamEmaArgs{opt_clip_args(a, m), m.ema, m.ema_decay, m.ema_num_updates};
}
inline SgdEmaArgs opt_ema_args(const SgdArgs& a, const OptMods& m) {
  return SgdEmaArgs{opt_clip_args(a, m), m.ema, m.ema_decay, m.ema_num_updates};
}
template <class A>
auto opt_guard_args(const A& a, const OptMods& m) { return GuardArgs<decltype(opt_clip_args(a, m))>{opt_clip_args(a, m), m.ok}; }
template <class A>
auto opt_ema_guard_args(const A& a, const OptMods& m) { return GuardArgs<decltype(opt_ema_args(a, m))>{opt_ema_args(a, m), m.ok}; }

// RuleArgs (optim_rules.h) and LayerwiseArgs (layerwise_kernels.h) carry the modifiers as fields of the
// same five names; their kernels always read a clip factor.
template <class A>
void apply_mods(A& a, const OptMods& m) {
  a.gscale = opt_clip_factor(m);
  a.ok = m.ok;
  a.ema = m.ema;
  a.ema_decay = m.ema_decay;
  a.ema_num_updates = m.ema_num_updates;
}

// The launch of the variant `m` selects (optim_launch.cpp); the constant / scheduled split stays in the launchers.
void adam_launch(const AdamArgs& a, const OptMods& m, hipStream_t s);
void sgd_launch(const SgdArgs& a, const OptMods& m, hipStream_t s);
// adam_apply_ranges' form: up to 3 ranges of the flat buffers in one launch; throws when m.ok is set
void adam_launch_ranges(const AdamArgs& a, const OptMods& m, int nr, const int64_t* beg, const int64_t* n, hipStream_t s);

}  // namespace tfd
