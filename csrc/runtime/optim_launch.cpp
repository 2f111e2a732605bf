// The flat optimizers' launch by variant (optim_launch.h): the only callers of the clip, EMA and guard
// launchers of tfd_kernels.h.
#include "../optim_launch.h"

namespace tfd {

void adam_launch(const AdamArgs& a, const OptMods& m, hipStream_t s) {
  switch (opt_variant(m)) {
    case OptVariant::Plain: return adam_apply(a, s);
    case OptVariant::Clip: return adam_apply_clip(opt_clip_args(a, m), s);
    case OptVariant::Ema: return adam_apply_ema(opt_ema_args(a, m), s);
    case OptVariant::Guard: return adam_apply_guard(opt_guard_args(a, m), s);
    case OptVariant::EmaGuard: return adam_apply_guard(opt_ema_guard_args(a, m), s);
  }
}

void sgd_launch(const SgdArgs& a, const OptMods& m, hipStream_t s) {
  switch (opt_variant(m)) {
    case OptVariant::Plain: return sgd_apply(a, s);
    case OptVariant::Clip: return sgd_apply_clip(opt_clip_args(a, m), s);
    case OptVariant::Ema: return sgd_apply_ema(opt_ema_args(a, m), s);
    case OptVariant::Guard: return sgd_apply_guard(opt_guard_args(a, m), s);
    case OptVariant::EmaGuard: return sgd_apply_guard(opt_ema_guard_args(a, m), s);
  }
}

void adam_launch_ranges(const AdamArgs& a, const OptMods& m, int nr, const int64_t* beg, const int64_t* n, hipStream_t s) {
  switch (opt_ranges_variant(m)) {
    case OptVariant::Plain: return adam_apply_ranges(a, nr, beg, n, s);
    case OptVariant::Clip: return adam_ranges_clip(opt_clip_args(a, m), nr, beg, n, s);
    default: return adam_ranges_ema(opt_ema_args(a, m), nr, beg, n, s);  // Ema: the guard was refused above
  }
}

}  // namespace tfd
