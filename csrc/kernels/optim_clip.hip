// The flat optimizer kernels under global-norm clipping (csrc/optim_kernels.h): the instantiations
// over AdamClipArgs / SgdClipArgs, whose gradient multiplier is grad_scale * *gscale with gscale the
// clip factor grad_norm.hip left on the device. They carry the LrSchedule, so clipping composes with
// every schedule. A code object of their own: optim.hip's and optim_sched.hip's stay what the
// unclipped paths always ran.
#include "../optim_kernels.h"

namespace tfd {

void adam_apply_clip(const AdamClipArgs& a, hipStream_t s) {
  adam_kernel<<<blocks_for(a.a.n, 4), kOptThreads, 0, s>>>(a);
}
void adam_ranges_clip(const AdamClipArgs& a, int nr, const int64_t* beg, const int64_t* n, hipStream_t s) {
  int nb = 0;
  const AdamRanges r = make_adam_ranges("adam_ranges_clip", nr, beg, n, &nb);
  adam_ranges_kernel<<<nb, kOptThreads, 0, s>>>(a, r);
}
void sgd_apply_clip(const SgdClipArgs& a, hipStream_t s) {
  sgd_kernel<<<blocks_for(a.a.n, 1), kOptThreads, 0, s>>>(a);
}

}  // namespace tfd
