// The flat optimizer kernels under the non-finite guard (csrc/optim_kernels.h): the instantiations over
// GuardArgs<AdamClipArgs / SgdClipArgs / AdamEmaArgs / SgdEmaArgs>. They are the clip and the EMA
// variants plus one 4-B uniform load -- ok of grad_guard.hip's {norm, scale, ok}, issued beside the
// step counter and the clip factor, after the first item's operand loads -- and one wave-uniform branch
// before the first store: with ok == 0 the kernel returns and p, m, v / accum, the bf16 shadow and the
// EMA shadow keep their bits. With ok == 1 the update is the wrapped variant's, bit for bit. A code
// object of their own: optim.hip's, optim_sched.hip's, optim_clip.hip's and optim_ema.hip's stay what
// the unguarded paths always ran.
#include "../optim_kernels.h"

namespace tfd {

void adam_apply_guard(const AdamGuardArgs& a, hipStream_t s) {
  adam_kernel<<<blocks_for(a.k.a.n, 4), kOptThreads, 0, s>>>(a);
}
void adam_apply_guard(const AdamEmaGuardArgs& a, hipStream_t s) {
  adam_kernel<<<blocks_for(a.k.k.a.n, 4), kOptThreads, 0, s>>>(a);
}
void sgd_apply_guard(const SgdGuardArgs& a, hipStream_t s) {
  sgd_kernel<<<blocks_for(a.k.a.n, 1), kOptThreads, 0, s>>>(a);
}
void sgd_apply_guard(const SgdEmaGuardArgs& a, hipStream_t s) {
  sgd_kernel<<<blocks_for(a.k.k.a.n, 1), kOptThreads, 0, s>>>(a);
}

}  // namespace tfd
