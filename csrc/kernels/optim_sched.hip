// The flat optimizer kernels with a learning-rate schedule evaluated on the device (csrc/optim_kernels.h,
// csrc/lr_schedule.h): the instantiations over AdamArgs / SgdArgs, in a code object of their own so
// that optim.hip's stays what the default (constant-rate) path always ran; and the schedule's probe.
#include "../optim_kernels.h"

namespace tfd {
namespace {

// debug probe: the schedule's device function over a vector of steps (one block)
__global__ __launch_bounds__(kOptThreads) void lr_schedule_eval_kernel(LrSchedule sc, const int64_t* __restrict__ steps,
                                                                       float* __restrict__ out, int64_t n) {
  for (int64_t i = threadIdx.x; i < n; i += kOptThreads) out[i] = lr_at(sc, steps[i]);
}

}  // namespace

void adam_apply_sched(const AdamArgs& a, hipStream_t s) {
  adam_kernel<<<blocks_for(a.n, 4), kOptThreads, 0, s>>>(a);
}
void adam_ranges_sched(const AdamArgs& a, const AdamRanges& r, int blocks, hipStream_t s) {
  adam_ranges_kernel<<<blocks, kOptThreads, 0, s>>>(a, r);
}
void sgd_apply_sched(const SgdArgs& a, hipStream_t s) {
  sgd_kernel<<<blocks_for(a.n, 1), kOptThreads, 0, s>>>(a);
}
void lr_schedule_eval(const LrSchedule& sc, const int64_t* steps, float* out, int64_t n, hipStream_t s) {
  if (n > 0) lr_schedule_eval_kernel<<<1, kOptThreads, 0, s>>>(sc, steps, out, n);
}

}  // namespace tfd
