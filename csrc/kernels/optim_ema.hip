// The flat optimizer kernels with the moving average of the weights (csrc/optim_kernels.h, csrc/ema.h):
// the instantiations over AdamEmaArgs / SgdEmaArgs. They are the clip variant -- schedule evaluated on
// the device, gradient multiplier grad_scale * *gscale, gscale a device 1.0f without clipping -- plus
// one 4-B load and one 4-B store per element for the shadow, whose new value e' = fmaf(1 - d_t,
// p' - e, e) is formed from p' while the optimizer holds it in registers. A code object of their own:
// optim.hip's, optim_sched.hip's and optim_clip.hip's stay what the paths without EMA always ran.
// ema_apply is the same update as a pass of its own (12 B per element): for updates that are not one
// of these kernels, and the device reference the fused variants equal bit for bit.
#include "../optim_kernels.h"

namespace tfd {
namespace {

__global__ __launch_bounds__(kOptThreads) void ema_kernel(float* __restrict__ e, const float* __restrict__ p, int64_t n,
                                                          float decay, int num_updates, const int64_t* __restrict__ step,
                                                          int t_offset) {
  const int64_t stride = (int64_t)gridDim.x * kOptThreads;
  const int64_t i0 = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
  const bool v4 = ((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
  const int64_t n4 = v4 ? n >> 2 : 0;
  // the first item's operands are loaded before t (a dependent load of the step counter) is awaited
  f32x4 e4{}, p4{};
  if (i0 < n4) {
    e4 = reinterpret_cast<const f32x4*>(e)[i0];
    p4 = reinterpret_cast<const f32x4*>(p)[i0];
  }
  const float omd = ema_omd_at(decay, num_updates, (step ? *step : 0) + t_offset);
  for (int64_t i = i0; i < n4; i += stride) {
    if (i != i0) {
      e4 = reinterpret_cast<const f32x4*>(e)[i];
      p4 = reinterpret_cast<const f32x4*>(p)[i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) e4[j] = ema_step(e4[j], p4[j], omd);
    reinterpret_cast<f32x4*>(e)[i] = e4;
  }
  for (int64_t i = (n4 << 2) + i0; i < n; i += stride) e[i] = ema_step(e[i], p[i], omd);
}

}  // namespace

void adam_apply_ema(const AdamEmaArgs& a, hipStream_t s) {
  adam_kernel<<<blocks_for(a.k.a.n, 4), kOptThreads, 0, s>>>(a);
}
void adam_ranges_ema(const AdamEmaArgs& a, int nr, const int64_t* beg, const int64_t* n, hipStream_t s) {
  int nb = 0;
  const AdamRanges r = make_adam_ranges("adam_ranges_ema", nr, beg, n, &nb);
  adam_ranges_kernel<<<nb, kOptThreads, 0, s>>>(a, r);
}
void sgd_apply_ema(const SgdEmaArgs& a, hipStream_t s) {
  sgd_kernel<<<blocks_for(a.k.a.n, 1), kOptThreads, 0, s>>>(a);
}
void ema_apply(float* e, const float* p, int64_t n, float decay, int num_updates, const int64_t* step, int t_offset,
               hipStream_t s) {
  if (n > 0) ema_kernel<<<blocks_for(n, 4), kOptThreads, 0, s>>>(e, p, n, decay, num_updates, step, t_offset);
}

}  // namespace tfd
