// Non-finite guard: the finish of the global gradient norm (grad_norm.hip) that also decides whether
// the optimizer step is applied. Stage 1 is grad_sumsq, unchanged; this finish sums its partials as
// grad_norm_finish does -- one block, fp64, a fixed order -- and writes {norm, scale, ok}:
//   norm  = grad_scale * sqrt(sum), cast to fp32            (what grad_norm_finish writes)
//   scale = clip_norm / max(norm, clip_norm)                (likewise; clip_norm = +inf clips nothing:
//           it is taken as FLT_MAX, so scale is exactly 1 for every finite norm and not inf / inf)
//   ok    = 1 if norm is finite, else 0 -- and then scale = 0
// "Not finite" is said of that fp32 norm: any inf or NaN element makes its square, its block's partial
// and the sum non-finite; so do finite gradients whose sum of squares overflows fp32 in stage 1 or
// whose scaled norm overflows the cast. Those steps are skipped as well: a gradient whose norm fp32
// cannot hold has no usable clip factor or trust ratio either.
// The thread that writes ok also adds 1 - ok to the int64 counter of skipped steps, a plain
// read-modify-write by one thread of one block: no atomics and nothing to zero, so every replay of a
// captured graph counts its own skipped steps.
#include <float.h>
#include <math.h>

#include "../common.h"
#include "../tfd_kernels.h"

namespace tfd {
namespace {

constexpr int kGuardThreads = 256;

__global__ __launch_bounds__(kGuardThreads) void grad_guard_finish_kernel(const float* __restrict__ partials, int nb,
                                                                          float grad_scale, float clip_norm,
                                                                          float* __restrict__ out,
                                                                          int64_t* __restrict__ skipped) {
  __shared__ double acc[kGuardThreads];
  // the counter's load goes out first (a uniform address under no branch: one scalar load), not as a
  // round trip of its own after the tree
  const int64_t count = *skipped;
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += kGuardThreads) s += (double)partials[i];
  acc[threadIdx.x] = s;
  __syncthreads();
  for (int o = kGuardThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)((double)grad_scale * sqrt(acc[0]));
    const float c = clip_norm < FLT_MAX ? clip_norm : FLT_MAX;
    // all exponent bits set: inf or NaN (a bit test, so no fast-math flag can fold it away)
    const bool ok = (__float_as_uint(norm) & 0x7F800000u) != 0x7F800000u;
    out[0] = norm;
    out[1] = ok ? c / (norm > c ? norm : c) : 0.f;
    out[2] = ok ? 1.f : 0.f;
    *skipped = count + (ok ? 0 : 1);
  }
}

}  // namespace

void grad_guard_finish(const float* partials, int nb, float grad_scale, float clip_norm, float* out, int64_t* skipped,
                       hipStream_t s) {
  grad_guard_finish_kernel<<<1, kGuardThreads, 0, s>>>(partials, nb, grad_scale, clip_norm, out, skipped);
}

}  // namespace tfd
