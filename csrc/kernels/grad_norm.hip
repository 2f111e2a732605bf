// Global gradient norm on the device: the norm and the clip factor of tf.clip_by_global_norm, produced
// inside the step graph for the clip instantiations of the optimizer kernels (optim_clip.hip).
//   stage 1 (grad_sumsq): sum of squares of a flat fp32 or bf16 buffer, one fp32 partial per block.
//     The grid is a function of n alone, every lane adds in a fixed order, the wave reduction is a
//     fixed butterfly and the four waves meet through LDS in a fixed order: no atomics, so the
//     partials -- and the norm -- are bit-identical run to run. The partials are plain stores that
//     cover [0, gridDim.x) every call: nothing to zero beforehand.
//   stage 2 (grad_norm_finish): one block sums the partials in a fixed order in fp64 and writes
//     {norm, scale}: norm = grad_scale * sqrt(sum), scale = clip_norm / max(norm, clip_norm) in fp32,
//     exactly 1 while norm <= clip_norm. No special case for non-finite norms: inf gives scale 0; a NaN
//     norm fails the compare, leaves scale at 1, and the NaN gradients propagate as without clipping.
//     (The finish that does make a case of them, and skips the step, is grad_guard.hip's.)
#include <math.h>

#include "../common.h"
#include "../tfd_kernels.h"

namespace tfd {
namespace {

constexpr int kNormThreads = 256;
constexpr int kNormLoads = 4;  // 16-byte (fp32) / 8-byte (bf16) loads in flight per lane before the first add

template <bool BF>
__device__ __forceinline__ f32x4 norm_load4(const void* x, int64_t i) {
  if constexpr (BF) {
    const uint2 gb = reinterpret_cast<const uint2*>(x)[i];
    return f32x4{bf2f((uint16_t)(gb.x & 0xFFFF)), bf2f((uint16_t)(gb.x >> 16)), bf2f((uint16_t)(gb.y & 0xFFFF)),
                 bf2f((uint16_t)(gb.y >> 16))};
  } else {
    return reinterpret_cast<const f32x4*>(x)[i];
  }
}
template <bool BF>
__device__ __forceinline__ float norm_load1(const void* x, int64_t i) {
  if constexpr (BF) return bf2f(reinterpret_cast<const uint16_t*>(x)[i]);
  else return reinterpret_cast<const float*>(x)[i];
}

// n4: the number of 4-element vectors read with vector loads (n / 4, or 0 for a base pointer that
// is not aligned to them); the elements [4 * n4, n) are read one by one
template <bool BF>
__global__ __launch_bounds__(kNormThreads) void grad_sumsq_kernel(const void* __restrict__ x, int64_t n4, int64_t n,
                                                                  float* __restrict__ partials) {
  const int64_t stride = (int64_t)gridDim.x * kNormThreads;
  const int64_t i0 = (int64_t)blockIdx.x * kNormThreads + threadIdx.x;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int64_t base = i0; base < n4; base += stride * kNormLoads) {
    // every load is issued (a lane past the end re-reads vector 0, which exists: base < n4) and the
    // bound selects the square afterwards: a load under a branch would be awaited before the next is
    // issued, and the loop would run at one load in flight
    f32x4 v[kNormLoads];
    bool in[kNormLoads];
#pragma unroll
    for (int u = 0; u < kNormLoads; ++u) {
      const int64_t i = base + u * stride;
      in[u] = i < n4;
      v[u] = norm_load4<BF>(x, in[u] ? i : 0);
    }
#pragma unroll
    for (int u = 0; u < kNormLoads; ++u) {
      const f32x4 sq = v[u] * v[u];
      acc += in[u] ? sq : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  for (int64_t i = (n4 << 2) + i0; i < n; i += stride) {
    const float e = norm_load1<BF>(x, i);
    sum += e * e;
  }
  sum = wave_sum(sum);
  __shared__ float wsum[kNormThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(kNormThreads) void grad_norm_finish_kernel(const float* __restrict__ partials, int nb,
                                                                        float grad_scale, float clip_norm,
                                                                        float* __restrict__ out) {
  __shared__ double acc[kNormThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += kNormThreads) s += (double)partials[i];
  acc[threadIdx.x] = s;
  __syncthreads();
  for (int o = kNormThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)((double)grad_scale * sqrt(acc[0]));
    out[0] = norm;
    out[1] = clip_norm / (norm > clip_norm ? norm : clip_norm);
  }
}

}  // namespace

int grad_norm_blocks(int64_t n) {
  const int64_t per_block = (int64_t)kNormThreads * kNormLoads * 4;
  const int64_t b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > kGradNormMaxBlocks ? kGradNormMaxBlocks : b));
}

void grad_sumsq(const float* g, const uint16_t* gbf, int64_t n, float* partials, hipStream_t s) {
  const int nb = grad_norm_blocks(n);
  if (gbf) {
    const int64_t n4 = (reinterpret_cast<uintptr_t>(gbf) & 7) == 0 ? n >> 2 : 0;
    grad_sumsq_kernel<true><<<nb, kNormThreads, 0, s>>>(gbf, n4, n, partials);
  } else {
    const int64_t n4 = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? n >> 2 : 0;
    grad_sumsq_kernel<false><<<nb, kNormThreads, 0, s>>>(g, n4, n, partials);
  }
}

void grad_norm_finish(const float* partials, int nb, float grad_scale, float clip_norm, float* out, hipStream_t s) {
  grad_norm_finish_kernel<<<1, kNormThreads, 0, s>>>(partials, nb, grad_scale, clip_norm, out);
}

}  // namespace tfd
