// Multi-tensor (flat-buffer) optimizer kernels: one launch updates every parameter of the model.
// ApplyAdam semantics follow TF1 (training_ops ApplyAdam, reached from
// /root/reference/mnist_python_m.py:208,222 and mnist_single.py:95):
//   m_t = m + (g - m)(1 - b1);  v_t = v + (g^2 - v)(1 - b2)
//   p  -= lr * sqrt(1 - b2^t) / (1 - b1^t) * m_t / (sqrt(v_t) + eps),   t = global_step + 1
// The fp32 master is updated in place and its bf16 shadow (the operand every MFMA kernel reads)
// is rewritten in the same pass. t comes from the device global_step (read-only here: the step's
// last conv-grad reduce kernel bumps it), so a captured step graph needs no host round trip and
// the optimizer needs no cross-block arrival counter (a 2048-way fan-in on one word).
#include <math.h>

#include <stdexcept>
#include "../common.h"
#include "../tfd_kernels.h"
#include "../optim_kernels.h"

namespace tfd {
namespace {

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = f2bf_bits(x[i]);
}
__global__ void cast_bf16_f32_kernel(const uint16_t* __restrict__ x, float* __restrict__ y, int64_t n, float sc) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = bf2f(x[i]) * sc;
}
__global__ void scale_kernel(float* __restrict__ x, int64_t n, float sc) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= sc;
}
__global__ void axpy_kernel(float* __restrict__ d, const float* __restrict__ s, int64_t n, float alpha) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] += alpha * s[i];
}

// plain fp32 copy, float4 per lane when both ends are 16-B aligned (IPC peer buffers of the GPU
// parameter server, csrc/runtime/gpu_ps.cpp)
__global__ void copy_f32_kernel(float* __restrict__ d, const float* __restrict__ s, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool v4 = ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0;
  const int64_t n4 = v4 ? n >> 2 : 0;
  for (int64_t i = i0; i < n4; i += stride) reinterpret_cast<f32x4*>(d)[i] = reinterpret_cast<const f32x4*>(s)[i];
  for (int64_t i = (n4 << 2) + i0; i < n; i += stride) d[i] = s[i];
}

// ---- roofline probes (tools/debug/roofline_probe.py) ----
// The optimizer's byte floor: the same traffic as ApplyAdam over a flat buffer -- fp32 p, m, v read
// and written in place, a bf16 gradient read, the bf16 shadow written (28 B per parameter) -- plus
// an optional extra fp32 read stream (the conv weight-gradient slabs the one-GPU tail also reads),
// with no math beyond adds. U float4 per lane in flight (grid-stride by U strides).
template <int U>
__global__ __launch_bounds__(kOptThreads) void stream_floor_kernel(float* __restrict__ p, float* __restrict__ m,
                                                                   float* __restrict__ v, const uint16_t* __restrict__ g,
                                                                   uint16_t* __restrict__ pbf, const float* __restrict__ x,
                                                                   int64_t n4, int64_t nx4) {
  const int64_t stride = (int64_t)gridDim.x * kOptThreads;
  for (int64_t base = (int64_t)blockIdx.x * kOptThreads + threadIdx.x; base < n4; base += stride * U) {
    f32x4 pp[U], mm[U], vv[U];
    uint2 gg[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * stride;
      if (i < n4) {
        pp[u] = reinterpret_cast<const f32x4*>(p)[i];
        mm[u] = reinterpret_cast<const f32x4*>(m)[i];
        vv[u] = reinterpret_cast<const f32x4*>(v)[i];
        gg[u] = reinterpret_cast<const uint2*>(g)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * stride;
      if (i < n4) {
        const float gs = __uint_as_float(gg[u].x << 16);
        f32x4 q = pp[u] + gs;
        if (i < nx4) q += reinterpret_cast<const f32x4*>(x)[i];
        reinterpret_cast<f32x4*>(p)[i] = q;
        reinterpret_cast<f32x4*>(m)[i] = mm[u] + gs;
        reinterpret_cast<f32x4*>(v)[i] = vv[u] + gs;
        reinterpret_cast<uint2*>(pbf)[i] = make_uint2(pack_bf2(q[0], q[1]), pack_bf2(q[2], q[3]));
      }
    }
  }
}
// an empty kernel: the dependent-launch boundary floor of a chain of launches
__global__ void noop_kernel() {}

}  // namespace

void adam_apply(const AdamArgs& a, hipStream_t s) {
  // a constant rate launches this file's instantiations (the kernels as they were before schedules);
  // the ones that carry a schedule live in their own code object (optim_sched.hip)
  if (a.sched.kind == LR_CONSTANT) adam_kernel<<<blocks_for(a.n, 4), kOptThreads, 0, s>>>(adam_const(a));
  else adam_apply_sched(a, s);
}
void adam_apply_ranges(const AdamArgs& a, int nr, const int64_t* beg, const int64_t* n, hipStream_t s) {
  int nb = 0;
  const AdamRanges r = make_adam_ranges("adam_apply_ranges", nr, beg, n, &nb);
  if (a.sched.kind == LR_CONSTANT) adam_ranges_kernel<<<nb, kOptThreads, 0, s>>>(adam_const(a), r);
  else adam_ranges_sched(a, r, nb, s);
}
void stream_floor(float* p, float* m, float* v, const uint16_t* g, uint16_t* pbf, const float* x, int64_t n4, int64_t nx4,
                  int blocks, int unroll, hipStream_t s) {
  if (blocks < 1) throw std::runtime_error("stream_floor: blocks >= 1");
  if (unroll == 1) stream_floor_kernel<1><<<blocks, kOptThreads, 0, s>>>(p, m, v, g, pbf, x, n4, nx4);
  else if (unroll == 2) stream_floor_kernel<2><<<blocks, kOptThreads, 0, s>>>(p, m, v, g, pbf, x, n4, nx4);
  else if (unroll == 4) stream_floor_kernel<4><<<blocks, kOptThreads, 0, s>>>(p, m, v, g, pbf, x, n4, nx4);
  else throw std::runtime_error("stream_floor: unroll 1, 2 or 4");
}
void noop_launch(int blocks, hipStream_t s) { noop_kernel<<<blocks < 1 ? 1 : blocks, 64, 0, s>>>(); }
void sgd_apply(const SgdArgs& a, hipStream_t s) {
  if (a.sched.kind == LR_CONSTANT) sgd_kernel<<<blocks_for(a.n, 1), kOptThreads, 0, s>>>(sgd_const(a));
  else sgd_apply_sched(a, s);
}
void cast_f32_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t s) {
  cast_f32_bf16_kernel<<<blocks_for(n, 1), kOptThreads, 0, s>>>(x, y, n);
}
void cast_bf16_f32(const uint16_t* x, float* y, int64_t n, float scale, hipStream_t s) {
  cast_bf16_f32_kernel<<<blocks_for(n, 1), kOptThreads, 0, s>>>(x, y, n, scale);
}
void copy_f32(float* dst, const float* src, int64_t n, hipStream_t s) {
  if (n > 0) copy_f32_kernel<<<blocks_for(n, 4), kOptThreads, 0, s>>>(dst, src, n);
}
void scale_f32(float* x, int64_t n, float scale, hipStream_t s) {
  scale_kernel<<<blocks_for(n, 1), kOptThreads, 0, s>>>(x, n, scale);
}
void vec_accumulate(float* dst, const float* src, int64_t n, float alpha, hipStream_t s) {
  axpy_kernel<<<blocks_for(n, 1), kOptThreads, 0, s>>>(dst, src, n, alpha);
}

}  // namespace tfd
