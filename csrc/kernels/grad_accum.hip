// Gradient accumulation over micro-batches (csrc/grad_accum.h): acc = g, acc += g, or out = acc + g, a
// flat streaming kernel in the shape of the flat optimizer kernels -- 256-thread grid-stride blocks,
// 16-byte accesses, every load of a lane's batch issued before its first store, default cache policy
// (the buffers are re-read by the next kernel: docs/DESIGN.md section 1 measured non-temporal
// accesses slower there). One plain fp32 add per element, no atomics: bit-identical run to run.
//   head / body / tail: the body is n4 vectors of 4 elements starting at element `head`, where every
//   pointer in use is 16-byte (fp32) or 8-byte (bf16) aligned; the elements [0, head) and
//   [head + 4 * n4, n) go one by one. Pointers that do not share one phase (element index mod 4) have
//   no such body: n4 = 0 and everything goes one by one.
#include "../common.h"
#include "../grad_accum.h"
#include "../launch_check.h"

namespace tfd {
namespace {

constexpr int kAccThreads = 256;
// Grid and loads in flight, from the A/B of profiles/grad_accum_step.log (add mode, M.TOTAL elements, the
// buffers cache-resident as they are in the step: the gradient was written by the kernels just before):
// 1 stride per lane 4.75 - 4.86 us at every grid from 512 to 4096 blocks, 2 strides 4.99 - 5.17, 4 strides
// 5.10 - 6.33 (the worst at 4096 blocks). More loads in flight buy nothing at this occupancy.
constexpr int kAccMaxBlocks = 1024;  // 4 blocks of 256 threads per CU; the rest is grid-stride
constexpr int kAccLoads = 1;         // strides per lane in flight

template <bool BF>
__device__ __forceinline__ f32x4 acc_load4(const void* x, int64_t i) {
  if constexpr (BF) {
    const uint2 gb = reinterpret_cast<const uint2*>(x)[i];
    return f32x4{bf2f((uint16_t)(gb.x & 0xFFFF)), bf2f((uint16_t)(gb.x >> 16)), bf2f((uint16_t)(gb.y & 0xFFFF)),
                 bf2f((uint16_t)(gb.y >> 16))};
  } else {
    return reinterpret_cast<const f32x4*>(x)[i];
  }
}
template <bool BF>
__device__ __forceinline__ float acc_load1(const void* x, int64_t i) {
  if constexpr (BF) return bf2f(reinterpret_cast<const uint16_t*>(x)[i]);
  else return reinterpret_cast<const float*>(x)[i];
}
template <bool BF>
__device__ __forceinline__ void acc_store4(void* y, int64_t i, f32x4 v) {
  if constexpr (BF) reinterpret_cast<uint2*>(y)[i] = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
  else reinterpret_cast<f32x4*>(y)[i] = v;
}
template <bool BF>
__device__ __forceinline__ void acc_store1(void* y, int64_t i, float v) {
  if constexpr (BF) reinterpret_cast<uint16_t*>(y)[i] = f2bf_bits(v);
  else reinterpret_cast<float*>(y)[i] = v;
}

// g / acc / dst: the bases (element 0). dst is acc itself but in GA_EMIT. No __restrict__: GA_ADD reads
// and writes acc, and GA_EMIT's dst may be g (the engine emits into the buffer the last micro-batch's
// gradient is in); a lane writes only the elements it has loaded.
template <int MODE, bool GBF, bool OBF, int U>
__global__ __launch_bounds__(kAccThreads) void grad_accum_kernel(const void* g, const float* acc, void* dst, int64_t head,
                                                                 int64_t n4, int64_t n, int64_t* bump) {
  const int64_t stride = (int64_t)gridDim.x * kAccThreads;
  const int64_t i0 = (int64_t)blockIdx.x * kAccThreads + threadIdx.x;
  const void* gv = GBF ? (const void*)((const uint16_t*)g + head) : (const void*)((const float*)g + head);
  const float* av = acc + head;
  void* dv = OBF ? (void*)((uint16_t*)dst + head) : (void*)((float*)dst + head);
  for (int64_t base = i0; base < n4; base += stride * U) {
    // every load is issued (a lane past the end re-reads vector 0, which exists: base < n4) before
    // the first store; the bound selects the stores
    f32x4 x[U], a[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * stride;
      in[u] = i < n4;
      x[u] = acc_load4<GBF>(gv, in[u] ? i : 0);
      if constexpr (MODE != GA_STORE) a[u] = acc_load4<false>(av, in[u] ? i : 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * stride;
      f32x4 r = x[u];
      if constexpr (MODE != GA_STORE) r = a[u] + x[u];
      if (in[u]) acc_store4<OBF>(dv, i, r);
    }
  }
  // scalar head [0, head) and tail [head + 4 * n4, n)
  const int64_t ns = n - (n4 << 2);
  for (int64_t j = i0; j < ns; j += stride) {
    const int64_t i = j < head ? j : j + (n4 << 2);
    float r = acc_load1<GBF>(g, i);
    if constexpr (MODE != GA_STORE) r = acc[i] + r;
    acc_store1<OBF>(dst, i, r);
  }
  if constexpr (MODE == GA_EMIT) {
    if (bump && i0 == 0) *bump += 1;
  }
}

// element index mod 4 of a pointer to elements of `elem` bytes
int phase(const void* p, int elem) { return (int)((reinterpret_cast<uintptr_t>(p) / (uintptr_t)elem) & 3); }

template <int MODE, bool GBF, bool OBF>
void launch(const void* g, const float* acc, void* dst, int64_t head, int64_t n4, int64_t n, int64_t* bump, int blocks,
            int loads, hipStream_t s) {
  if (loads == 1) TFD_LAUNCH(grad_accum_kernel<MODE, GBF, OBF, 1><<<blocks, kAccThreads, 0, s>>>(g, acc, dst, head, n4, n, bump));
  else if (loads == 2) TFD_LAUNCH(grad_accum_kernel<MODE, GBF, OBF, 2><<<blocks, kAccThreads, 0, s>>>(g, acc, dst, head, n4, n, bump));
  else if (loads == 4) TFD_LAUNCH(grad_accum_kernel<MODE, GBF, OBF, 4><<<blocks, kAccThreads, 0, s>>>(g, acc, dst, head, n4, n, bump));
  else throw std::runtime_error("grad_accum: loads in flight must be 1, 2 or 4");
}

}  // namespace

void grad_accum(const GradAccumArgs& a, hipStream_t s, int blocks, int loads) {
  if (a.n < 1 || !a.acc || (!a.g && !a.gbf)) throw std::runtime_error("grad_accum: n >= 1, acc and g");
  if (a.mode < GA_STORE || a.mode > GA_EMIT) throw std::runtime_error("grad_accum: mode");
  const bool emit = a.mode == GA_EMIT;
  if (emit != (a.out || a.outbf)) throw std::runtime_error("grad_accum: out goes with GA_EMIT and only with it");
  const bool gbf = a.gbf != nullptr, obf = emit && a.outbf != nullptr;
  const void* g = gbf ? (const void*)a.gbf : (const void*)a.g;
  void* dst = emit ? (obf ? (void*)a.outbf : (void*)a.out) : (void*)a.acc;
  const int ph = phase(g, gbf ? 2 : 4);
  const bool same = ph == phase(a.acc, 4) && (!emit || ph == phase(dst, obf ? 2 : 4));
  int64_t head = 0, n4 = 0;
  if (same) {
    head = (4 - ph) & 3;
    if (head > a.n) head = a.n;
    n4 = (a.n - head) >> 2;
  }
  if (loads == 0) loads = kAccLoads;
  if (blocks == 0) {
    const int64_t per_block = (int64_t)kAccThreads * loads;
    const int64_t b = (n4 + per_block - 1) / per_block;
    blocks = (int)(b < 1 ? 1 : (b > kAccMaxBlocks ? kAccMaxBlocks : b));
  }
  if (blocks < 1 || blocks > 65536) throw std::runtime_error("grad_accum: blocks");
  int64_t* bump = emit ? a.bump : nullptr;
  if (a.mode == GA_STORE) {
    if (gbf) launch<GA_STORE, true, false>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
    else launch<GA_STORE, false, false>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
  } else if (a.mode == GA_ADD) {
    if (gbf) launch<GA_ADD, true, false>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
    else launch<GA_ADD, false, false>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
  } else if (gbf) {
    if (obf) launch<GA_EMIT, true, true>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
    else launch<GA_EMIT, true, false>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
  } else {
    if (obf) launch<GA_EMIT, false, true>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
    else launch<GA_EMIT, false, false>(g, a.acc, dst, head, n4, a.n, bump, blocks, loads, s);
  }
}

}  // namespace tfd
