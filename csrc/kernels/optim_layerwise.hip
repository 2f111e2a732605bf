// Layer-wise optimizers over the flat buffer: LAMB and LARS, whose update of each variable is scaled
// by a trust ratio formed from two L2 norms over that variable (csrc/layerwise.h holds the
// definitions and the rounding bounds, csrc/layerwise_kernels.h the stages). A code object of its own:
// the flat Adam / momentum kernels (optim*.hip) stay what they were.
//
// All three stages run over the block table of layerwise.h: block b owns `count` <= kLwChunk elements
// from `first` (a multiple of 4) of ONE variable. A lane owns the float4 vectors threadIdx.x + u * 256,
// u < 4, of its block, and lanes 0..2 the block's scalar tail (count % 4, a variable's last block only).
// Every load of a stage is issued before its first use -- a lane past the end re-reads vector 0 of
// the block, which exists when the block has any vector, and the bound selects afterwards: a load
// under a branch would be awaited before the next is issued. The gradient is fp32 or the bf16 wire: the
// kernels test a.gbf ONCE, around their whole body (a template over the wire format, as
// grad_sumsq_kernel is; stage 3 does the same with the EMA pointer), so no body has a test among its
// loads, and the bf16 body keeps the raw bits until every load is issued (LwGrad). In the gfx950 ISA
// each body issues its 8 / 16 vector loads back to back. The scalars a stage depends on (the step
// counter, the clip factor, the variable's flags and its ratio) are loaded after the operands.
//
// The sums are deterministic: a fixed lane order, the wave_sum butterfly, the four waves through LDS
// in a fixed order, one plain store per block and sum; no atomics, nothing to zero beforehand.
#include <math.h>

#include <stdexcept>

#include "../common.h"
#include "../launch_check.h"
#include "../layerwise_kernels.h"
#include "../optim_const.h"  // EmaRef and the shadow's load / store / scalar update

namespace tfd {
namespace {

constexpr int kLwThreads = 256;
constexpr int kLwLoads = 4;
static_assert(kLwChunk == kLwThreads * kLwLoads * 4, "a block's chunk is one batch of loads per lane");

enum LwMode : int { LW_LAMB = 0, LW_LARS = 1, LW_NORMS = 2 };

// A gradient vector as loaded -- fp32, or the bf16 wire's raw bits -- and as fp32. The loads of a batch
// keep the raw form; the conversion comes after every load of the stage has been issued.
template <bool BF>
struct LwGrad {
  typedef f32x4 raw4;
  typedef float raw1;
  static __device__ __forceinline__ raw4 load4(const LayerwiseArgs& a, int64_t i) { return reinterpret_cast<const f32x4*>(a.g)[i]; }
  static __device__ __forceinline__ raw1 load1(const LayerwiseArgs& a, int64_t e) { return a.g[e]; }
  static __device__ __forceinline__ f32x4 f32(const raw4& r) { return r; }
  static __device__ __forceinline__ float f32(raw1 r) { return r; }
};
template <>
struct LwGrad<true> {
  typedef uint2 raw4;
  typedef uint16_t raw1;
  static __device__ __forceinline__ raw4 load4(const LayerwiseArgs& a, int64_t i) { return reinterpret_cast<const uint2*>(a.gbf)[i]; }
  static __device__ __forceinline__ raw1 load1(const LayerwiseArgs& a, int64_t e) { return a.gbf[e]; }
  static __device__ __forceinline__ f32x4 f32(const raw4& r) {
    return f32x4{bf2f((uint16_t)(r.x & 0xFFFF)), bf2f((uint16_t)(r.x >> 16)), bf2f((uint16_t)(r.y & 0xFFFF)),
                 bf2f((uint16_t)(r.y >> 16))};
  }
  static __device__ __forceinline__ float f32(raw1 r) { return bf2f(r); }
};
__device__ __forceinline__ f32x4 lw_ld4(const float* x, int64_t i) { return reinterpret_cast<const f32x4*>(x)[i]; }
__device__ __forceinline__ void lw_st4(float* x, int64_t i, const f32x4& v) { reinterpret_cast<f32x4*>(x)[i] = v; }
__device__ __forceinline__ float lw_hsum(const f32x4& v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// the block's two sums -> partials[block][0..1]
__device__ __forceinline__ void lw_store_partials(float s0, float s1, float* __restrict__ partials) {
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  __shared__ float w[2][kLwThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    w[0][threadIdx.x / kWave] = s0;
    w[1][threadIdx.x / kWave] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = (w[0][0] + w[0][1]) + (w[0][2] + w[0][3]);
    partials[2 * (int64_t)blockIdx.x + 1] = (w[1][0] + w[1][1]) + (w[1][2] + w[1][3]);
  }
}

// GUARD (LAMB only, the one stage 1 that stores): the non-finite guard's ok is loaded with the other
// scalars, and with ok == 0 neither m' nor v' is stored. The partials are stored either way -- every
// entry by every launch -- so stage 2 runs on whatever they hold and its output is unspecified on a
// skipped step.
template <int MODE, bool BF, bool GUARD>
__device__ __forceinline__ void lw_stage1_body(const LayerwiseArgs& a) {
  const LwBlock b = a.blocks[blockIdx.x];
  const int64_t v0 = b.first >> 2;
  const int n4 = b.count >> 2;
  const bool has_tail = (int)threadIdx.x < (b.count & 3);
  const int64_t te = b.first + ((int64_t)n4 << 2) + threadIdx.x;
  typedef LwGrad<BF> G;
  f32x4 pv[kLwLoads] = {}, mv[kLwLoads] = {}, vv[kLwLoads] = {};
  typename G::raw4 gv[kLwLoads] = {};
  bool in[kLwLoads] = {};
  float tp = 0.f, tm = 0.f, tv = 0.f;
  typename G::raw1 tg = 0;
  if (n4 > 0) {  // block-uniform
#pragma unroll
    for (int u = 0; u < kLwLoads; ++u) {
      const int item = (int)threadIdx.x + u * kLwThreads;
      in[u] = item < n4;
      const int64_t i = v0 + (in[u] ? item : 0);
      if (MODE != LW_NORMS) pv[u] = lw_ld4(a.p, i);
      if (MODE == LW_LAMB) {
        mv[u] = lw_ld4(a.s1, i);
        vv[u] = lw_ld4(a.s2, i);
      }
      gv[u] = G::load4(a, i);
    }
  }
  if (has_tail) {
    if (MODE != LW_NORMS) tp = a.p[te];
    if (MODE == LW_LAMB) {
      tm = a.s1[te];
      tv = a.s2[te];
    }
    tg = G::load1(a, te);
  }
  float mul = 1.f, ct = 0.f, lambda = 0.f;
  if (MODE != LW_NORMS) mul = a.grad_scale * *a.gscale;
  bool store = true;  // wave-uniform
  if (GUARD) store = *a.ok != 0.f;
  if (MODE == LW_LAMB) {
    const int64_t t = (a.step ? *a.step : 0) + a.t_offset;
    ct = lamb_ct(a.beta1, a.beta2, t);
    lambda = (a.segs[b.seg].flags & LW_DECAY) ? a.weight_decay : 0.f;
  }
  const float c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc0 = zero, acc1 = zero;
#pragma unroll
  for (int u = 0; u < kLwLoads; ++u) {
    const f32x4 g = G::f32(gv[u]) * mul;
    f32x4 second = g;
    if (MODE == LW_LAMB) {
      f32x4 m, v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        m[j] = lamb_m(mv[u][j], g[j], c1);
        v[j] = lamb_v(vv[u][j], g[j], c2);
        second[j] = lamb_u(pv[u][j], m[j], v[j], ct, a.eps, lambda);
      }
      if (store && in[u]) {
        const int64_t i = v0 + (int)threadIdx.x + u * kLwThreads;
        lw_st4(a.s1, i, m);
        lw_st4(a.s2, i, v);
      }
    }
    const f32x4 first = MODE == LW_NORMS ? g : pv[u];
    acc0 += in[u] ? first * first : zero;
    acc1 += in[u] ? second * second : zero;
  }
  float s0 = lw_hsum(acc0), s1 = lw_hsum(acc1);
  if (has_tail) {
    const float g = G::f32(tg) * mul;
    float second = g;
    if (MODE == LW_LAMB) {
      const float m = lamb_m(tm, g, c1), v = lamb_v(tv, g, c2);
      if (store) {
        a.s1[te] = m;
        a.s2[te] = v;
      }
      second = lamb_u(tp, m, v, ct, a.eps, lambda);
    }
    const float first = MODE == LW_NORMS ? g : tp;
    s0 += first * first;
    s1 += second * second;
  }
  lw_store_partials(s0, s1, a.partials);
}
template <int MODE>
__global__ __launch_bounds__(kLwThreads) void lw_stage1_kernel(LayerwiseArgs a) {
  if constexpr (MODE == LW_LAMB) {
    if (a.ok) {
      if (a.gbf) lw_stage1_body<MODE, true, true>(a);
      else lw_stage1_body<MODE, false, true>(a);
      return;
    }
  }
  if (a.gbf) lw_stage1_body<MODE, true, false>(a);
  else lw_stage1_body<MODE, false, false>(a);
}

// one block per variable: its blocks' partials in fp64, in a fixed order (a lane takes every 256th
// block in block order, then a tree over the lanes), then the ratio function
template <int MODE>
__global__ __launch_bounds__(kLwThreads) void lw_stage2_kernel(LayerwiseArgs a) {
  const LwSegBlocks sb = a.segs[blockIdx.x];
  __shared__ double acc[2][kLwThreads];
  double s0 = 0.0, s1 = 0.0;
  for (int i = threadIdx.x; i < sb.nblocks; i += kLwThreads) {
    s0 += (double)a.partials[2 * (int64_t)(sb.block0 + i)];
    s1 += (double)a.partials[2 * (int64_t)(sb.block0 + i) + 1];
  }
  acc[0][threadIdx.x] = s0;
  acc[1][threadIdx.x] = s1;
  __syncthreads();
  for (int o = kLwThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      acc[0][threadIdx.x] += acc[0][threadIdx.x + o];
      acc[1][threadIdx.x] += acc[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float* o = a.out + 3 * (int64_t)blockIdx.x;
    o[0] = lw_norm(acc[0][0]);
    o[1] = lw_norm(acc[1][0]);
    if (MODE == LW_LAMB) o[2] = lamb_ratio(acc[0][0], acc[1][0], sb.flags);
    else if (MODE == LW_LARS) o[2] = lars_ratio(acc[0][0], acc[1][0], a.eeta, a.weight_decay, a.eps, sb.flags);
    else o[2] = 1.f;
  }
}

// GUARD: the non-finite guard's ok is loaded with the ratio and t, after the operands, and with
// ok == 0 the block returns before its first store: p, accum, the bf16 shadow and the EMA shadow keep
// their bits
template <int MODE, bool BF, bool EMA, bool GUARD>  // LW_LAMB or LW_LARS
__device__ __forceinline__ void lw_stage3_body(const LayerwiseArgs& a) {
  const LwBlock b = a.blocks[blockIdx.x];
  const int64_t v0 = b.first >> 2;
  const int n4 = b.count >> 2;
  const bool has_tail = (int)threadIdx.x < (b.count & 3);
  const int64_t te = b.first + ((int64_t)n4 << 2) + threadIdx.x;
  const EmaRef em{a.ema, a.ema_decay, a.ema_num_updates};
  typedef LwGrad<BF> G;  // LAMB (always BF = false) keeps v' in the gradient's place
  // x1: LAMB m', LARS accum;  x2: LAMB v', LARS g as loaded
  f32x4 pv[kLwLoads] = {}, x1[kLwLoads] = {}, ev[kLwLoads] = {};
  typename G::raw4 x2[kLwLoads] = {};
  bool in[kLwLoads] = {};
  float tp = 0.f, t1 = 0.f;
  typename G::raw1 t2 = 0;
  if (n4 > 0) {
#pragma unroll
    for (int u = 0; u < kLwLoads; ++u) {
      const int item = (int)threadIdx.x + u * kLwThreads;
      in[u] = item < n4;
      const int64_t i = v0 + (in[u] ? item : 0);
      pv[u] = lw_ld4(a.p, i);
      x1[u] = lw_ld4(a.s1, i);
      if constexpr (MODE == LW_LAMB) x2[u] = lw_ld4(a.s2, i);
      else x2[u] = G::load4(a, i);
      if (EMA) ev[u] = ema_load4(em, i);
    }
  }
  if (has_tail) {
    tp = a.p[te];
    t1 = a.s1[te];
    if constexpr (MODE == LW_LAMB) t2 = a.s2[te];
    else t2 = G::load1(a, te);
  }
  // the ratio, t and the flags: loaded after the operands, awaited here
  const float r = a.out[3 * (int64_t)b.seg + 2];
  const int64_t t = (a.step ? *a.step : 0) + a.t_offset;
  if (GUARD) {
    if (*a.ok == 0.f) return;  // wave-uniform
  }
  const float lambda = (a.segs[b.seg].flags & LW_DECAY) ? a.weight_decay : 0.f;
  const float lr_r = lr_at(a.sched, t - 1) * r;
  const float omd = ema_omd_at(a.ema_decay, a.ema_num_updates, t);
  float ct = 0.f, mul = 1.f;
  if (MODE == LW_LAMB) ct = lamb_ct(a.beta1, a.beta2, t);
  else mul = a.grad_scale * *a.gscale;
#pragma unroll
  for (int u = 0; u < kLwLoads; ++u) {
    f32x4 p, acc;
    const f32x4 y = G::f32(x2[u]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (MODE == LW_LAMB) {
        p[j] = lamb_step(pv[u][j], lamb_u(pv[u][j], x1[u][j], y[j], ct, a.eps, lambda), lr_r);
      } else {
        acc[j] = lars_accum(x1[u][j], pv[u][j], y[j] * mul, a.momentum, lr_r, lambda);
        p[j] = pv[u][j] - acc[j];
      }
    }
    if (in[u]) {
      const int64_t i = v0 + (int)threadIdx.x + u * kLwThreads;
      lw_st4(a.p, i, p);
      if (MODE == LW_LARS) lw_st4(a.s1, i, acc);
      if (a.pbf) reinterpret_cast<uint2*>(a.pbf)[i] = make_uint2(pack_bf2(p[0], p[1]), pack_bf2(p[2], p[3]));
      if (EMA) ema_store4(em, i, ev[u], omd, p);
    }
  }
  if (has_tail) {
    float p;
    if (MODE == LW_LAMB) {
      p = lamb_step(tp, lamb_u(tp, t1, G::f32(t2), ct, a.eps, lambda), lr_r);
    } else {
      const float acc = lars_accum(t1, tp, G::f32(t2) * mul, a.momentum, lr_r, lambda);
      a.s1[te] = acc;
      p = tp - acc;
    }
    a.p[te] = p;
    if (a.pbf) a.pbf[te] = f2bf_bits(p);
    if (EMA) ema_update1(em, te, omd, p);
  }
}

// the wire format, the EMA shadow and the guard are tested once, around the whole body
template <int MODE, bool GUARD>
__device__ __forceinline__ void lw_stage3_pick(const LayerwiseArgs& a) {
  if constexpr (MODE == LW_LARS) {  // LAMB's stage 3 does not read the gradient
    if (a.gbf) {
      if (a.ema) lw_stage3_body<MODE, true, true, GUARD>(a);
      else lw_stage3_body<MODE, true, false, GUARD>(a);
      return;
    }
  }
  if (a.ema) lw_stage3_body<MODE, false, true, GUARD>(a);
  else lw_stage3_body<MODE, false, false, GUARD>(a);
}
template <int MODE>
__global__ __launch_bounds__(kLwThreads) void lw_stage3_kernel(LayerwiseArgs a) {
  if (a.ok) lw_stage3_pick<MODE, true>(a);
  else lw_stage3_pick<MODE, false>(a);
}

void lw_check(const LayerwiseArgs& a, const char* who, bool update) {
  auto need = [&](bool ok, const char* what) {
    if (!ok) throw std::runtime_error(std::string(who) + ": " + what);
  };
  need(a.blocks && a.segs && a.nblocks >= 1 && a.nsegs >= 1, "an empty block table");
  need(a.partials && a.out, "no partials / output buffer");
  need((a.g != nullptr) != (a.gbf != nullptr), "exactly one of g and gbf");
  need(((reinterpret_cast<uintptr_t>(a.g) & 15) | (reinterpret_cast<uintptr_t>(a.gbf) & 7)) == 0, "unaligned gradient");
  if (!update) return;
  need(a.p && a.s1 && a.gscale, "p, the first slot and gscale are required");
  need(((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.s1) | reinterpret_cast<uintptr_t>(a.s2) |
         reinterpret_cast<uintptr_t>(a.ema)) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.pbf) & 7) == 0,
       "unaligned buffer (16 bytes for fp32, 8 for bf16)");
}

template <int MODE>
void lw_apply(const LayerwiseArgs& a, hipStream_t s) {
  TFD_LAUNCH(lw_stage1_kernel<MODE><<<a.nblocks, kLwThreads, 0, s>>>(a));
  TFD_LAUNCH(lw_stage2_kernel<MODE><<<a.nsegs, kLwThreads, 0, s>>>(a));
  if (MODE != LW_NORMS) TFD_LAUNCH(lw_stage3_kernel<MODE == LW_NORMS ? LW_LARS : MODE><<<a.nblocks, kLwThreads, 0, s>>>(a));
}

}  // namespace

void lamb_apply(const LayerwiseArgs& a, hipStream_t s) {
  lw_check(a, "lamb_apply", true);
  if (!a.s2) throw std::runtime_error("lamb_apply: the v slot is required");
  lw_apply<LW_LAMB>(a, s);
}
void lars_apply(const LayerwiseArgs& a, hipStream_t s) {
  lw_check(a, "lars_apply", true);
  lw_apply<LW_LARS>(a, s);
}
void layer_norms_apply(const LayerwiseArgs& a, hipStream_t s) {
  lw_check(a, "layer_norms_apply", false);
  lw_apply<LW_NORMS>(a, s);
}

}  // namespace tfd
