// The flat optimizer kernels (ApplyAdam, the ZeRO-1 ranges form, GradientDescent / Momentum) as
// templates over their argument struct. Two .hip files instantiate them: optim.hip with the
// constant-rate views (optim_const.h: the default path, the kernels as they were before schedules)
// and optim_sched.hip with AdamArgs / SgdArgs (the LrSchedule evaluated from the device step counter
// where t is consumed). A third, optim_clip.hip, takes them over AdamClipArgs / SgdClipArgs: the same
// kernels with the gradient multiplier grad_scale * *gscale, the clip factor of global-norm clipping
// read from the device (grad_norm.hip). A fourth, optim_ema.hip, takes them over AdamEmaArgs /
// SgdEmaArgs: the clip variant plus the moving average of the weights, updated from p' while it is in
// registers (ema.h). A fifth, optim_guard.hip, takes them over GuardArgs<...> of the clip and the EMA
// wrappers: the same kernels, returning before their first store when the step's gradient is not finite
// (grad_guard.hip). Separate code objects on purpose: see mnist_tail.h.
#pragma once
#include <math.h>

#include <stdexcept>
#include <string>

#include "common.h"
#include "optim_const.h"
#include "tfd_kernels.h"

namespace tfd {
struct AdamRanges;
// the scheduled instantiations' launchers (optim_sched.hip)
void adam_apply_sched(const AdamArgs& a, hipStream_t s);
void adam_ranges_sched(const AdamArgs& a, const AdamRanges& r, int blocks, hipStream_t s);
void sgd_apply_sched(const SgdArgs& a, hipStream_t s);
}  // namespace tfd

namespace tfd {
namespace {

constexpr int kOptThreads = 256;
constexpr int kOptMaxBlocks = 2048;

struct AdamItem {
  f32x4 p, m, v, g;
};
template <class A>
__device__ __forceinline__ AdamItem adam_load4(const A& a, int64_t i) {
  AdamItem x;
  x.p = reinterpret_cast<const f32x4*>(a.p)[i];
  x.m = reinterpret_cast<const f32x4*>(a.m)[i];
  x.v = reinterpret_cast<const f32x4*>(a.v)[i];
  if (a.gbf) {
    const uint2 gb = reinterpret_cast<const uint2*>(a.gbf)[i];
    x.g = f32x4{bf2f((uint16_t)(gb.x & 0xFFFF)), bf2f((uint16_t)(gb.x >> 16)), bf2f((uint16_t)(gb.y & 0xFFFF)),
                bf2f((uint16_t)(gb.y >> 16))};
  } else {
    x.g = reinterpret_cast<const f32x4*>(a.g)[i];
  }
  return x;
}
// em / xe / omd: the moving average of the weights (optim_const.h), its float4 loaded beside x and
// its 1 - d_t -- empty tags unless K is an EMA wrapper
template <class A, class C, class E, class EV, class EO>
__device__ __forceinline__ void adam_apply4(const A& a, int64_t i, AdamItem x, C clip, float lr_t, float c1, float c2,
                                            const E& em, EV xe, EO omd) {
  const f32x4 g = x.g * grad_mul(a, clip);
  f32x4 p = x.p, m = x.m, v = x.v;
  m = m + (g - m) * c1;
  v = v + (g * g - v) * c2;
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] -= lr_t * m[j] / (sqrtf(v[j]) + a.eps);
  reinterpret_cast<f32x4*>(a.p)[i] = p;
  reinterpret_cast<f32x4*>(a.m)[i] = m;
  reinterpret_cast<f32x4*>(a.v)[i] = v;
  if (a.pbf) reinterpret_cast<uint2*>(a.pbf)[i] = make_uint2(pack_bf2(p[0], p[1]), pack_bf2(p[2], p[3]));
  ema_store4(em, i, xe, omd, p);
}
// The optimizer kernels are templates over their argument struct: the constant-rate view (AdamConst
// / SgdConst, optim_const.h: the default path, as it was before schedules) or the struct with the
// LrSchedule, evaluated from the step counter where t is consumed. The launchers pick by the kind.
// K is that struct or its clip wrapper: optim_args(k) is the struct, clip_load(k) the wrapper's device
// clip factor (nothing for the bare struct) and grad_mul(a, clip) the gradient's multiplier, grad_scale
// times the factor if there is one (optim_const.h).
template <class K>
__global__ __launch_bounds__(kOptThreads) void adam_kernel(K k) {
  const auto& a = optim_args(k);
  // the first item's operands are loaded before t (a dependent load of the step counter) is awaited
  const int64_t n4 = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kOptThreads;
  const int64_t i0 = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
  const auto em = ema_of(k);
  AdamItem x{};
  decltype(ema_load4(em, 0)) xe{};
  if (i0 < n4) {
    x = adam_load4(a, i0);
    xe = ema_load4(em, i0);
  }
  const int64_t t = (a.step ? *a.step : 0) + a.t_offset;
  const auto clip = clip_load(k);  // a load like t: issued here, awaited with it
  const auto ok = guard_load(k);   // likewise (optim_const.h); nothing unless K is a guard wrapper
  if (guard_skip(ok)) return;      // wave-uniform, before the first store: a skipped step writes nothing
  const auto omd = ema_omd(em, t);
  const float b1p = powf(a.beta1, (float)t), b2p = powf(a.beta2, (float)t);
  const float lr_t = base_lr(a, t) * sqrtf(1.f - b2p) / (1.f - b1p);
  const float c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
  for (int64_t i = i0; i < n4; i += stride) {
    if (i != i0) {
      x = adam_load4(a, i);
      xe = ema_load4(em, i);
    }
    adam_apply4(a, i, x, clip, lr_t, c1, c2, em, xe, omd);
  }
  // scalar tail (n % 4)
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * kOptThreads + threadIdx.x; i < a.n; i += stride) {
    const float g = (a.gbf ? bf2f(a.gbf[i]) : a.g[i]) * grad_mul(a, clip);
    float m = a.m[i] + (g - a.m[i]) * c1;
    float v = a.v[i] + (g * g - a.v[i]) * c2;
    const float p = a.p[i] - lr_t * m / (sqrtf(v) + a.eps);
    a.p[i] = p; a.m[i] = m; a.v[i] = v;
    if (a.pbf) a.pbf[i] = f2bf_bits(p);
    ema_update1(em, i, omd, p);
  }
}

}  // namespace
struct AdamRanges {
  int nr;
  int64_t beg4[3], pre4[4];  // range starts and prefix sums in float4 units
  int64_t tail_beg, tail_n;  // the last range's n % 4 scalar elements
};
namespace {
// same per-element math as adam_kernel, over a table of ranges (the logical float4 index is mapped
// to its range by the prefix sums)
template <class K>
__global__ __launch_bounds__(kOptThreads) void adam_ranges_kernel(K k, AdamRanges r) {
  const auto& a = optim_args(k);
  // the first item's operands are loaded before t (a dependent load of the step counter) is awaited:
  // for the small conv + output-layer launch of the DP step that is one memory round trip of its ~3
  const int64_t stride = (int64_t)gridDim.x * kOptThreads;
  auto phys = [&](int64_t i) {
    const int k = i < r.pre4[1] ? 0 : (r.nr > 2 && i >= r.pre4[2] ? 2 : 1);
    return r.beg4[k] + (i - r.pre4[k]);
  };
  int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x;
  const auto em = ema_of(k);
  AdamItem x{};
  decltype(ema_load4(em, 0)) xe{};
  if (i < r.pre4[r.nr]) {
    x = adam_load4(a, phys(i));
    xe = ema_load4(em, phys(i));
  }
  const int64_t t = (a.step ? *a.step : 0) + a.t_offset;
  const auto clip = clip_load(k);
  const auto ok = guard_load(k);
  if (guard_skip(ok)) return;
  const auto omd = ema_omd(em, t);
  const float b1p = powf(a.beta1, (float)t), b2p = powf(a.beta2, (float)t);
  const float lr_t = base_lr(a, t) * sqrtf(1.f - b2p) / (1.f - b1p);
  const float c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
  for (; i < r.pre4[r.nr]; i += stride) {
    const int64_t pi = phys(i);
    if (i != (int64_t)blockIdx.x * kOptThreads + threadIdx.x) {
      x = adam_load4(a, pi);
      xe = ema_load4(em, pi);
    }
    adam_apply4(a, pi, x, clip, lr_t, c1, c2, em, xe, omd);
  }
  if (blockIdx.x == 0 && threadIdx.x < r.tail_n) {
    const int64_t i = r.tail_beg + threadIdx.x;
    const float g = (a.gbf ? bf2f(a.gbf[i]) : a.g[i]) * grad_mul(a, clip);
    const float m = a.m[i] + (g - a.m[i]) * c1;
    const float v = a.v[i] + (g * g - a.v[i]) * c2;
    const float p = a.p[i] - lr_t * m / (sqrtf(v) + a.eps);
    a.p[i] = p; a.m[i] = m; a.v[i] = v;
    if (a.pbf) a.pbf[i] = f2bf_bits(p);
    ema_update1(em, i, omd, p);
  }
}

// the shadow's 1 - d_t of an SGD update: t = *step + t_offset, as the schedule reads it
template <class A>
__device__ __forceinline__ NoEma sgd_ema_omd(const A&, NoEma) { return NoEma{}; }
__device__ __forceinline__ float sgd_ema_omd(const SgdArgs& a, const EmaRef& em) {
  return ema_omd(em, (a.step ? *a.step : 0) + a.t_offset);
}
// GradientDescent / Momentum (TF ApplyMomentum: accum = accum*mu + g; p -= lr*accum,
// nesterov: p -= lr*(g + mu*accum)); optional decoupled-from-nothing L2 weight decay folded in g.
template <class K>  // SgdConst, SgdArgs, SgdClipArgs, SgdEmaArgs or a guard wrapper of the last two
__global__ __launch_bounds__(kOptThreads) void sgd_kernel(K k) {
  const auto& a = optim_args(k);
  const int64_t stride = (int64_t)gridDim.x * kOptThreads;
  const float lr = base_lr(a);
  const auto clip = clip_load(k);
  const auto ok = guard_load(k);
  if (guard_skip(ok)) return;
  const auto em = ema_of(k);
  const auto omd = sgd_ema_omd(a, em);
  for (int64_t i = (int64_t)blockIdx.x * kOptThreads + threadIdx.x; i < a.n; i += stride) {
    float g = (a.gbf ? bf2f(a.gbf[i]) : a.g[i]) * grad_mul(a, clip) + a.weight_decay * a.p[i];
    float p = a.p[i];
    if (a.mom) {
      const float acc = a.mom[i] * a.momentum + g;
      a.mom[i] = acc;
      p -= a.nesterov ? lr * (g + a.momentum * acc) : lr * acc;
    } else {
      p -= lr * g;
    }
    a.p[i] = p;
    if (a.pbf) a.pbf[i] = f2bf_bits(p);
    ema_update1(em, i, omd, p);
  }
}

inline int blocks_for(int64_t n, int per_thread) {
  const int64_t b = (n / per_thread + kOptThreads - 1) / kOptThreads;
  return (int)(b < 1 ? 1 : (b > kOptMaxBlocks ? kOptMaxBlocks : b));
}

// the range table of adam_ranges_kernel from element ranges [beg, beg + n); *blocks: its grid
inline AdamRanges make_adam_ranges(const char* who, int nr, const int64_t* beg, const int64_t* n, int* blocks) {
  if (nr < 1 || nr > 3) throw std::runtime_error(std::string(who) + ": 1..3 ranges");
  AdamRanges r{};
  r.nr = nr;
  r.pre4[0] = 0;
  for (int k = 0; k < nr; ++k) {
    if (beg[k] % 4 || (k < nr - 1 && n[k] % 4)) throw std::runtime_error(std::string(who) + ": unaligned range");
    r.beg4[k] = beg[k] / 4;
    r.pre4[k + 1] = r.pre4[k] + n[k] / 4;
  }
  r.tail_beg = beg[nr - 1] + n[nr - 1] / 4 * 4;
  r.tail_n = n[nr - 1] % 4;
  *blocks = blocks_for(r.pre4[nr] * 4, 4);
  return r;
}

}  // namespace
}  // namespace tfd
