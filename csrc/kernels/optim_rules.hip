// RMSProp (plain / centered, with and without momentum) and Adagrad over the flat buffer: one launch
// each, the shape of adam_kernel (optim_kernels.h) -- 256 threads, grid-stride over float4 items with
// the grid capped as blocks_for caps it, 16-byte loads and stores of p and the slots, uint2 reads of a
// bf16 gradient, the bf16 shadow written as packed uint2, an n % 4 scalar tail. csrc/optim_rules.h holds
// the definitions and the argument struct. A code object of its own: the flat Adam / momentum kernels
// (optim*.hip) and the fused MNIST tail stay what they were.
//
// The first item's operands are loaded before the step counter, the clip factor and the guard's ok are
// awaited; with the guard's ok == 0 the kernel returns before its first store (wave-uniform). The EMA
// shadow is updated from p' in registers (ema.h). The wire format and the shadow pointer are tested
// once, around the whole body, so no body has a test among its loads. No atomics, no LDS, no memset.
#include <math.h>

#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ema.h"
#include "../launch_check.h"
#include "../optim_rules.h"

namespace tfd {
namespace {

constexpr int kRuleThreads = 256;
constexpr int kRuleMaxBlocks = 2048;

enum Rule : int { RULE_RMSPROP = 0, RULE_ADAGRAD = 1 };

// one float4 item as loaded: the gradient keeps its wire form until the loads are issued
template <bool BF>
struct RuleGrad {
  typedef f32x4 raw4;
  static __device__ __forceinline__ raw4 load4(const RuleArgs& a, int64_t i) { return reinterpret_cast<const f32x4*>(a.g)[i]; }
  static __device__ __forceinline__ float load1(const RuleArgs& a, int64_t e) { return a.g[e]; }
  static __device__ __forceinline__ f32x4 f32(const raw4& r) { return r; }
};
template <>
struct RuleGrad<true> {
  typedef uint2 raw4;
  static __device__ __forceinline__ raw4 load4(const RuleArgs& a, int64_t i) { return reinterpret_cast<const uint2*>(a.gbf)[i]; }
  static __device__ __forceinline__ float load1(const RuleArgs& a, int64_t e) { return bf2f(a.gbf[e]); }
  static __device__ __forceinline__ f32x4 f32(const raw4& r) {
    return f32x4{bf2f((uint16_t)(r.x & 0xFFFF)), bf2f((uint16_t)(r.x >> 16)), bf2f((uint16_t)(r.y & 0xFFFF)),
                 bf2f((uint16_t)(r.y >> 16))};
  }
};
template <bool BF>
struct RuleItem {
  f32x4 p, s1, s2, s3, e;
  typename RuleGrad<BF>::raw4 g;
};
__device__ __forceinline__ f32x4 rule_ld4(const float* x, int64_t i) { return reinterpret_cast<const f32x4*>(x)[i]; }
__device__ __forceinline__ void rule_st4(float* x, int64_t i, const f32x4& v) { reinterpret_cast<f32x4*>(x)[i] = v; }

// the slots an instantiation reads: s1 always, s2 (mom) with momentum, s3 (mg) when centered
template <int RULE, bool CENTERED, bool MOM, bool BF, bool EMA>
__device__ __forceinline__ RuleItem<BF> rule_load4(const RuleArgs& a, int64_t i) {
  RuleItem<BF> x{};
  x.p = rule_ld4(a.p, i);
  x.s1 = rule_ld4(a.s1, i);
  if (RULE == RULE_RMSPROP && MOM) x.s2 = rule_ld4(a.s2, i);
  if (RULE == RULE_RMSPROP && CENTERED) x.s3 = rule_ld4(a.s3, i);
  x.g = RuleGrad<BF>::load4(a, i);
  if (EMA) x.e = rule_ld4(a.ema, i);
  return x;
}

// THE element update: new slots and p' from the old ones and g (already multiplied)
template <int RULE, bool CENTERED, bool MOM>
__device__ __forceinline__ void rule_update(const RuleArgs& a, float g, float lr, float c, float& p, float& s1, float& s2,
                                            float& s3) {
  if (RULE == RULE_ADAGRAD) {
    s1 = adagrad_accum(s1, g);
    p = p - rule_delta(g, lr, s1);
    return;
  }
  s1 = rms_ms(s1, g, c);
  float d;
  if (CENTERED) {
    s3 = rms_mg(s3, g, c);
    d = rms_denom_centered(s1, s3, a.eps);
  } else {
    d = rms_denom(s1, a.eps);
  }
  const float delta = rule_delta(g, lr, d);
  s2 = MOM ? rms_mom(s2, delta, a.momentum) : delta;
  p = p - s2;
}

template <int RULE, bool CENTERED, bool MOM, bool BF, bool EMA>
__device__ __forceinline__ void rule_body(const RuleArgs& a) {
  typedef RuleGrad<BF> G;
  const int64_t n4 = a.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kRuleThreads;
  const int64_t i0 = (int64_t)blockIdx.x * kRuleThreads + threadIdx.x;
  // the first item's operands are loaded before t, the clip factor and ok (dependent loads) are awaited
  RuleItem<BF> x{};
  if (i0 < n4) x = rule_load4<RULE, CENTERED, MOM, BF, EMA>(a, i0);
  const int64_t t = (a.step ? *a.step : 0) + a.t_offset;
  const float clip = *a.gscale;
  const float ok = a.ok ? *a.ok : 1.f;
  if (ok == 0.f) return;  // wave-uniform, before the first store: a skipped step writes nothing
  const float lr = lr_at(a.sched, t - 1);
  const float mul = a.grad_scale * clip;
  const float c = 1.f - a.decay;
  const float omd = EMA ? ema_omd_at(a.ema_decay, a.ema_num_updates, t) : 0.f;
  for (int64_t i = i0; i < n4; i += stride) {
    if (i != i0) x = rule_load4<RULE, CENTERED, MOM, BF, EMA>(a, i);
    const f32x4 g = G::f32(x.g) * mul;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float p = x.p[j], s1 = x.s1[j], s2 = x.s2[j], s3 = x.s3[j];
      rule_update<RULE, CENTERED, MOM>(a, g[j], lr, c, p, s1, s2, s3);
      x.p[j] = p; x.s1[j] = s1; x.s2[j] = s2; x.s3[j] = s3;
      if (EMA) x.e[j] = ema_step(x.e[j], p, omd);
    }
    rule_st4(a.p, i, x.p);
    rule_st4(a.s1, i, x.s1);
    if (RULE == RULE_RMSPROP) rule_st4(a.s2, i, x.s2);
    if (RULE == RULE_RMSPROP && CENTERED) rule_st4(a.s3, i, x.s3);
    if (a.pbf) reinterpret_cast<uint2*>(a.pbf)[i] = make_uint2(pack_bf2(x.p[0], x.p[1]), pack_bf2(x.p[2], x.p[3]));
    if (EMA) rule_st4(a.ema, i, x.e);
  }
  // scalar tail (n % 4)
  for (int64_t i = (n4 << 2) + i0; i < a.n; i += stride) {
    const float g = G::load1(a, i) * mul;
    float p = a.p[i], s1 = a.s1[i], s2 = 0.f, s3 = 0.f;
    if (RULE == RULE_RMSPROP && MOM) s2 = a.s2[i];
    if (RULE == RULE_RMSPROP && CENTERED) s3 = a.s3[i];
    rule_update<RULE, CENTERED, MOM>(a, g, lr, c, p, s1, s2, s3);
    a.p[i] = p;
    a.s1[i] = s1;
    if (RULE == RULE_RMSPROP) a.s2[i] = s2;
    if (RULE == RULE_RMSPROP && CENTERED) a.s3[i] = s3;
    if (a.pbf) a.pbf[i] = f2bf_bits(p);
    if (EMA) a.ema[i] = ema_step(a.ema[i], p, omd);
  }
}

// the wire format and the EMA shadow are tested once, around the whole body
template <int RULE, bool CENTERED, bool MOM>
__device__ __forceinline__ void rule_pick(const RuleArgs& a) {
  if (a.gbf) {
    if (a.ema) rule_body<RULE, CENTERED, MOM, true, true>(a);
    else rule_body<RULE, CENTERED, MOM, true, false>(a);
  } else {
    if (a.ema) rule_body<RULE, CENTERED, MOM, false, true>(a);
    else rule_body<RULE, CENTERED, MOM, false, false>(a);
  }
}
template <bool CENTERED, bool MOM>
__global__ __launch_bounds__(kRuleThreads) void rmsprop_kernel(RuleArgs a) {
  rule_pick<RULE_RMSPROP, CENTERED, MOM>(a);
}
__global__ __launch_bounds__(kRuleThreads) void adagrad_kernel(RuleArgs a) { rule_pick<RULE_ADAGRAD, false, false>(a); }

// as blocks_for(n, 4) of optim_kernels.h
int rule_blocks(int64_t n) {
  const int64_t b = (n / 4 + kRuleThreads - 1) / kRuleThreads;
  return (int)(b < 1 ? 1 : (b > kRuleMaxBlocks ? kRuleMaxBlocks : b));
}

void rule_check(const RuleArgs& a, const char* who, bool need_s2, bool need_s3) {
  auto need = [&](bool ok, const char* what) {
    if (!ok) throw std::runtime_error(std::string(who) + ": " + what);
  };
  need(a.n >= 1, "n >= 1");
  need(a.p && a.s1 && a.gscale, "p, the first slot and gscale are required");
  need(!need_s2 || a.s2, "the mom slot is required");
  need(!need_s3 || a.s3, "the mg slot is required (centered)");
  need((a.g != nullptr) != (a.gbf != nullptr), "exactly one of g and gbf");
  need(((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.s1) | reinterpret_cast<uintptr_t>(a.s2) |
         reinterpret_cast<uintptr_t>(a.s3) | reinterpret_cast<uintptr_t>(a.ema) | reinterpret_cast<uintptr_t>(a.g)) & 15) == 0 &&
           ((reinterpret_cast<uintptr_t>(a.pbf) | reinterpret_cast<uintptr_t>(a.gbf)) & 7) == 0,
       "unaligned buffer (16 bytes for fp32, 8 for bf16)");
}

}  // namespace

void rmsprop_apply(const RuleArgs& a, bool centered, hipStream_t s) {
  rule_check(a, "rmsprop_apply", true, centered);
  const int nb = rule_blocks(a.n);
  const bool mom = a.momentum != 0.f;
  if (centered) {
    if (mom) TFD_LAUNCH(rmsprop_kernel<true, true><<<nb, kRuleThreads, 0, s>>>(a));
    else TFD_LAUNCH(rmsprop_kernel<true, false><<<nb, kRuleThreads, 0, s>>>(a));
  } else {
    if (mom) TFD_LAUNCH(rmsprop_kernel<false, true><<<nb, kRuleThreads, 0, s>>>(a));
    else TFD_LAUNCH(rmsprop_kernel<false, false><<<nb, kRuleThreads, 0, s>>>(a));
  }
}
void adagrad_apply(const RuleArgs& a, hipStream_t s) {
  rule_check(a, "adagrad_apply", false, false);
  TFD_LAUNCH(adagrad_kernel<<<rule_blocks(a.n), kRuleThreads, 0, s>>>(a));
}
int rules_max_blocks() { return kRuleMaxBlocks; }
int rules_threads() { return kRuleThreads; }

}  // namespace tfd
