// Constant-rate views of the optimizer kernels' argument structs (device code: included by the .hip
// sources only). Every optimizer kernel is a template over its argument struct: AdamArgs / SgdArgs /
// MnistAdamArgs carry an LrSchedule (lr_schedule.h) that the kernel evaluates from the device step
// counter; the *Const structs below carry the bare rate instead -- the kernel-argument layout and,
// instruction for instruction, the code these kernels had before schedules existed. The launchers
// pick the instantiation from the schedule's kind on the host, so the default (constant) path has no
// schedule code to branch over and no larger argument block (with the schedule behind a device-side
// compare the fused MNIST tail doubled in size and the step measured 0.6 us slower,
// profiles/lr_schedule_bench_ab.log). The scheduled instantiations are compiled in .hip files of their
// own (optim_sched.hip, mnist_tail_sched.hip), so the default path's code objects hold what they held.
#pragma once
#include "common.h"
#include "ema.h"
#include "tfd_kernels.h"

namespace tfd {

struct AdamConst {
  float* p; float* m; float* v; const float* g; uint16_t* pbf;
  const uint16_t* gbf;
  int64_t n;
  float lr, beta1, beta2, eps;
  const int64_t* step;
  int t_offset;
  float grad_scale;
};
struct SgdConst {
  float* p; float* mom; const float* g; uint16_t* pbf; const uint16_t* gbf; int64_t n;
  float lr, momentum, weight_decay, grad_scale; int nesterov;
};
struct MnistAdamConst {
  float* p; float* m; float* v;
  uint16_t* pbf;
  float lr, beta1, beta2, eps;
  const int64_t* t;
  int64_t* step;
  const uint16_t* gbf;
};
// The views are written out field by field, so they are pinned to the structs they mirror: a field
// added to AdamArgs / SgdArgs / MnistAdamArgs changes its size and must be added here (struct and
// conversion) before these hold again.
static_assert(sizeof(AdamArgs) == 192 && sizeof(AdamConst) == 88, "AdamArgs changed: update AdamConst and adam_const");
static_assert(sizeof(SgdArgs) == 184 && sizeof(SgdConst) == 72, "SgdArgs changed: update SgdConst and sgd_const");
static_assert(sizeof(MnistAdamArgs) == 176 && sizeof(MnistAdamConst) == 72,
              "MnistAdamArgs changed: update MnistAdamConst and mnist_adam_const");
inline AdamConst adam_const(const AdamArgs& a) {
  return AdamConst{a.p, a.m, a.v, a.g, a.pbf, a.gbf, a.n, a.sched.lr, a.beta1, a.beta2, a.eps, a.step, a.t_offset,
                   a.grad_scale};
}
inline SgdConst sgd_const(const SgdArgs& a) {
  return SgdConst{a.p, a.mom, a.g, a.pbf, a.gbf, a.n, a.sched.lr, a.momentum, a.weight_decay, a.grad_scale, a.nesterov};
}
inline MnistAdamConst mnist_adam_const(const MnistAdamArgs& o) {
  return MnistAdamConst{o.p, o.m, o.v, o.pbf, o.sched.lr, o.beta1, o.beta2, o.eps, o.t, o.step, o.gbf};
}

// The rate of the update whose Adam t is given: a schedule reads s = t - 1, global_step before the
// update. Evaluated where the kernels consume t, so their first operand loads are issued before the
// step counter is awaited.
__device__ __forceinline__ float base_lr(const AdamConst& a, int64_t) { return a.lr; }
__device__ __forceinline__ float base_lr(const AdamArgs& a, int64_t t) { return lr_at(a.sched, t - 1); }
__device__ __forceinline__ float base_lr(const MnistAdamConst& o, int64_t) { return o.lr; }
__device__ __forceinline__ float base_lr(const MnistAdamArgs& o, int64_t t) { return lr_at(o.sched, t - 1); }
// (the constant kind never touches the step counter)
__device__ __forceinline__ float base_lr(const SgdConst& a) { return a.lr; }
__device__ __forceinline__ float base_lr(const SgdArgs& a) {
  return lr_at(a.sched, (a.step ? *a.step : 0) + a.t_offset - 1);
}

// The kernels' view of their argument: the struct itself, or the one a clip wrapper holds
// (AdamClipArgs / SgdClipArgs, tfd_kernels.h). clip_load is the wrapper's clip factor, {norm, scale}[1]
// of grad_norm.hip read from the device once per thread -- for a bare struct an empty tag, so that the
// unclipped instantiations' gradient multiplier is a.grad_scale where it is used, as it always was.
struct NoClip {};
template <class A>
__device__ __forceinline__ const A& optim_args(const A& a) { return a; }
__device__ __forceinline__ const AdamArgs& optim_args(const AdamClipArgs& k) { return k.a; }
__device__ __forceinline__ const SgdArgs& optim_args(const SgdClipArgs& k) { return k.a; }
template <class A>
__device__ __forceinline__ NoClip clip_load(const A&) { return NoClip{}; }
__device__ __forceinline__ float clip_load(const AdamClipArgs& k) { return *k.gscale; }
__device__ __forceinline__ float clip_load(const SgdClipArgs& k) { return *k.gscale; }
template <class A>
__device__ __forceinline__ float grad_mul(const A& a, NoClip) { return a.grad_scale; }
template <class A>
__device__ __forceinline__ float grad_mul(const A& a, float clip) { return a.grad_scale * clip; }

// The moving average of the weights (ema.h), for the EMA wrappers (AdamEmaArgs / SgdEmaArgs /
// MnistAdamEmaArgs, tfd_kernels.h): ema_of(k) is the shadow and its decay, ema_omd its 1 - d_t at
// Adam's t, ema_load4 / ema_store4 the shadow's float4 beside p's, ema_update1 the scalar form. For
// every other struct ema_of is an empty tag and each of these is empty, so those instantiations hold
// the code they held.
struct NoEma {};
struct EmaRef { float* e; float decay; int num_updates; };
template <class K>
__device__ __forceinline__ NoEma ema_of(const K&) { return NoEma{}; }
__device__ __forceinline__ EmaRef ema_of(const AdamEmaArgs& k) { return EmaRef{k.ema, k.decay, k.num_updates}; }
__device__ __forceinline__ EmaRef ema_of(const SgdEmaArgs& k) { return EmaRef{k.ema, k.decay, k.num_updates}; }
__device__ __forceinline__ EmaRef ema_of(const MnistAdamEmaArgs& k) { return EmaRef{k.ema, k.decay, k.num_updates}; }
__device__ __forceinline__ const AdamArgs& optim_args(const AdamEmaArgs& k) { return k.k.a; }
__device__ __forceinline__ const SgdArgs& optim_args(const SgdEmaArgs& k) { return k.k.a; }
__device__ __forceinline__ float clip_load(const AdamEmaArgs& k) { return *k.k.gscale; }
__device__ __forceinline__ float clip_load(const SgdEmaArgs& k) { return *k.k.gscale; }
// the fused MNIST tail's view of its argument: the struct itself, or the one the EMA wrapper holds
// (host too: the launcher passes the view's pointers as the kernel's leading parameters)
template <class O>
__host__ __device__ __forceinline__ const O& tail_args(const O& o) { return o; }
__host__ __device__ __forceinline__ const MnistAdamArgs& tail_args(const MnistAdamEmaArgs& k) { return k.o; }

// The non-finite guard (GuardArgs<K>, tfd_kernels.h; optim_guard.hip holds the instantiations): every
// view above is that of the wrapped K. guard_load is ok of grad_guard.hip's {norm, scale, ok}, read from
// the device once per thread through a uniform address -- a load like t and the clip factor -- and
// guard_skip whether the kernel returns before its first store. For every other struct guard_load is an
// empty tag and guard_skip a constant false, so those instantiations hold the code they held.
struct NoGuard {};
template <class K>
__device__ __forceinline__ decltype(auto) optim_args(const GuardArgs<K>& g) { return optim_args(g.k); }
template <class K>
__device__ __forceinline__ float clip_load(const GuardArgs<K>& g) { return clip_load(g.k); }
template <class K>
__device__ __forceinline__ auto ema_of(const GuardArgs<K>& g) { return ema_of(g.k); }
template <class K>
__device__ __forceinline__ NoGuard guard_load(const K&) { return NoGuard{}; }
template <class K>
__device__ __forceinline__ float guard_load(const GuardArgs<K>& g) { return *g.ok; }
__device__ __forceinline__ constexpr bool guard_skip(NoGuard) { return false; }
__device__ __forceinline__ bool guard_skip(float ok) { return ok == 0.f; }

__device__ __forceinline__ NoEma ema_omd(NoEma, int64_t) { return NoEma{}; }
__device__ __forceinline__ float ema_omd(const EmaRef& r, int64_t t) { return ema_omd_at(r.decay, r.num_updates, t); }
__device__ __forceinline__ NoEma ema_load4(NoEma, int64_t) { return NoEma{}; }
__device__ __forceinline__ f32x4 ema_load4(const EmaRef& r, int64_t i) { return reinterpret_cast<const f32x4*>(r.e)[i]; }
__device__ __forceinline__ void ema_store4(NoEma, int64_t, NoEma, NoEma, const f32x4&) {}
__device__ __forceinline__ void ema_store4(const EmaRef& r, int64_t i, f32x4 e, float omd, const f32x4& p) {
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = ema_step(e[j], p[j], omd);
  reinterpret_cast<f32x4*>(r.e)[i] = e;
}
__device__ __forceinline__ void ema_update1(NoEma, int64_t, NoEma, float) {}
__device__ __forceinline__ void ema_update1(const EmaRef& r, int64_t i, float omd, float p) {
  r.e[i] = ema_step(r.e[i], p, omd);
}

}  // namespace tfd
