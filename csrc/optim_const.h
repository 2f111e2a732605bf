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

}  // namespace tfd
