// RMSProp and Adagrad over the flat buffer (tf.train.RMSPropOptimizer, tf.train.AdagradOptimizer): the
// per-element definitions, ONE for the host and the device as layerwise.h is for LAMB / LARS, the
// argument struct of kernels/optim_rules.hip and its launchers.
//
//   RMSProp (TF ApplyRMSProp / ApplyCenteredRMSProp)
//     ms'  = ms + (g g - ms)(1 - decay)
//     mg'  = mg + (g - mg)(1 - decay)                          (centered only)
//     d    = ms' + eps;   centered: d = ms' - mg' mg' + eps
//     mom' = momentum mom + lr g / sqrt(d);   p' = p - mom'
//     slots start as ms = 1, mom = 0, mg = 0
//   Adagrad (TF ApplyAdagrad)
//     accum' = accum + g g;   p' = p - lr g / sqrt(accum')     (no epsilon; accum starts > 0)
// g is the gradient times grad_scale * *gscale, lr = lr_at(sched, t - 1), t = *step + t_offset.
//
// There is no clamp on d, as in TF: ms' >= mg'^2 holds for the exact averages, but both are rounded, so
// a centered d can come out negative when the gradient has been constant for long (ms' - mg'^2 -> 0)
// and eps is below that rounding; sqrt then gives NaN and the element is NaN from there on. Choose eps
// above 2^-23 ms' for such gradients, as with TF.
//
// momentum == 0 (MOM = false, chosen on the host): mom is NOT read -- 0 * mom is dropped -- and
// mom' = lr g / sqrt(d) is still stored, so the slot and a checkpoint hold what TF's would. A
// non-finite stale mom (0 * inf = NaN in TF) is therefore not propagated; that is the one difference.
//
// Every update is spelled with explicit fmaf / mul / div / sqrtf, so -ffp-contract cannot reshape it.
// The one free place is g itself (gradient * multiplier), whose product the device compiler may contract
// into the g - mg of the centered rule: one rounding fewer, inside the bounds of tests/test_rules_gpu.py.
// 1 - decay is formed in fp32 from the fp32 decay, which is within 2^-24 decay of the fp64 one; the
// subtraction is exact for decay in [0.5, 1] (Sterbenz) and rounds once below. The coefficient therefore
// differs from the fp64 1 - decay by up to (decay / (1 - decay) + 1) * 2^-24 relatively, the bound the
// tests and docs/DESIGN.md section 9g use for every decay: 10 * 2^-24 at decay = 0.9 (9 * 2^-24 of it from
// the decay's own rounding, the rest the subtraction's, which is 0 there).
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "lr_schedule.h"  // TFD_HD, LrSchedule

namespace tfd {

TFD_HD inline float rms_ms(float ms, float g, float c) { return fmaf(fmaf(g, g, -ms), c, ms); }
TFD_HD inline float rms_mg(float mg, float g, float c) { return fmaf(g - mg, c, mg); }
TFD_HD inline float rms_denom(float ms_new, float eps) { return ms_new + eps; }
TFD_HD inline float rms_denom_centered(float ms_new, float mg_new, float eps) { return fmaf(-mg_new, mg_new, ms_new) + eps; }
// lr g / sqrt(d): the whole of mom' when momentum == 0
TFD_HD inline float rule_delta(float g, float lr, float d) { return lr * g / sqrtf(d); }
TFD_HD inline float rms_mom(float mom, float delta, float momentum) { return fmaf(momentum, mom, delta); }
TFD_HD inline float adagrad_accum(float accum, float g) { return fmaf(g, g, accum); }

struct RuleArgs {
  float* p;
  float* s1;            // RMSProp: ms;  Adagrad: accum
  float* s2;            // RMSProp: mom (written always, read when momentum != 0);  Adagrad: unused
  float* s3;            // centered RMSProp: mg;  otherwise unused
  const float* g;       // fp32 gradient, or
  const uint16_t* gbf;  // (when non-null) the bf16 wire
  uint16_t* pbf;        // bf16 shadow of p (round-to-nearest-even of the stored p'), or null
  int64_t n;
  LrSchedule sched;     // lr = lr_at(sched, t - 1)
  float decay, momentum, eps;  // RMSProp
  const int64_t* step;  // t = *step + t_offset (null: t_offset)
  int t_offset;
  float grad_scale;     // the gradient's multiplier is grad_scale * *gscale
  const float* gscale;  // device clip factor; a device 1.0f without clipping
  float* ema;           // moving average of the weights (ema.h), or null
  float ema_decay;
  int ema_num_updates;
  const float* ok;      // non-finite guard (grad_guard.hip): device ok, or null. With *ok == 0 nothing is stored
};

// one launch each; centered needs s3, and momentum == 0 picks the instantiation that does not read s2
void rmsprop_apply(const RuleArgs& a, bool centered, hipStream_t s);
void adagrad_apply(const RuleArgs& a, hipStream_t s);
// the launchers' grid cap (blocks) and block size: a buffer above blocks * threads * 4 elements takes
// a second grid-stride pass
int rules_max_blocks();
int rules_threads();

}  // namespace tfd
