// Exponential moving average of the weights (tf.train.ExponentialMovingAverage, the
// variable_averages of SyncReplicasOptimizer), updated inside the optimizer kernels. ONE definition
// for the host and the device, as lr_schedule.h is for the rate:
//   d_t = decay                                   (num_updates off)
//   d_t = min(decay, (1 + t) / (10 + t))          (num_updates on: TF's num_updates = global_step)
//   e'  = e - (1 - d_t)(e - p') = fmaf(1 - d_t, p' - e, e)
// with p' the parameter AFTER the optimizer update and t Adam's t, global_step after this update. No
// zero-debias (TF's default): the shadow starts as a copy of the parameters.
//
// Rounding, all fp32. d_t: (1 + t) and (10 + t) are exact below 2^24, the quotient rounds once
// (|err| <= 2^-25 d_t, correctly rounded division) and the min is exact. omd = 1 - d_t rounds once
// more, by at most 2^-25 (omd <= 0.9 < 1). The update rounds twice: p' - e, then the fused
// multiply-add. So d_t read back through one update from e = 1, p = 0 (e' = 1 - omd, exact by
// Sterbenz for omd in [0.5, 1] and within 2^-25 otherwise) is within 3 * 2^-25 < 2 * 2^-24 of the
// fp64 value.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lr_schedule.h"  // TFD_HD

namespace tfd {

TFD_HD inline float ema_decay_at(float decay, int num_updates, int64_t t) {
  if (!num_updates) return decay;
  const float d = (1.f + (float)t) / (10.f + (float)t);
  return d < decay ? d : decay;
}
// 1 - d_t: what the kernels keep per thread
TFD_HD inline float ema_omd_at(float decay, int num_updates, int64_t t) {
  return 1.f - ema_decay_at(decay, num_updates, t);
}
// THE update: the only place that spells it (explicit operations, so -ffp-contract cannot reshape it)
TFD_HD inline float ema_step(float e, float p_new, float omd) { return fmaf(omd, p_new - e, e); }

}  // namespace tfd
