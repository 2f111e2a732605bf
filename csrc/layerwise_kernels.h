// Host-side launcher API of the layer-wise optimizer kernels (kernels/optim_layerwise.hip; the
// definitions are in layerwise.h). Three launches over one block table:
//   stage 1  per block: LAMB reads p, m, v, g, writes m', v', forms u; LARS reads p, g and writes
//            nothing else; each block stores its fp32 partial sums {sum p^2, sum u^2 or sum g^2}
//   stage 2  per variable: the blocks' partials summed in block order in fp64, the ratio function,
//            out[s] = {|p|, |u| or |g|, r}
//   stage 3  per block: reads its variable's r, writes p' (LARS: accum' too), the bf16 shadow when
//            pbf is given and the EMA shadow when ema is given
// Elements that belong to no segment are touched in no buffer.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "layerwise.h"
#include "lr_schedule.h"

namespace tfd {

struct LayerwiseArgs {
  float* p;
  float* s1;            // LAMB: m; LARS: accum
  float* s2;            // LAMB: v; LARS: unused
  const float* g;       // fp32 gradient, or
  const uint16_t* gbf;  // (when non-null) the bf16 wire
  uint16_t* pbf;        // bf16 shadow of p, or null
  const LwBlock* blocks;      // device [nblocks]
  const LwSegBlocks* segs;    // device [nsegs]
  int nblocks, nsegs;
  float* partials;      // device [nblocks][2]; every entry is stored by every stage-1 launch
  float* out;           // device [nsegs][3] = {|p|, |u| or |g|, r}
  LrSchedule sched;     // lr = lr_at(sched, t - 1)
  float beta1, beta2;   // LAMB
  float momentum, eeta; // LARS
  float eps, weight_decay;
  const int64_t* step;  // t = *step + t_offset (null: t_offset)
  int t_offset;
  float grad_scale;     // the gradient's multiplier is grad_scale * *gscale
  const float* gscale;  // device clip factor; a device 1.0f without clipping
  float* ema;           // moving average of the weights (ema.h), or null
  float ema_decay;
  int ema_num_updates;
  const float* ok;      // non-finite guard (grad_guard.hip): device ok of {norm, scale, ok}, or null. With
                        // *ok == 0 no stage stores to p, s1, s2, pbf or ema; partials and out are written
                        // and hold nothing specified
};

void lamb_apply(const LayerwiseArgs& a, hipStream_t s);  // stages 1, 2, 3
void lars_apply(const LayerwiseArgs& a, hipStream_t s);
// stages 1 and 2 on one buffer (a.g or a.gbf): out[s] = {|x|, |x|, 1}
void layer_norms_apply(const LayerwiseArgs& a, hipStream_t s);

}  // namespace tfd
