// Gradient accumulation over micro-batches (kernels/grad_accum.hip): one flat streaming pass per
// micro-batch over n elements, in one of three modes chosen by the host per launch --
//   GA_STORE  acc[i] = g[i]             the first micro-batch: acc is never zero-filled
//   GA_ADD    acc[i] = acc[i] + g[i]    the ones in between
//   GA_EMIT   out[i] = acc[i] + g[i]    the last: acc is not written; out is fp32 (out) or bf16 rounded to
//                                       nearest even (outbf, when non-null) and may be g itself
// g is fp32 (g) or bf16 widened exactly (gbf, when non-null). Each element is one plain fp32 add in
// micro-batch order, no atomics: bit-identical run to run. Any n >= 1 and any element alignment of the
// pointers: a scalar head and tail surround a body of 16-byte accesses (all scalar when the pointers
// do not share one phase).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tfd {

enum GradAccumMode { GA_STORE = 0, GA_ADD = 1, GA_EMIT = 2 };

struct GradAccumArgs {
  float* acc;
  const float* g;
  const uint16_t* gbf;
  float* out;
  uint16_t* outbf;
  int64_t n;
  int mode;
  int64_t* bump;  // GA_EMIT, if set: *bump += 1 by one thread (the engine's global_step: the micro-batch
                  // kernels bump the micro counter, and the optimizer behind this launch reads t here)
};
// blocks / loads: 0 = the defaults (kernels/grad_accum.hip); the probe's A/B passes others
void grad_accum(const GradAccumArgs& a, hipStream_t s, int blocks = 0, int loads = 0);

}  // namespace tfd
