// Device step log (kernels/step_log.hip): a ring of per-step records written inside the step graph, so
// that a replayed n-step graph leaves the loss curve, the clip history and the guard's decisions of
// every step behind and the host reads them once per call instead of once per step.
//   t   int64 [C]     the step number of the record in that slot (0: never written)
//   rec fp32  [C][8]  {loss, correct, lr, grad_norm, clip_scale, ok, rows, reserved}
// The record of update t -- t is global_step after the update -- lives in slot (t - 1) % C. One launch
// of one 256-thread block per mode, plain vector stores, no atomics and nothing to zero: every replay
// of a captured graph writes its own records, and a reused slot is written whole.
//   SL_LOSS  behind the head kernel of every training (micro-)batch, on its stream. counter is what
//            the head reads -- global_step or, under accumulation, the micro counter m -- BEFORE its
//            bump; the update index is s = m / K and t = s + 1. Sums loss_row[0..B) and
//            correct_row[0..B) in fp64 in a fixed order. acc_mode, chosen by the host per launch as
//            grad_accum's is:
//              SL_WHOLE  (K = 1) writes the whole record: loss = fp32(sum / B), correct, rows = B,
//                        lr = lr_at(sched, s), grad_norm = NaN, clip_scale = 1, ok = 1
//              SL_STORE  acc = {sum loss, sum correct}          the first micro-batch
//              SL_ADD    acc += ...                             the ones in between
//              SL_EMIT   the whole record from acc + ..., rows = K * B; acc is not written
//   SL_NORM  behind the norm / guard finish, on its stream, AFTER the step bump: copies the device
//            triple {norm, scale, ok} into fields 3..5 of slot (global_step - 1) % C.
// Nothing reads the log back on the device: the step computes the same bits with it on and off.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "lr_schedule.h"

namespace tfd {

enum StepLogMode { SL_LOSS = 0, SL_NORM = 1 };
enum StepLogAcc { SL_WHOLE = 0, SL_STORE = 1, SL_ADD = 2, SL_EMIT = 3 };
constexpr int kStepLogFields = 8;
enum StepLogField { SLF_LOSS = 0, SLF_CORRECT, SLF_LR, SLF_GRAD_NORM, SLF_CLIP_SCALE, SLF_OK, SLF_ROWS, SLF_RESERVED };

struct StepLogArgs {
  int64_t* t;              // [capacity]
  float* rec;              // [capacity][8], 32-byte aligned
  int64_t capacity;        // >= 1
  const int64_t* counter;  // SL_LOSS: the head's counter before its bump; SL_NORM: global_step after it
  int mode;                // StepLogMode
  // SL_LOSS
  int acc_mode;            // StepLogAcc
  int64_t accum;           // K >= 1 (SL_WHOLE: 1)
  const float* loss_row;   // [B]
  const float* correct_row;
  int B;
  double* acc;             // [2], K > 1 only
  LrSchedule sched;
  // SL_NORM
  const float* triple;     // {norm, scale, ok}
};
void step_log(const StepLogArgs& a, hipStream_t s);

}  // namespace tfd
