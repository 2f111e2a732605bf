// Device step log (csrc/step_log.h): one kernel, one block of 256 threads, two modes. SL_LOSS sums the
// head kernel's per-row loss and correct flags in fp64 -- per-thread strided partials, then a
// fixed-order shuffle tree inside each wave and the four wave totals added in wave order through LDS,
// so the record is bit-identical run to run -- and writes the step's record (or, under accumulation,
// stores / adds the two sums and writes the record with the last micro-batch). SL_NORM copies the
// step's {norm, scale, ok} into the record. Latency-bound: at the largest batch it reads 30 KB; the
// counter is one uniform load issued before the row loads. Plain stores only, no atomics; every
// field of a record is stored by the launch that owns it, so nothing is ever zero-filled.
#include "../common.h"
#include "../launch_check.h"
#include "../step_log.h"

namespace tfd {
namespace {

constexpr int kLogThreads = 256;
constexpr int kLogWaves = kLogThreads / kWave;

// every lane ends with nothing useful but lane 0, which holds the wave's sum in a fixed order
__device__ __forceinline__ double wave_sum_down(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}

// slot of the record of update t >= 1
__device__ __forceinline__ int64_t slot_of(int64_t t, int64_t capacity) {
  const int64_t r = (t - 1) % capacity;
  return r < 0 ? r + capacity : r;
}

__global__ __launch_bounds__(kLogThreads) void step_log_kernel(StepLogArgs a) {
  __shared__ double part[kLogWaves][2];
  const int64_t c = *a.counter;  // uniform address under no branch: one scalar load
  if (a.mode == SL_NORM) {
    // after the bump: the step just taken is update c
    if (c >= 1 && threadIdx.x < 3)
      a.rec[slot_of(c, a.capacity) * kStepLogFields + SLF_GRAD_NORM + threadIdx.x] = a.triple[threadIdx.x];
    return;
  }
  double l = 0.0, k = 0.0;
  for (int i = threadIdx.x; i < a.B; i += kLogThreads) {
    l += (double)a.loss_row[i];
    k += (double)a.correct_row[i];
  }
  l = wave_sum_down(l);
  k = wave_sum_down(k);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    part[w][0] = l;
    part[w][1] = k;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  l = part[0][0];
  k = part[0][1];
#pragma unroll
  for (int i = 1; i < kLogWaves; ++i) {
    l += part[i][0];
    k += part[i][1];
  }
  if (a.acc_mode == SL_STORE) {
    a.acc[0] = l;
    a.acc[1] = k;
    return;
  }
  if (a.acc_mode != SL_WHOLE) {  // micro-batch order: one plain fp64 add each
    l = a.acc[0] + l;
    k = a.acc[1] + k;
    if (a.acc_mode == SL_ADD) {
      a.acc[0] = l;
      a.acc[1] = k;
      return;
    }
  }
  if (c < 0) return;
  const int64_t s = c / a.accum;  // the update index: global_step before the update
  const int64_t rows = a.accum * (int64_t)a.B;
  const int64_t slot = slot_of(s + 1, a.capacity);
  f32x4* r = reinterpret_cast<f32x4*>(a.rec + slot * kStepLogFields);
  r[0] = f32x4{(float)(l / (double)rows), (float)k, lr_at(a.sched, s), __uint_as_float(0x7FC00000u)};
  r[1] = f32x4{1.f, 1.f, (float)rows, 0.f};
  a.t[slot] = s + 1;
}

}  // namespace

void step_log(const StepLogArgs& a, hipStream_t s) {
  if (!a.t || !a.rec || a.capacity < 1 || !a.counter) throw std::runtime_error("step_log: t, rec, capacity >= 1 and counter");
  if ((reinterpret_cast<uintptr_t>(a.rec) & 31) != 0) throw std::runtime_error("step_log: rec must be 32-byte aligned");
  if (a.mode == SL_NORM) {
    if (!a.triple) throw std::runtime_error("step_log: SL_NORM needs the {norm, scale, ok} triple");
  } else if (a.mode == SL_LOSS) {
    if (!a.loss_row || !a.correct_row || a.B < 1) throw std::runtime_error("step_log: SL_LOSS needs the rows and B >= 1");
    if (a.acc_mode < SL_WHOLE || a.acc_mode > SL_EMIT) throw std::runtime_error("step_log: acc_mode");
    if (a.accum < 1 || (a.acc_mode == SL_WHOLE) != (a.accum == 1))
      throw std::runtime_error("step_log: SL_WHOLE goes with accum == 1 and only with it");
    if (a.acc_mode != SL_WHOLE && !a.acc) throw std::runtime_error("step_log: accumulation needs acc");
  } else {
    throw std::runtime_error("step_log: mode");
  }
  TFD_LAUNCH(step_log_kernel<<<1, kLogThreads, 0, s>>>(a));
}

}  // namespace tfd
