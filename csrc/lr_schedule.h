// Learning-rate schedules as a function of global_step (tf.train.exponential_decay,
// piecewise_constant, polynomial_decay, cosine_decay, plus a linear warm-up). ONE definition for the
// host and the device: the optimizer kernels evaluate lr_at() from the device step counter they
// already read for Adam's t, so a captured step graph follows the schedule with no re-capture and
// no read-back; the GPU parameter server evaluates the same function on the host from its update
// count. The struct is a POD passed by value in kernel arguments.
//
// s is global_step BEFORE the update (Adam's t - 1), which is what TF's graph reads.
#pragma once
#include <math.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

// always inlined: an out-of-line call inside a kernel waits for every outstanding load at the call
#if defined(__HIPCC__) || defined(__CUDACC__)
#define TFD_HD __host__ __device__ __attribute__((always_inline))
#else
#define TFD_HD __attribute__((always_inline))
#endif

namespace tfd {

enum LrKind : int { LR_CONSTANT = 0, LR_EXPONENTIAL = 1, LR_PIECEWISE = 2, LR_POLYNOMIAL = 3, LR_COSINE = 4 };
constexpr int kLrMaxBoundaries = 4;

struct LrSchedule {
  int kind;                 // LrKind. LR_CONSTANT never has a warm-up (make_lr_schedule in the runtime
                            // rewrites constant + warm-up as a piecewise schedule with no boundary), so
                            // the default path is one compare and the stored float
  int staircase;            // exponential: integer quotient s / decay_steps
  float lr;                 // base rate (constant: THE rate, returned untouched)
  float rate;               // exponential: decay rate
  float end;                // polynomial: end rate
  float power;              // polynomial: exponent
  float alpha;              // cosine: floor as a fraction of lr
  int nb;                   // piecewise: number of boundaries given (0..4)
  int64_t decay_steps;      // >= 1
  int64_t warmup_steps;     // w > 0: lr(s) *= (s + 1) / w for s < w
  int64_t boundaries[kLrMaxBoundaries];
  float values[kLrMaxBoundaries + 1];  // absolute rates, returned untouched
};

inline LrSchedule lr_constant(float lr) {
  LrSchedule sc{};
  sc.kind = LR_CONSTANT;
  sc.lr = lr;
  sc.decay_steps = 1;
  return sc;
}

// Build and validate a schedule from its flat description (the form the torch bindings take):
// kind: constant | exponential | piecewise | polynomial | cosine;
// params: {lr, decay_steps, rate, end, power, alpha, warmup_steps, staircase} (trailing ones optional;
// defaults 0, 1, 1, 0, 1, 0, 0, 0); boundaries / values: piecewise only.
inline LrSchedule make_lr_schedule(const std::string& kind, const std::vector<double>& params,
                                   const std::vector<int64_t>& boundaries, const std::vector<double>& values) {
  auto par = [&](size_t i, double dflt) { return i < params.size() ? params[i] : dflt; };
  // step counts arrive as doubles: integral and below 2^53 (exactly representable), or an error
  auto steps = [&](size_t i, double dflt, const char* name) {
    const double v = par(i, dflt);
    if (!(v >= 0.0 && v <= 9007199254740992.0) || v != floor(v))
      throw std::invalid_argument(std::string("lr schedule: ") + name + " must be a non-negative integer");
    return (int64_t)v;
  };
  LrSchedule sc{};
  sc.lr = (float)par(0, 0.0);
  sc.decay_steps = steps(1, 1.0, "decay_steps");
  sc.rate = (float)par(2, 1.0);
  sc.end = (float)par(3, 0.0);
  sc.power = (float)par(4, 1.0);
  sc.alpha = (float)par(5, 0.0);
  sc.warmup_steps = steps(6, 0.0, "warmup_steps");
  sc.staircase = par(7, 0.0) != 0.0 ? 1 : 0;
  if (kind == "constant") sc.kind = LR_CONSTANT;
  else if (kind == "exponential") sc.kind = LR_EXPONENTIAL;
  else if (kind == "piecewise") sc.kind = LR_PIECEWISE;
  else if (kind == "polynomial") sc.kind = LR_POLYNOMIAL;
  else if (kind == "cosine") sc.kind = LR_COSINE;
  else throw std::invalid_argument("lr schedule: unknown kind '" + kind + "'");
  if (sc.decay_steps < 1) throw std::invalid_argument("lr schedule: decay_steps >= 1");
  if (sc.warmup_steps < 0) throw std::invalid_argument("lr schedule: warmup_steps >= 0");
  if (sc.kind != LR_PIECEWISE && (!boundaries.empty() || !values.empty()))
    throw std::invalid_argument("lr schedule: boundaries / values belong to the piecewise kind");
  std::vector<double> vals = values;
  if (sc.kind == LR_CONSTANT && sc.warmup_steps > 0) {  // keeps the constant kind free of arithmetic
    sc.kind = LR_PIECEWISE;
    vals.assign(1, (double)sc.lr);
  }
  if (sc.kind == LR_PIECEWISE) {
    if (boundaries.size() > (size_t)kLrMaxBoundaries) throw std::invalid_argument("lr schedule: at most 4 boundaries");
    if (vals.size() != boundaries.size() + 1)
      throw std::invalid_argument("lr schedule: len(values) must be len(boundaries) + 1");
    for (size_t i = 1; i < boundaries.size(); ++i)
      if (boundaries[i] <= boundaries[i - 1]) throw std::invalid_argument("lr schedule: boundaries must increase strictly");
    sc.nb = (int)boundaries.size();
    for (int i = 0; i < kLrMaxBoundaries; ++i) sc.boundaries[i] = i < sc.nb ? boundaries[i] : INT64_MAX;
    for (int i = 0; i <= kLrMaxBoundaries; ++i) sc.values[i] = (float)vals[i < sc.nb ? i : sc.nb];
    // the last given value sits at index nb; an unused boundary (INT64_MAX >= every s) must select it
  }
  return sc;
}

TFD_HD inline float lr_at(const LrSchedule& sc, int64_t s) {
  if (sc.kind == LR_CONSTANT) return sc.lr;
  float lr;
  if (sc.kind == LR_PIECEWISE) {
    // TF's inclusive convention: v_i for the first i with s <= b_i, else the last value
    // (unused boundaries are INT64_MAX and unused values repeat the last one -- make_lr_schedule --
    // so every index here is static: no scratch copy of the kernel-argument struct)
    lr = sc.values[kLrMaxBoundaries];
#pragma unroll
    for (int i = kLrMaxBoundaries - 1; i >= 0; --i)
      if (s <= sc.boundaries[i]) lr = sc.values[i];
  } else if (sc.kind == LR_EXPONENTIAL) {
    const float e = sc.staircase ? (float)(s / sc.decay_steps) : (float)s / (float)sc.decay_steps;
    lr = sc.lr * powf(sc.rate, e);
  } else {
    const float f = (float)(s < sc.decay_steps ? s : sc.decay_steps) / (float)sc.decay_steps;
    if (sc.kind == LR_POLYNOMIAL) {
      lr = (sc.lr - sc.end) * powf(1.f - f, sc.power) + sc.end;
    } else {
      // 0.5 (1 + cos(pi f)) = cos^2(pi f / 2): no cancellation near f = 1
      const float c = cosf(1.57079632679489662f * f);
      lr = sc.lr * ((1.f - sc.alpha) * (c * c) + sc.alpha);
    }
  }
  if (s < sc.warmup_steps) lr *= (float)(s + 1) / (float)sc.warmup_steps;
  return lr;
}

}  // namespace tfd
