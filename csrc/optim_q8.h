// 8-bit Adam over the flat buffer: both moments kept as OCP fp8 codes with one fp32 scale per 256 elements.
// The definitions, ONE for the host and the device as optim_rules.h is for RMSProp / Adagrad, the argument
// structs of kernels/optim_q8.hip and its launchers. training/optimizers.py states the same in numpy.
//
//   blocks   block k covers flat elements [256 k, min(256 k + 256, n)); nb = ceil(n / 256). Blocks follow the
//            flat index and may straddle variables.
//   state    m8, v8: uint8[n];  am, av: float[nb], the block's max |m| and max v
//            m: e4m3 (float8_e4m3fn), normalised so that the block's maximum is 256
//            v: e5m2 (float8_e5m2),   normalised so that the block's maximum is 32768
//            both targets are powers of two and codes of their format, so scaling by them is exact
//   decode   m = dec_e4m3(m8) * (am * 2^-8);   v = dec_e5m2(v8) * (av * 2^-15)        (fp32, one product each)
//   encode   a' = max |x'| over the block, and a' = 0 where that maximum is below 2^-90 (the zero block, below);
//            inv = a' > 0 ? T / a' : 0  (one IEEE fp32 division per block);
//            code = cvt(x' * inv), round to nearest even. In a block with a' > 0, a v' > 0 whose code would be
//            0x00 takes 0x01: a parameter that has seen a gradient never divides by 0 + eps. The element that
//            attains a' gets the code of T and decodes to exactly a'; the zero block has scale 0 and codes 0.
//   zero     a block whose maximum is below kQ8Tiny = 2^-90 (8.1e-28) is stored as the zero block. T / a' is
//   block    finite only for a' above T / FLT_MAX (7.5e-37 for m, 9.6e-35 for v); below that inv = inf and
//            0 * inf = NaN would reach the codes of a block whose gradient is exactly zero, whose maximum
//            shrinks by beta1 per step. From 2^-90 up, inv <= 2^105 is finite and every decoded value
//            (>= 2^-90 2^-15 2^-16 = 2^-121) is a normal fp32 number. What is dropped moves nothing:
//            sqrt(v) < 2^-45 = 2.8e-14 beside eps, |m| < 8.1e-28 in the numerator. fp32 Adam decays to 0 likewise.
//   update   adam_kernel's element update (optim_kernels.h) on the DECODED m and v:
//            m' = m + (g - m)(1 - beta1);  v' = v + (g g - v)(1 - beta2);
//            p' = p - lr_t m' / (sqrt(v') + eps),  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)
//            with g = gradient * grad_scale * *gscale, t = *step + t_offset, lr = lr_at(sched, t - 1).
//            p' is formed from the unquantised m' and v', which are then encoded.
// decode followed by encode over the same blocks reproduces codes and scales: the maximum decodes to a', so
// the scale comes back, and every other value is dec(code) * (a' 2^-k) * fl(T / a'), within 2^-22 of dec(code)
// relatively -- far inside the rounding interval of its code (codes are at least 2^-4 apart relatively).
// Non-finite gradients are the guard's business (set_skip_nonfinite); without it the result on them is
// unspecified, and nothing faults.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "lr_schedule.h"  // TFD_HD, LrSchedule

namespace tfd {

constexpr int kQ8Block = 256;
enum Q8Kind : int { Q8_M = 0, Q8_V = 1 };  // e4m3 at target 256; e5m2 at target 32768

TFD_HD inline int64_t q8_blocks(int64_t n) { return (n + kQ8Block - 1) / kQ8Block; }
TFD_HD inline float q8_target(int kind) { return kind == Q8_M ? 256.f : 32768.f; }
// what a decoded code is multiplied by, and what a value is multiplied by before it is converted
TFD_HD inline float q8_dscale(float absmax, int kind) { return absmax * (kind == Q8_M ? 0x1p-8f : 0x1p-15f); }
constexpr float kQ8Tiny = 0x1p-90f;
// a block's stored maximum from its measured one: below kQ8Tiny (and for NaN) the zero block
TFD_HD inline float q8_absmax(float measured) { return measured >= kQ8Tiny ? measured : 0.f; }
// absmax: q8_absmax's result, so 0 or at least kQ8Tiny and the quotient is finite
TFD_HD inline float q8_inv(float absmax, int kind) { return absmax > 0.f ? q8_target(kind) / absmax : 0.f; }
// the element update, spelled as adam_apply4 spells it
TFD_HD inline float adam8_m(float m, float g, float c1) { return m + (g - m) * c1; }
TFD_HD inline float adam8_v(float v, float g, float c2) { return v + (g * g - v) * c2; }
TFD_HD inline float adam8_p(float p, float m_new, float v_new, float lr_t, float eps) {
  return p - lr_t * m_new / (sqrtf(v_new) + eps);
}
TFD_HD inline float adam8_lr_t(float lr, float beta1, float beta2, int64_t t) {
  const float b1p = powf(beta1, (float)t), b2p = powf(beta2, (float)t);
  return lr * sqrtf(1.f - b2p) / (1.f - b1p);
}

struct Adam8Args {
  float* p;
  uint8_t* m8;          // e4m3 codes of m
  uint8_t* v8;          // e5m2 codes of v
  float* am;            // [q8_blocks(n)] max |m| per block
  float* av;            // [q8_blocks(n)] max v per block
  const float* g;       // fp32 gradient, or
  const uint16_t* gbf;  // (when non-null) the bf16 wire
  uint16_t* pbf;        // bf16 shadow of p (round-to-nearest-even of the stored p'), or null
  int64_t n;
  LrSchedule sched;     // lr = lr_at(sched, t - 1)
  float beta1, beta2, eps;
  const int64_t* step;  // t = *step + t_offset (null: t_offset)
  int t_offset;
  float grad_scale;     // the gradient's multiplier is grad_scale * *gscale
  const float* gscale;  // device clip factor; a device 1.0f without clipping
  float* ema;           // moving average of the weights (ema.h), or null
  float ema_decay;
  int ema_num_updates;
  const float* ok;      // non-finite guard: device ok, or null. With *ok == 0 nothing is stored
};

// the codec alone: x (fp32[n]) <-> codes (uint8[n]) + absmax (float[q8_blocks(n)])
struct Q8CodecArgs {
  float* x;
  uint8_t* codes;
  float* absmax;
  int64_t n;
  int kind;
};

void adam8_apply(const Adam8Args& a, hipStream_t s);
void q8_encode_launch(const Q8CodecArgs& a, hipStream_t s);  // reads x
void q8_decode_launch(const Q8CodecArgs& a, hipStream_t s);  // writes x
// the launchers' grid cap (workgroups) and block size; a wave owns one 256-element block at a time, so a
// buffer above blocks * (threads / 64) * 256 elements takes a second grid-stride pass
int q8_max_blocks();
int q8_threads();

}  // namespace tfd
