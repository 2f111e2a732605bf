// Train-time data augmentation on the device (kernels/mnist_augment.hip): random shift / rotation /
// scale and Simard-style elastic distortion of the batch a training step is about to read, written
// into a feed-mode pair xaug [B][784] fp32 / yaug [B] int32 at the head of the step body. The step
// kernels then run as in feed mode (perm == nullptr) and never learn that the batch was warped.
//
// Definition, per batch row b (training/augment.py augment_batch_ref is the same in numpy fp64):
//   sample  i   = step * B + b            64-bit; the position of the row in the stream of samples
//   row         = perm[i % n]
//   draws       Philox4x32-10, counter = (i lo, i hi, draw, rank), key = (seed, kAugmentKey); each call
//               gives four u01 uniforms (24 bits). Nothing else enters: a replayed graph, an eager call,
//               an n-step graph and K micro-batches of B (samples K*t*B .. K*(t+1)*B - 1, the samples of
//               one batch of K*B at step t) all draw the same numbers for the same sample.
//     draw 0             {ty, tx, theta, s}: ty, tx = shift_px (2u - 1), theta = rotate_rad (2u - 1),
//                        s = 1 + scale (2u - 1)
//     draw 1 + k         k in [0, 196): N_x elements 4k .. 4k + 3 (row-major 28 x 28), each 2u - 1
//     draw 197 + k       the same for N_y
//   smoothing   S = alpha G N G^T, G[i][j] = g[|i - j|] (28 x 28 symmetric Toeplitz: the field is zero
//               outside the image), g[d] = exp(-d^2 / 2 sigma^2) / sum_{k=-27..27} exp(-k^2 / 2 sigma^2),
//               computed by the host in fp64 and rounded to fp32: the device evaluates no exponential
//   source      (y, x) = ctr + (1 / s) R(theta) ((r, c) - ctr) - (ty, tx) + (S_y[r][c], S_x[r][c]),
//               ctr = 13.5, R(theta) (dy, dx) = (cos dy - sin dx, sin dy + cos dx)
//   sample      bilinear with zeros outside [0, 27]^2 (continuous everywhere): the coordinate is clamped
//               to [-1, 28] and read from a zero-bordered tile
// With all five magnitudes 0 the output is the gathered row bit for bit.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tfd {

constexpr uint32_t kAugmentKey = 0xA06E17A1u;  // second Philox key word (dropout's is 0x5EED1234)
constexpr int kAugmentTaps = 28;               // g[0 .. 27]
enum AugmentDraw { AUG_DRAW_AFFINE = 0, AUG_DRAW_NX = 1, AUG_DRAW_NY = 197 };

struct AugmentConfig {
  float shift_px;       // |ty|, |tx| <= shift_px pixels
  float rotate_rad;     // |theta| <= rotate_rad
  float scale;          // s in [1 - scale, 1 + scale], scale < 1
  float elastic_alpha;  // displacement scale in pixels; 0: no elastic phases
  float elastic_sigma;  // the Gaussian's sigma in pixels (what g was computed from)
  float g[kAugmentTaps];
};
inline bool augment_on(const AugmentConfig& c) {
  return c.shift_px != 0.f || c.rotate_rad != 0.f || c.scale != 0.f || c.elastic_alpha != 0.f;
}
// the config of (shift_px, rotate_deg, scale, elastic_alpha, elastic_sigma), g included; throws
// std::invalid_argument on a negative magnitude, scale >= 1 or alpha > 0 without sigma > 0
AugmentConfig make_augment_config(double shift_px, double rotate_deg, double scale, double elastic_alpha,
                                  double elastic_sigma);

struct AugmentArgs {
  const float* data;    // [n][784] fp32, 16-byte aligned
  const int* labels;    // [n]
  const int* perm;      // [n], values in [0, n)
  const int64_t* step;  // the data cursor, on the device: global_step, or the micro-batch counter
  int n;                // >= 1
  int B;                // grid: one 256-thread block per batch row
  uint32_t seed, rank;
  float* xaug;          // [B][784], 16-byte aligned
  int* yaug;            // [B]
  AugmentConfig cfg;
};
void augment_batch(const AugmentArgs& a, hipStream_t s);

}  // namespace tfd
