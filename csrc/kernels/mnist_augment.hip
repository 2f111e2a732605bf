// Device data augmentation (csrc/mnist_augment.h): one 256-thread block warps one image of the batch.
//
//   load      the row's 196 16-byte loads are issued first (step -> perm -> row is the only dependent
//             chain); under their latency every thread draws the affine parameters (the same Philox
//             counter in every thread: no broadcast) and threads 0..195 draw the two noise fields, two
//             Philox calls each. The pixels land in a 30 x 30 zero-bordered LDS tile.
//   smooth    S = alpha G N G^T on the fp32 matrix core (v_mfma_f32_16x16x4_f32, gemm_f32.h). A field is
//             a 32 x 32 LDS image with a row stride of 48 floats: the four lane groups of a B-fragment
//             read four consecutive rows, 0 / 48 / 96 / 144 floats = banks 0 / 48 / 32 / 16 of 64, 16
//             lanes each: conflict-free. G never exists in memory: a lane builds its eight A values from
//             the 28-entry table (zero where either index is >= 28, which also keeps the padding zero).
//             Both passes are ONE routine, out = (G in)^T: pass 1 gives (G N)^T = N^T G, pass 2 gives
//             (G N^T G)^T = G N G^T (G is symmetric), so no pass reads an LDS image by columns, and the
//             transposed store is one 16-byte write per tile (a lane's four C rows are four consecutive
//             columns of the transposed image). Wave w takes field w >> 1 and the row tile w & 1 of it,
//             both column tiles behind one A fragment: 2 tiles x 8 K-steps per wave and pass, 128 MFMAs
//             per image.
//   resample  threads 0..195 produce four contiguous destination pixels each, four LDS taps per pixel,
//             and store one 16-byte vector; thread 0 stores the label.
// elastic_alpha == 0 skips the noise and both passes behind a block-uniform branch. Plain vector
// stores only: no atomics, nothing to clear.
#include "../mnist_augment.h"

#include <cmath>
#include <stdexcept>

#include "../common.h"
#include "../gemm_f32.h"
#include "../launch_check.h"

namespace tfd {
namespace {

constexpr int kAugThreads = 256;
constexpr int IMG = 28, PIX = IMG * IMG, CHUNKS = PIX / 4;
constexpr int TS = IMG + 2;        // the zero-bordered tile: pixel (r, c) at (r + 1) * TS + c + 1
constexpr int FS = 48;             // row stride of a 32 x 32 field image
constexpr int FIELD = 32 * FS;
constexpr float CTR = 13.5f;
static_assert(IMG % 4 == 0 && CHUNKS <= kAugThreads && 4 * (IMG + 1) <= kAugThreads, "one chunk, one border cell per thread");

__device__ __forceinline__ float sym(uint32_t x) { return 2.f * u01(x) - 1.f; }  // exact: a multiple of 2^-23

// out = scale (G in)^T for rows [16 ti, 16 ti + 16) of G in, both column tiles; ga[ks] = G[16 ti + (lane & 15)][4 ks + (lane >> 4)].
// MASK: `in` holds 28 x 28 numbers in an image whose padding was never written.
template <bool MASK>
__device__ __forceinline__ void smooth_pass(const float* in, float* out, const float (&ga)[8], float scale, int ti, int lane) {
  const int n = lane & 15, kg = lane >> 4;
  float b0[8], b1[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const int k = 4 * ks + kg;
    b0[ks] = in[k * FS + n];
    b1[ks] = in[k * FS + 16 + n];
    if (MASK) {
      if (k >= IMG) b0[ks] = 0.f;
      if (k >= IMG || 16 + n >= IMG) b1[ks] = 0.f;
    }
  }
  f32x4 c0 = zero_f4(), c1 = zero_f4();
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    c0 = mfma16x16x4f32(ga[ks], b0[ks], c0);
    c1 = mfma16x16x4f32(ga[ks], b1[ks], c1);
  }
  // C rows 16 ti + 4 kg + {0..3} of column 16 tj + n  ->  row 16 tj + n, columns 16 ti + 4 kg + {0..3}
  *reinterpret_cast<f32x4*>(out + n * FS + 16 * ti + 4 * kg) = c0 * scale;
  *reinterpret_cast<f32x4*>(out + (16 + n) * FS + 16 * ti + 4 * kg) = c1 * scale;
}

// bilinear sample of the zero-bordered tile; any coordinate, NaN included, reads inside the tile
__device__ __forceinline__ float bilinear(const float* tile, float y, float x) {
  y = fminf(fmaxf(y, -1.f), (float)IMG);
  x = fminf(fmaxf(x, -1.f), (float)IMG);
  const float y0 = fminf(floorf(y), (float)(IMG - 1)), x0 = fminf(floorf(x), (float)(IMG - 1));
  const float wy = y - y0, wx = x - x0;
  const float* p = tile + ((int)y0 + 1) * TS + (int)x0 + 1;
  const float top = (1.f - wx) * p[0] + wx * p[1];
  const float bot = (1.f - wx) * p[TS] + wx * p[TS + 1];
  return (1.f - wy) * top + wy * bot;
}

__global__ __launch_bounds__(kAugThreads) void augment_kernel(const float* __restrict__ data, const int* __restrict__ perm,
                                                              const int64_t* __restrict__ step,
                                                              const int* __restrict__ labels, float* __restrict__ xaug,
                                                              int* __restrict__ yaug, int B, int n, uint32_t seed,
                                                              uint32_t rank, AugmentConfig cfg) {
  __shared__ float tile[TS * TS];
  __shared__ __attribute__((aligned(16))) float fld[4 * FIELD];  // N_x, N_y (then S_x, S_y), T_x, T_y
  __shared__ float gl[32];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int64_t i = *step * (int64_t)B + b;
  const int row = perm[(int)(i % (int64_t)n)];
  f32x4 px = zero_f4();
  if (tid < CHUNKS) px = reinterpret_cast<const f32x4*>(data + (size_t)row * PIX)[tid];
  int label = 0;
  if (tid == 0) label = labels[row];

  const uint32_t lo = (uint32_t)i, hi = (uint32_t)((uint64_t)i >> 32);
  const bool elastic = cfg.elastic_alpha != 0.f;
  if (elastic) {
    if (tid < 32) gl[tid] = tid < kAugmentTaps ? cfg.g[tid] : 0.f;
    if (tid < CHUNKS) {
      float* dst = fld + (4 * tid / IMG) * FS + 4 * tid % IMG;
      const Philox4 nx = philox4x32_10(lo, hi, AUG_DRAW_NX + tid, rank, seed, kAugmentKey);
      *reinterpret_cast<f32x4*>(dst) = f32x4{sym(nx.v[0]), sym(nx.v[1]), sym(nx.v[2]), sym(nx.v[3])};
      const Philox4 ny = philox4x32_10(lo, hi, AUG_DRAW_NY + tid, rank, seed, kAugmentKey);
      *reinterpret_cast<f32x4*>(dst + FIELD) = f32x4{sym(ny.v[0]), sym(ny.v[1]), sym(ny.v[2]), sym(ny.v[3])};
    }
  }
  const Philox4 aff = philox4x32_10(lo, hi, AUG_DRAW_AFFINE, rank, seed, kAugmentKey);
  const float ty = cfg.shift_px * sym(aff.v[0]), tx = cfg.shift_px * sym(aff.v[1]);
  const float theta = cfg.rotate_rad * sym(aff.v[2]);
  const float inv = 1.f / (1.f + cfg.scale * sym(aff.v[3]));
  float sn, cs;
  sincosf(theta, &sn, &cs);

  // the border: rows 0 and 29, then columns 0 and 29 of rows 1..28
  if (tid < 2 * TS) tile[(tid / TS) * (TS - 1) * TS + tid % TS] = 0.f;
  else if (tid < 2 * TS + 2 * IMG) tile[((tid - 2 * TS) % IMG + 1) * TS + ((tid - 2 * TS) / IMG) * (TS - 1)] = 0.f;
  const int r = 4 * tid / IMG, c0 = 4 * tid % IMG;
  if (tid < CHUNKS) {
    float* t = tile + (r + 1) * TS + c0 + 1;
    t[0] = px[0]; t[1] = px[1]; t[2] = px[2]; t[3] = px[3];
  }
  __syncthreads();

  if (elastic) {
    const int lane = tid & 63, w = tid >> 6, f = w >> 1, ti = w & 1;
    float ga[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int gi = 16 * ti + (lane & 15), gj = 4 * ks + (lane >> 4);
      ga[ks] = (gi < IMG && gj < IMG) ? gl[gi > gj ? gi - gj : gj - gi] : 0.f;
    }
    smooth_pass<true>(fld + f * FIELD, fld + (2 + f) * FIELD, ga, 1.f, ti, lane);
    __syncthreads();
    smooth_pass<false>(fld + (2 + f) * FIELD, fld + f * FIELD, ga, cfg.elastic_alpha, ti, lane);
    __syncthreads();
  }
  if (tid >= CHUNKS) return;

  const float dy = (float)r - CTR;
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + j;
    const float dx = (float)c - CTR;
    float y = CTR + inv * (cs * dy - sn * dx) - ty;
    float x = CTR + inv * (sn * dy + cs * dx) - tx;
    if (elastic) {
      x += fld[r * FS + c];
      y += fld[FIELD + r * FS + c];
    }
    o[j] = bilinear(tile, y, x);
  }
  reinterpret_cast<f32x4*>(xaug + (size_t)b * PIX)[tid] = o;
  if (tid == 0) yaug[b] = label;
}

}  // namespace

AugmentConfig make_augment_config(double shift_px, double rotate_deg, double scale, double elastic_alpha,
                                  double elastic_sigma) {
  if (!(shift_px >= 0 && rotate_deg >= 0 && scale >= 0 && scale < 1 && elastic_alpha >= 0 && elastic_sigma >= 0))
    throw std::invalid_argument("augment: shift, rotate, alpha, sigma >= 0 and 0 <= scale < 1");
  if (elastic_alpha > 0 && !(elastic_sigma > 0)) throw std::invalid_argument("augment: elastic_alpha > 0 needs elastic_sigma > 0");
  AugmentConfig c{};
  c.shift_px = (float)shift_px;
  c.rotate_rad = (float)(rotate_deg * (3.14159265358979323846 / 180.0));
  c.scale = (float)scale;
  c.elastic_alpha = (float)elastic_alpha;
  c.elastic_sigma = (float)elastic_sigma;
  if (elastic_alpha > 0) {
    double e[kAugmentTaps], sum = 0.0;
    for (int d = 0; d < kAugmentTaps; ++d) {
      e[d] = std::exp(-(double)(d * d) / (2.0 * elastic_sigma * elastic_sigma));
      sum += d ? 2.0 * e[d] : e[d];
    }
    for (int d = 0; d < kAugmentTaps; ++d) c.g[d] = (float)(e[d] / sum);
  }
  return c;
}

void augment_batch(const AugmentArgs& a, hipStream_t s) {
  if (!a.data || !a.labels || !a.perm || !a.step || !a.xaug || !a.yaug)
    throw std::runtime_error("augment_batch: data, labels, perm, step, xaug and yaug");
  if (a.n < 1 || a.B < 1 || a.B > 65535) throw std::runtime_error("augment_batch: n >= 1 and 1 <= B <= 65535");
  if (((reinterpret_cast<uintptr_t>(a.data) | reinterpret_cast<uintptr_t>(a.xaug)) & 15) != 0)
    throw std::runtime_error("augment_batch: data and xaug must be 16-byte aligned");
  TFD_LAUNCH(augment_kernel<<<a.B, kAugThreads, 0, s>>>(a.data, a.perm, a.step, a.labels, a.xaug, a.yaug, a.B, a.n, a.seed,
                                                         a.rank, a.cfg));
}

}  // namespace tfd
