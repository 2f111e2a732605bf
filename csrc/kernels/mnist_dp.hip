// DP-SGD kernels (csrc/mnist_dp.h). dp_norm_kernel: one 256-thread block (4 waves) per image; nothing of a
// per-example weight gradient is ever stored: the GEMM accumulators are squared and summed in registers.
//
//   A  stage + conv2 dgrad + relu / pool-1 backward, as input_grad_kernel runs them (the same operand
//      layouts, the same bf16 rounding point): W2 resident by LDS-DMA, dz2 in a zero-bordered chunk-major
//      image, v_mfma_f32_16x16x32_bf16, dp1 in 32 accumulator registers per lane. Beside the staging the
//      four fc row reductions (p2, dh, hd, dlogits) run from 16-byte global loads.
//   B  conv1 weight gradient. K runs over conv1 output pixels, so both operands are position-major:
//      dz1T [32 c][28 rows][32 cols] bf16 (cols 28..31 zero; channel pitch 904 so the 16 channels of a B
//      fragment read hit distinct banks), scattered from the accumulators over the dead dz2 image / W2, and
//      five column-shifted copies xs[kw][32 rows][32 cols] of the zero-bordered bf16 x image, so the A
//      fragment of tap (kh, kw) at output row oh is ONE aligned 16-byte read of xs[kw][oh + kh][8 g ..]
//      (conv2_bwd_lds's tail lays its x out the same way). M = 25 -> 32 taps, N = 32, K = 28 x 32: wave w
//      owns tile (w & 1, w >> 1), 28 MFMAs. The bias: thread (c, part) sums dz1T[c] rows part, part + 8, ...
//   C  conv2 weight gradient. M = 800 (tap, ci), N = 64, K = 14 rows x 16 cols = 224 (cols 14, 15 zero in
//      dz2T [64 co][224], pitch 232): five column-shifted copies p1s[kw][32 ci][18 rows][16 cols] (pitch
//      296) of the zero-bordered p1 image give every A fragment as one aligned 16-byte read. Wave w holds
//      the 14 B fragments of N-tiles 2 (w & 1), + 1 in registers for the whole phase and walks M-tiles
//      (w >> 1) + 2 i: 7 A reads feed 14 MFMAs. The bias: thread (co, quarter) sums 56 dz2T slots.
//   D  eight partial sums per thread -> wave sums by shuffles -> LDS -> every thread adds the four waves' in
//      wave order: a fixed order, no atomics, nothing to clear. Then the optional in-place scaling.
// dp_noise_kernel: one thread per 4 elements, one Philox call, 16-byte load and store.
#include "../mnist_dp.h"

#include <atomic>
#include <stdexcept>

#include "../common.h"
#include "../launch_check.h"
#include "../mnist_layout.h"

namespace tfd {
using namespace mnist;
namespace {

constexpr int DP_NT = 256;
// phase A (input_grad_kernel's carve)
constexpr int DP_COLS = 20, DP_ROWS = 18, DP_PLANE = 368;  // dz2 image: dz2[r][c] at slot (r + 2) * 20 + c + 2
constexpr int DP_WTAP = C1 * C2;
constexpr int DP_W_OFF = 8 * DP_PLANE * 16;                // 47,104
constexpr int DP_SMEM = DP_W_OFF + KTAPS * DP_WTAP * 2;    // 149,504
constexpr int DP_PIX = IMG * IMG;
// phase B
constexpr int DP_ZP = IMG * 32 + 8;                        // dz1T channel pitch, elements
constexpr int DP_XS_OFF = C1 * DP_ZP * 2;                  // 57,856
constexpr int DP_B_END = DP_XS_OFF + 5 * 32 * 32 * 2;      // 68,096
// phase C
constexpr int DP_PP = DP_ROWS * 16 + 8;                    // p1s (kw, ci) pitch, elements: 296
constexpr int DP_DZ_OFF = 5 * C1 * DP_PP * 2;              // 94,720
constexpr int DP_DP = P1H * 16 + 8;                        // dz2T channel pitch, elements: 232
constexpr int DP_C_END = DP_DZ_OFF + C2 * DP_DP * 2;       // 124,416
constexpr int DP_RED_OFF = DP_SMEM - 4 * 8 * 4;            // the wave sums, behind everything
static_assert(DP_SMEM <= 160 * 1024 && DP_PLANE >= DP_ROWS * DP_COLS && DP_PLANE * 16 % 256 == 0, "LDS carve");
static_assert(DP_WTAP / 512 == DP_NT / 64, "one DMA instruction per wave and tap");
static_assert(DP_B_END % 16 == 0 && DP_XS_OFF % 16 == 0 && DP_ZP * 2 % 16 == 0 && DP_B_END <= DP_RED_OFF, "phase B carve");
static_assert(DP_C_END % 16 == 0 && DP_DZ_OFF % 16 == 0 && DP_PP * 2 % 16 == 0 && DP_DP * 2 % 16 == 0 && DP_C_END <= DP_RED_OFF,
              "phase C carve");

__device__ __forceinline__ float sumsq_bf8(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float lo = __uint_as_float(w[k] << 16), hi = __uint_as_float(w[k] & 0xFFFF0000u);
    s += lo * lo;
    s += hi * hi;
  }
  return s;
}
__device__ __forceinline__ uint4 scale_bf8(const uint4& v, float c) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    o[k] = pack_bf2(__fmul_rn(c, __uint_as_float(w[k] << 16)), __fmul_rn(c, __uint_as_float(w[k] & 0xFFFF0000u)));
  return make_uint4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ void zero_lds(char* smem, int bytes, int t) {
  for (int i = t; i < bytes / 16; i += DP_NT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(DP_NT) void dp_norm_kernel(DpNormArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* img = reinterpret_cast<bf16*>(smem);
  bf16* wt = reinterpret_cast<bf16*>(smem + DP_W_OFF);
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, w = t >> 6, g = lane >> 4, l16 = lane & 15;
  uint16_t* dz2 = a.dz2 + (size_t)b * 196 * C2;
  {
    const uint16_t* wsrc = a.pbf + OFF_WC2;
    const int rr = t >> 3, sl = t & 7;  // wave w: rows 8 w .. 8 w + 7 of every tap
#pragma unroll
    for (int tap = 0; tap < KTAPS; ++tap)
      __builtin_amdgcn_global_load_lds((const void*)(wsrc + tap * DP_WTAP + rr * 64 + ((sl ^ (rr & 7)) << 3)),
                                       (__attribute__((address_space(3))) void*)(wt + tap * DP_WTAP + w * 512), 16, 0, 0);
  }
  int row = b;
  if (a.perm) row = a.perm[(int)((*a.step * (int64_t)a.B + b) % (int64_t)a.n)];
  f32x4 xv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (t < DP_PIX / 4) xv = reinterpret_cast<const f32x4*>(a.data + (size_t)row * DP_PIX)[t];
  // part[k]: this thread's share of the eight sums (conv1 W, b; conv2 W, b; then ||p2||^2, ||dh||^2, ||hd||^2, ||dlogits||^2)
  float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  {
    const uint4* p2r = reinterpret_cast<const uint4*>(a.p2 + (size_t)b * FEAT);
    part[4] = sumsq_bf8(p2r[t]);
    if (t + DP_NT < FEAT / 8) part[4] += sumsq_bf8(p2r[t + DP_NT]);
    if (t < HID / 8) part[5] = sumsq_bf8(reinterpret_cast<const uint4*>(a.dh + (size_t)b * HID)[t]);
    else part[6] = sumsq_bf8(reinterpret_cast<const uint4*>(a.hd + (size_t)b * HID)[t - HID / 8]);
    if (t < NCLS) {
      const float d = a.dlogits[(size_t)b * NCLS + t];
      part[7] = d * d;
    }
  }
  {
    constexpr int NI = (8 * DP_PLANE + DP_NT - 1) / DP_NT;  // 12 slots per thread, the last half used
    uint4 vi[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int i = t + DP_NT * j, ch = i / DP_PLANE, px = i - ch * DP_PLANE;
      const int r = px / DP_COLS - 2, c = px % DP_COLS - 2;
      vi[j] = make_uint4(0u, 0u, 0u, 0u);
      if (i < 8 * DP_PLANE && px < DP_ROWS * DP_COLS && (unsigned)r < 14u && (unsigned)c < 14u)
        vi[j] = *reinterpret_cast<const uint4*>(dz2 + (r * 14 + c) * C2 + ch * 8);
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
      if (t + DP_NT * j < 8 * DP_PLANE) *reinterpret_cast<uint4*>(img + (t + DP_NT * j) * 8) = vi[j];
  }
  // LDS-DMA is outside the compiler's wait insertion: this wave's have landed, the barrier says every wave's
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- A: conv2 dgrad ----
  f32x4 acc[4][2];
  int ih[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ih[j] = min(w + 4 * j, 13);
    acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  {
    const bf16* ab = img + (g * DP_PLANE + l16 + 4) * 8;
    const bf16* bb = wt + l16 * 64;
    const int sw0 = (g ^ (l16 & 7)) << 3, sw1 = ((g + 4) ^ (l16 & 7)) << 3;
#pragma unroll
    for (int tap = 0; tap < KTAPS; ++tap) {
      const int kh = tap / 5, kw = tap - 5 * kh;
#pragma unroll
      for (int sk = 0; sk < 2; ++sk) {
        const bf16* br = bb + tap * DP_WTAP + (sk ? sw1 : sw0);
        const bf16x8 fb0 = *reinterpret_cast<const bf16x8*>(br);
        const bf16x8 fb1 = *reinterpret_cast<const bf16x8*>(br + 16 * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8 fa = *reinterpret_cast<const bf16x8*>(ab + ((ih[j] + 4 - kh) * DP_COLS - kw + sk * 4 * DP_PLANE) * 8);
          acc[j][0] = mfma16x16x32(fa, fb0, acc[j][0]);
          acc[j][1] = mfma16x16x32(fa, fb1, acc[j][1]);
        }
      }
    }
  }
  uint16_t pv[4][2][4];
  uint8_t iv[4][2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t o = ((size_t)b * 196 + ih[j] * 14 + min(4 * g + r, 13)) * C1 + 16 * nt + l16;
        pv[j][nt][r] = a.p1[o];
        iv[j][nt][r] = a.idx1[o];
      }
  __syncthreads();  // every wave is out of the K loop: the image and W2 become dz1T and the x copies
  zero_lds(smem, DP_B_END, t);
  __syncthreads();

  // ---- A: relu + pool-1 backward into dz1T; the five shifted bf16 x copies ----
  uint16_t* dz1 = reinterpret_cast<uint16_t*>(smem);
  uint16_t* xs = reinterpret_cast<uint16_t*>(smem + DP_XS_OFF);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (w + 4 * j > 13) break;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = 4 * g + r, wi = iv[j][nt][r] & 3;
        if (x < 14)
          dz1[(16 * nt + l16) * DP_ZP + (2 * ih[j] + (wi >> 1)) * 32 + 2 * x + (wi & 1)] =
              pv[j][nt][r] != 0 ? f2bf_bits(acc[j][nt][r]) : (uint16_t)0;
      }
  }
  if (t < DP_PIX / 4) {
    const int r = (4 * t) / IMG, c0 = 4 * t - IMG * r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint16_t xb = f2bf_bits(xv[k]);
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const int c = c0 + k + 2 - kw;  // xs[kw][r'][c] = xpad[r'][c + kw], xpad[r + 2][col + 2] = x[r][col]
        if (c >= 0) xs[(kw * 32 + r + 2) * 32 + c] = xb;
      }
    }
  }
  __syncthreads();

  // ---- B: conv1 weight gradient and bias ----
  {
    const int mt = w & 1, nt = w >> 1, tap = 16 * mt + l16;
    const bool live = tap < KTAPS;
    const int kh = live ? tap / 5 : 0, kw = live ? tap - 5 * (tap / 5) : 0;
    const bf16* ar = reinterpret_cast<const bf16*>(xs) + (kw * 32 + kh) * 32 + 8 * g;
    const bf16* br = reinterpret_cast<const bf16*>(dz1) + (16 * nt + l16) * DP_ZP + 8 * g;
    bf16x8 zero;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero[e] = (bf16)0.0f;
    f32x4 c1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int oh = 0; oh < IMG; ++oh) {
      bf16x8 fa = *reinterpret_cast<const bf16x8*>(ar + oh * 32);
      if (!live) fa = zero;
      c1 = mfma16x16x32(fa, *reinterpret_cast<const bf16x8*>(br + oh * 32), c1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[0] += c1[r] * c1[r];
    const int c = t >> 3, q = t & 7;
    float s = 0.f;
    for (int oh = q; oh < IMG; oh += 8)
      for (int x = 0; x < IMG; ++x) s += bf2f(dz1[c * DP_ZP + oh * 32 + x]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (q == 0) part[1] = s * s;
  }
  // the operands of phase C, requested in front of the barrier
  uint4 pq[4], zq[7];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = t + DP_NT * j;
    pq[j] = make_uint4(0u, 0u, 0u, 0u);
    if (i < 196 * 4) pq[j] = *reinterpret_cast<const uint4*>(a.p1 + (size_t)b * 196 * C1 + i * 8);
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int i = t + DP_NT * j;
    zq[j] = make_uint4(0u, 0u, 0u, 0u);
    if (i < 196 * 8) zq[j] = *reinterpret_cast<const uint4*>(dz2 + i * 8);
  }
  __syncthreads();  // every wave is out of phase B
  zero_lds(smem, DP_C_END, t);
  __syncthreads();

  // ---- C: stage p1s[kw][ci][r][c] = p1pad[r][c + kw][ci] and dz2T[co][oh * 16 + ow] ----
  // Not optimised: a channel-major to position-major transpose by 2-byte LDS stores (160 + 56 per thread) behind a
  // clear of all 124 KB, although only the border rows, the pad columns and the shifted-out columns need the zeros.
  // This staging is the likeliest home of the ~10 us the kernel takes over input_grad_kernel; packing two positions
  // per store, or transposing through registers, is the first thing to try.
  uint16_t* p1s = reinterpret_cast<uint16_t*>(smem);
  uint16_t* dzt = reinterpret_cast<uint16_t*>(smem + DP_DZ_OFF);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = t + DP_NT * j, pos = i >> 2, ch = i & 3, ph = pos / 14, pw = pos - 14 * ph;
    if (i < 196 * 4) {
      const uint32_t wd[4] = {pq[j].x, pq[j].y, pq[j].z, pq[j].w};
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const int c = pw + 2 - kw;  // 0 <= c <= 15 always holds at the top: pw <= 13
        if (c >= 0) {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            p1s[(kw * C1 + ch * 8 + e) * DP_PP + (ph + 2) * 16 + c] = (uint16_t)(wd[e >> 1] >> (16 * (e & 1)));
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int i = t + DP_NT * j, pos = i >> 3, ch = i & 7, oh = pos / 14, ow = pos - 14 * oh;
    if (i < 196 * 8) {
      const uint32_t wd[4] = {zq[j].x, zq[j].y, zq[j].z, zq[j].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) dzt[(ch * 8 + e) * DP_DP + oh * 16 + ow] = (uint16_t)(wd[e >> 1] >> (16 * (e & 1)));
    }
  }
  __syncthreads();

  // ---- C: conv2 weight gradient and bias ----
  {
    const int nh = w & 1;
    bf16x8 fb[2][7];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int ks = 0; ks < 7; ++ks)
        fb[n][ks] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16*>(dzt) + (16 * (2 * nh + n) + l16) * DP_DP + ks * 32 + 8 * g);
    float s2 = 0.f;
    for (int m = w >> 1; m < 2 * KTAPS; m += 2) {
      const int tap = m >> 1, kh = tap / 5, kw = tap - 5 * kh, ci = 16 * (m & 1) + l16;
      const bf16* ar = reinterpret_cast<const bf16*>(p1s) + (kw * C1 + ci) * DP_PP + ((g >> 1) + kh) * 16 + 8 * (g & 1);
      f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
      for (int ks = 0; ks < 7; ++ks) {
        const bf16x8 fa = *reinterpret_cast<const bf16x8*>(ar + ks * 32);
        c0 = mfma16x16x32(fa, fb[0][ks], c0);
        c1 = mfma16x16x32(fa, fb[1][ks], c1);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s2 += c0[r] * c0[r] + c1[r] * c1[r];
    }
    part[2] = s2;
    const int co = t >> 2, q = t & 3;
    float s = 0.f;
    for (int k = 0; k < 56; ++k) s += bf2f(dzt[co * DP_DP + q * 56 + k]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (q == 0) part[3] = s * s;
  }

  // ---- D: the eight sums, norm and clip factor ----
  float* red = reinterpret_cast<float*>(smem + DP_RED_OFF);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = wave_sum(part[k]);
    if (lane == 0) red[w * 8 + k] = v;
  }
  __syncthreads();
  float tot[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) tot[k] = ((red[k] + red[8 + k]) + red[16 + k]) + red[24 + k];
  const float bb = (float)a.B * (float)a.B;
  const float sq[8] = {tot[0] * bb, tot[1] * bb, tot[2] * bb, tot[3] * bb, tot[4] * tot[5] * bb, tot[5] * bb, tot[6] * tot[7] * bb,
                       tot[7] * bb};
  float n2 = sq[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) n2 += sq[k];
  const float nrm = sqrtf(n2);
  const float c = nrm > a.clip ? a.clip / nrm : 1.0f;
  if (t < 8) a.sq[(size_t)b * 8 + t] = sq[t];
  if (t == 8) a.norm[b] = nrm;
  if (t == 9) a.c[b] = c;
  if (!a.scale || c == 1.0f) return;
  if (t < NCLS) a.dlogits[(size_t)b * NCLS + t] = __fmul_rn(c, a.dlogits[(size_t)b * NCLS + t]);
  if (t < HID / 8) {
    uint4* p = reinterpret_cast<uint4*>(a.dh + (size_t)b * HID) + t;
    *p = scale_bf8(*p, c);
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int i = t + DP_NT * j;
    if (i < 196 * 8) {
      uint4* p = reinterpret_cast<uint4*>(dz2) + i;
      *p = scale_bf8(*p, c);
    }
  }
}

constexpr int DPN_NT = 256;

__global__ __launch_bounds__(DPN_NT) void dp_noise_kernel(DpNoiseArgs a) {
  const int64_t q = (int64_t)blockIdx.x * DPN_NT + threadIdx.x, j0 = 4 * q;
  if (j0 >= a.n) return;
  bool in[4] = {false, false, false, false};
  for (int r = 0; r < a.nreg; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) in[e] = in[e] || (j0 + e >= a.beg[r] && j0 + e < a.end[r]);
  if (!(in[0] || in[1] || in[2] || in[3])) return;
  const int64_t st = *a.step;
  const Philox4 p = philox4x32_10((uint32_t)q, (uint32_t)st, (uint32_t)(st >> 32), 0u, a.seed, kDpNoiseKey);
  float z[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float r = sqrtf(-2.0f * logf(1.0f - u01(p.v[2 * h])));
    float sn, cs;
    sincospif(2.0f * u01(p.v[2 * h + 1]), &sn, &cs);
    z[2 * h] = __fmul_rn(r, cs);
    z[2 * h + 1] = __fmul_rn(r, sn);
  }
  f32x4* gp = reinterpret_cast<f32x4*>(a.grad + j0);
  f32x4 gv = *gp;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (in[e]) gv[e] = __builtin_fmaf(a.amp, z[e], gv[e]);
  *gp = gv;
}

}  // namespace

void dp_norm_prepare() {
  static std::atomic<bool> done[64];  // the attribute is per device: once for each the process launches on
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && done[dev].load()) return;
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(dp_norm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DP_SMEM));
  if (dev >= 0 && dev < 64) done[dev].store(true);
}

void dp_norm(const DpNormArgs& a, hipStream_t s) {
  if (!a.data || !a.p1 || !a.idx1 || !a.dz2 || !a.p2 || !a.hd || !a.dh || !a.dlogits || !a.pbf || !a.sq || !a.norm || !a.c)
    throw std::runtime_error("dp_norm: every factor and every output");
  if (a.perm && !a.step) throw std::runtime_error("dp_norm: perm needs step");
  if (a.n < 1 || a.B < 1 || a.B > 65535) throw std::runtime_error("dp_norm: n >= 1 and 1 <= B <= 65535");
  if (!(a.clip > 0.f)) throw std::runtime_error("dp_norm: clip > 0");
  const uintptr_t al = reinterpret_cast<uintptr_t>(a.data) | reinterpret_cast<uintptr_t>(a.p1) | reinterpret_cast<uintptr_t>(a.dz2) |
                       reinterpret_cast<uintptr_t>(a.p2) | reinterpret_cast<uintptr_t>(a.hd) | reinterpret_cast<uintptr_t>(a.dh) |
                       reinterpret_cast<uintptr_t>(a.pbf);
  if ((al & 15) != 0) throw std::runtime_error("dp_norm: data, p1, dz2, p2, hd, dh and pbf must be 16-byte aligned");
  dp_norm_prepare();
  TFD_LAUNCH(dp_norm_kernel<<<a.B, DP_NT, DP_SMEM, s>>>(a));
}

void dp_noise(const DpNoiseArgs& a, hipStream_t s) {
  if (!a.grad || !a.step) throw std::runtime_error("dp_noise: grad and step");
  if (a.n < 4 || a.n % 4 != 0 || a.n / 4 > 0x7FFFFFFFLL || (reinterpret_cast<uintptr_t>(a.grad) & 15) != 0)
    throw std::runtime_error("dp_noise: n a multiple of 4 below 2^33, grad 16-byte aligned");
  if (a.nreg < 1 || a.nreg > 8) throw std::runtime_error("dp_noise: 1 to 8 regions");
  for (int r = 0; r < a.nreg; ++r)
    if (a.beg[r] < 0 || a.end[r] < a.beg[r] || a.end[r] > a.n) throw std::runtime_error("dp_noise: a region outside [0, n)");
  const int64_t blocks = (a.n / 4 + DPN_NT - 1) / DPN_NT;
  TFD_LAUNCH(dp_noise_kernel<<<(unsigned)blocks, DPN_NT, 0, s>>>(a));
}

}  // namespace tfd
