// Input gradient + FGSM batch (csrc/mnist_input_grad.h): one 256-thread block (4 waves) per image, all of
// W2 resident in LDS (149.5 KB: one block per CU), every phase of the image inside the block.
//
//   stage     W2 [25 taps][32 ci][64 co] bf16 comes in by LDS-DMA (global_load_lds_dwordx4: no VGPR round
//             trip; one wave instruction = 8 rows, 25 per wave), chunk-swizzled on the SOURCE address as
//             conv2_bwd_lds stages it: 16-B chunk c of row r holds global chunk c ^ (r & 7), so the 16 rows
//             of a B-fragment read hit 16 distinct bank quads. Under the DMA the image's dz2 goes through
//             registers into a zero-bordered channel-chunk-major image [8 chunks][18 rows][20 cols] x 16 B
//             (planes padded to 368 slots = 23 x 256 B), and the x row, the label and the two W1 B-fragments
//             (straight from global memory: 16 B per lane, taps >= 25 zero) are requested.
//   conv2 dgrad  M-tile = one p1 row (16 lanes = iw 0..15, 14 stored: the lanes of an A fragment read 16
//             consecutive 16-B slots at (ih + 4 - kh, iw + 4 - kw)); wave w owns rows w, w + 4, w + 8, w + 12
//             (a row past 13 is row 13 again, not stored) and both N-tiles over all of K: per k-step (tap, co
//             half) 2 B + 4 A fragment reads feed 8 MFMAs, 32 accumulator registers.
//   relu/pool once every wave is out of the K loop the image and W2 are dead: dz1 [784][32] bf16 (chunk
//             c of pixel p at c ^ ((p >> 2) & 3): 16 consecutive pixels of an A fragment cover all banks
//             once) is zeroed over them, then each lane scatters its dp1 values, rounded to bf16, to their
//             window positions. idx1 is masked to 0..3, so no operand can place a store outside dz1.
//   tap GEMM  T [784][25] fp32 behind dz1: 49 M-tiles x 2 N-tiles, one MFMA each, A from dz1, B the W1
//             fragments held since the start. Row pitch 25 floats (odd): the gather's lanes, consecutive
//             pixels, read 64 distinct banks.
//   gather    thread o, o + 256, ...: dx[u][v] = sum over i, j ascending of the in-image T terms, into an LDS row.
//   epilogue  threads 0..195: four pixels each, 16-byte stores of dx and xadv; thread 0 the label.
// Plain stores only: no atomics, nothing to clear, the same bits every run.
#include "../mnist_input_grad.h"

#include <stdexcept>

#include "../common.h"
#include "../launch_check.h"
#include "../mnist_layout.h"

namespace tfd {
using namespace mnist;
namespace {

constexpr int IG_NT = 256;
constexpr int IG_COLS = 20, IG_ROWS = 18, IG_PLANE = 368;  // dz2 image: dz2[r][c] at slot (r + 2) * 20 + c + 2
constexpr int IG_WTAP = C1 * C2;                           // elements of one tap's [ci][co] rows
constexpr int IG_W_OFF = 8 * IG_PLANE * 16;                // 47,104
constexpr int IG_SMEM = IG_W_OFF + KTAPS * IG_WTAP * 2;    // 149,504
constexpr int IG_PIX = IMG * IMG;
constexpr int IG_T_OFF = IG_PIX * C1 * 2;                  // dz1 at 0 (50,176 B), then T
constexpr int IG_TP = 25;
constexpr int IG_DX_OFF = IG_T_OFF + IG_PIX * IG_TP * 4;   // 128,576: the gathered dx row
static_assert(IG_SMEM <= 160 * 1024 && IG_PLANE >= IG_ROWS * IG_COLS && IG_PLANE * 16 % 256 == 0, "LDS carve");
static_assert(IG_DX_OFF + IG_PIX * 4 <= IG_SMEM && IG_T_OFF % 16 == 0 && IG_DX_OFF % 16 == 0, "LDS reuse after the K loop");
static_assert(IG_WTAP / 512 == IG_NT / 64, "one DMA instruction per wave and tap");

__device__ __forceinline__ int ig_dz1(int px, int c) {  // element offset of dz1[px][c]
  return px * C1 + (((c >> 3) ^ ((px >> 2) & 3)) << 3) + (c & 7);
}

__global__ __launch_bounds__(IG_NT) void input_grad_kernel(const uint16_t* __restrict__ dz2, const uint16_t* __restrict__ p1,
                                                           const uint8_t* __restrict__ idx1, const uint16_t* __restrict__ pbf,
                                                           const float* __restrict__ data, const int* __restrict__ labels,
                                                           const int* __restrict__ perm, const int64_t* __restrict__ step,
                                                           int n, int B, float eps, int adv_rows, float* __restrict__ dx,
                                                           float* __restrict__ xadv, int* __restrict__ yadv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* img = reinterpret_cast<bf16*>(smem);
  bf16* wt = reinterpret_cast<bf16*>(smem + IG_W_OFF);
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, w = t >> 6, g = lane >> 4, l16 = lane & 15;
  {
    const uint16_t* wsrc = pbf + OFF_WC2;
    const int rr = t >> 3, sl = t & 7;  // wave w: rows 8 w .. 8 w + 7 of every tap
#pragma unroll
    for (int tap = 0; tap < KTAPS; ++tap)
      __builtin_amdgcn_global_load_lds((const void*)(wsrc + tap * IG_WTAP + rr * 64 + ((sl ^ (rr & 7)) << 3)),
                                       (__attribute__((address_space(3))) void*)(wt + tap * IG_WTAP + w * 512), 16, 0, 0);
  }
  int row = b;
  if (perm) row = perm[(int)((*step * (int64_t)B + b) % (int64_t)n)];
  f32x4 xv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (t < IG_PIX / 4) xv = reinterpret_cast<const f32x4*>(data + (size_t)row * IG_PIX)[t];
  int label = 0;
  if (t == 0 && yadv) label = labels[row];
  bf16x8 w1f[2];  // B[k = c][n = tap] = W1[tap][c]: 8 consecutive channels of one tap
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int tap = 16 * nt + l16;
#pragma unroll
    for (int e = 0; e < 8; ++e) w1f[nt][e] = (bf16)0.0f;
    if (tap < KTAPS) w1f[nt] = *reinterpret_cast<const bf16x8*>(pbf + OFF_WC1 + tap * C1 + 8 * g);
  }
  {
    const uint16_t* src = dz2 + (size_t)b * 196 * C2;
    constexpr int NI = (8 * IG_PLANE + IG_NT - 1) / IG_NT;  // 12 slots per thread, the last half used
    uint4 vi[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int i = t + IG_NT * j, ch = i / IG_PLANE, px = i - ch * IG_PLANE;
      const int r = px / IG_COLS - 2, c = px % IG_COLS - 2;
      vi[j] = make_uint4(0u, 0u, 0u, 0u);
      if (i < 8 * IG_PLANE && px < IG_ROWS * IG_COLS && (unsigned)r < 14u && (unsigned)c < 14u)
        vi[j] = *reinterpret_cast<const uint4*>(src + (r * 14 + c) * C2 + ch * 8);
    }
#pragma unroll
    for (int j = 0; j < NI; ++j)
      if (t + IG_NT * j < 8 * IG_PLANE) *reinterpret_cast<uint4*>(img + (t + IG_NT * j) * 8) = vi[j];
  }
  // LDS-DMA is outside the compiler's wait insertion: this wave's have landed, the barrier says every wave's
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- conv2 dgrad ----
  f32x4 acc[4][2];
  int ih[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ih[j] = min(w + 4 * j, 13);
    acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  {
    const bf16* ab = img + (g * IG_PLANE + l16 + 4) * 8;
    const bf16* bb = wt + l16 * 64;
    const int sw0 = (g ^ (l16 & 7)) << 3, sw1 = ((g + 4) ^ (l16 & 7)) << 3;
#pragma unroll
    for (int tap = 0; tap < KTAPS; ++tap) {
      const int kh = tap / 5, kw = tap - 5 * kh;
#pragma unroll
      for (int sk = 0; sk < 2; ++sk) {
        const bf16* br = bb + tap * IG_WTAP + (sk ? sw1 : sw0);
        const bf16x8 fb0 = *reinterpret_cast<const bf16x8*>(br);
        const bf16x8 fb1 = *reinterpret_cast<const bf16x8*>(br + 16 * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8 fa = *reinterpret_cast<const bf16x8*>(ab + ((ih[j] + 4 - kh) * IG_COLS - kw + sk * 4 * IG_PLANE) * 8);
          acc[j][0] = mfma16x16x32(fa, fb0, acc[j][0]);
          acc[j][1] = mfma16x16x32(fa, fb1, acc[j][1]);
        }
      }
    }
  }
  // the relu values and window positions of this lane's dp1 values, requested in front of the barrier
  uint16_t pv[4][2][4];
  uint8_t iv[4][2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t o = ((size_t)b * 196 + ih[j] * 14 + min(4 * g + r, 13)) * C1 + 16 * nt + l16;
        pv[j][nt][r] = p1[o];
        iv[j][nt][r] = idx1[o];
      }
  __syncthreads();  // every wave is out of the K loop: the image and W2 become dz1, T and the dx row
  for (int i = t; i < IG_T_OFF / 16; i += IG_NT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  // ---- relu + pool-1 backward ----
  uint16_t* dz1 = reinterpret_cast<uint16_t*>(smem);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (w + 4 * j > 13) break;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = 4 * g + r, wi = iv[j][nt][r] & 3;
        if (x < 14) {
          const int px = (2 * ih[j] + (wi >> 1)) * IMG + 2 * x + (wi & 1);
          dz1[ig_dz1(px, 16 * nt + l16)] = pv[j][nt][r] != 0 ? f2bf_bits(acc[j][nt][r]) : (uint16_t)0;
        }
      }
  }
  __syncthreads();

  // ---- conv1 dgrad: the tap GEMM ----
  float* T = reinterpret_cast<float*>(smem + IG_T_OFF);
  for (int m = w; m < IG_PIX / 16; m += 4) {
    const int p = 16 * m + l16;
    const bf16x8 fa = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16*>(dz1) + ig_dz1(p, 8 * g));
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const f32x4 c = mfma16x16x32(fa, w1f[nt], f32x4{0.f, 0.f, 0.f, 0.f});
      const int tap = 16 * nt + l16;
      if (tap < KTAPS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(16 * m + 4 * g + r) * IG_TP + tap] = c[r];
      }
    }
  }
  __syncthreads();

  // ---- ... and the gather ----
  float* dxs = reinterpret_cast<float*>(smem + IG_DX_OFF);
  for (int o = t; o < IG_PIX; o += IG_NT) {
    const int u = o / IMG, v = o - IMG * u;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int r = u - i + 2;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int c = v - j + 2;
        if ((unsigned)r < (unsigned)IMG && (unsigned)c < (unsigned)IMG) s += T[(r * IMG + c) * IG_TP + 5 * i + j];
      }
    }
    dxs[o] = s;
  }
  __syncthreads();

  // ---- epilogue ----
  if (t < IG_PIX / 4) {
    const f32x4 d = reinterpret_cast<const f32x4*>(dxs)[t];
    if (dx) reinterpret_cast<f32x4*>(dx + (size_t)b * IG_PIX)[t] = d;
    if (xadv) {
      const float e = b < adv_rows ? eps : 0.f;
      f32x4 o = xv;  // eps_b == 0: the row itself, bit for bit
      if (e != 0.f) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float sg = (float)((d[k] > 0.f) - (d[k] < 0.f));
          o[k] = fminf(fmaxf(xv[k] + e * sg, 0.f), 1.f);
        }
      }
      reinterpret_cast<f32x4*>(xadv + (size_t)b * IG_PIX)[t] = o;
    }
  }
  if (t == 0 && yadv) yadv[b] = label;
}

}  // namespace

void input_grad_prepare() {
  static bool done = false;
  if (done) return;
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(input_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             IG_SMEM));
  done = true;
}

void input_grad(const InputGradArgs& a, hipStream_t s) {
  if (!a.dz2 || !a.p1 || !a.idx1 || !a.pbf || !a.data) throw std::runtime_error("input_grad: dz2, p1, idx1, pbf and data");
  if ((a.perm && !a.step) || (a.xadv && (!a.yadv || !a.labels)) || (!a.xadv && a.yadv))
    throw std::runtime_error("input_grad: perm needs step; xadv, yadv and labels go together");
  if (a.n < 1 || a.B < 1 || a.B > 65535) throw std::runtime_error("input_grad: n >= 1 and 1 <= B <= 65535");
  if (!(a.eps >= 0.f)) throw std::runtime_error("input_grad: eps >= 0");
  const uintptr_t al = reinterpret_cast<uintptr_t>(a.dz2) | reinterpret_cast<uintptr_t>(a.pbf) | reinterpret_cast<uintptr_t>(a.data) |
                       reinterpret_cast<uintptr_t>(a.dx) | reinterpret_cast<uintptr_t>(a.xadv);
  if ((al & 15) != 0) throw std::runtime_error("input_grad: dz2, pbf, data, dx and xadv must be 16-byte aligned");
  input_grad_prepare();
  TFD_LAUNCH(input_grad_kernel<<<a.B, IG_NT, IG_SMEM, s>>>(a.dz2, a.p1, a.idx1, a.pbf, a.data, a.labels, a.perm, a.step, a.n,
                                                           a.B, a.eps, a.adv_rows, a.dx, a.xadv, a.yadv));
}

}  // namespace tfd
