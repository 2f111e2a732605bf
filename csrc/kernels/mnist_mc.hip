// Monte-Carlo dropout head (csrc/mnist_mc.h): mc_head_kernel, T masked passes of the output layer per
// row as one [T x 1024] x [1024 x 10] product on the fp32 matrix core. A code object of its own: the
// step's and the inference head's kernels are not touched.
//
// By instruction count the tile loop is VALU work, not matrix-core work: a lane's 16 Philox calls per sample
// tile are about 1500 integer operations beside 64 MFMAs of 8 passes each. That count, not a counter, is why
// everything that does not depend on the sample tile lives in registers (hr / keep_prob: 64, the B fragments
// of W_out: 64) and the tile loop holds nothing but draws, selects and MFMAs; which unit bounds the kernel was
// not measured. LDS: hr 4 KiB, two partial-tile buffers 8.5 KiB (double buffered: one barrier per tile), the
// final merge 1.5 KiB.
#include "../common.h"
#include "../gemm_f32.h"
#include "../launch_check.h"
#include "../mnist_infer.h"
#include "../mnist_layout.h"
#include "../mnist_mc.h"

namespace tfd {
using namespace mnist;
namespace {

constexpr int kTile = kMcSampleTile;
constexpr int kPartRow = 17;           // 16 columns + 1: lane m reads row m, 17 m + c hits 16 banks
constexpr int kFin = 2 + 2 * NCLS;     // a sample lane's {count, sum H, mean[10], M2[10]}
constexpr int kFinRow = kFin + 1;

__global__ __launch_bounds__(256) void mc_head_kernel(McHeadArgs a) {
  __shared__ __attribute__((aligned(16))) float hr_s[HID];
  __shared__ float part[2][4][kTile][kPartRow];
  __shared__ float fin[kTile][kFinRow];
  __shared__ float pbar_s[NCLS];
  const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int m = lane & 15, kk = lane >> 4;  // m: the lane's sample of a tile (A) and its output column (B, C)
  // ---- prologue: infer_head_kernel's. Slabs in split order on the fc1 bias, relu; thread t owns units 4t..4t+3
  {
    const int n0 = 4 * t;
    f32x4 p[kInferMaxSplits];
#pragma unroll
    for (int s = 0; s < kInferMaxSplits; ++s)
      if (s < a.splits) p[s] = *reinterpret_cast<const f32x4*>(a.fc1_slab + ((size_t)s * a.split_rows + row) * HID + n0);
    f32x4 h = *reinterpret_cast<const f32x4*>(a.p32 + OFF_BD1 + n0);
#pragma unroll
    for (int s = 0; s < kInferMaxSplits; ++s)
      if (s < a.splits) h += p[s];
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = fmaxf(h[j], 0.f);
    *reinterpret_cast<f32x4*>(hr_s + n0) = h;
  }
  // ---- the lane's B fragments, straight from global / L2, once per block: W_out[4 g + j][m], g = 64 wv + 4 q + kk
  float bw[64];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int u0 = 256 * wv + 16 * q + 4 * kk;
#pragma unroll
    for (int j = 0; j < 4; ++j) bw[4 * q + j] = m < NCLS ? a.p32[OFF_OUT + (size_t)(u0 + j) * NCLS + m] : 0.f;
  }
  float bout[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) bout[c] = a.p32[OFF_BOUT + c];
  const int lbl = a.labels ? a.labels[row] : -1;
  __syncthreads();
  // ---- the lane's A values before the mask: hr * (1 / keep_prob), the training heads' product
  const float kp = a.keep_prob, inv_kp = 1.0f / kp;
  float ha[64];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(hr_s + 256 * wv + 16 * q + 4 * kk);
#pragma unroll
    for (int j = 0; j < 4; ++j) ha[4 * q + j] = v[j] * inv_kp;
  }
  const uint64_t grow = a.row0 + (uint64_t)row;
  const uint32_t rlo = (uint32_t)grow, rhi = (uint32_t)(grow >> 32);
  const int T = a.samples, tiles = (T + kTile - 1) / kTile;
  // statistics of sample lane m (used by threads 0..15)
  float cnt = 0.f, hsum = 0.f, mean[NCLS], m2[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) mean[c] = m2[c] = 0.f;

  for (int tile = 0; tile < tiles; ++tile) {
    const uint32_t c0 = ((uint32_t)(tile * kTile + m) << 8) + (uint32_t)(64 * wv + kk);
    f32x4 acc = zero_f4();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const Philox4 r = philox4x32_10(c0 + 4u * q, rlo, rhi, a.rank, a.seed, kMcDropoutKey);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = mfma16x16x4f32(u01(r.v[j]) < kp ? ha[4 * q + j] : 0.f, bw[4 * q + j], acc);
    }
    // C: rows (samples) 4 kk .. 4 kk + 3 of column m
    float(*pp)[kPartRow] = part[tile & 1][wv];
#pragma unroll
    for (int i = 0; i < 4; ++i) pp[4 * kk + i][m] = acc[i];
    __syncthreads();  // one per tile: buffer tile & 1 is written again two tiles on, behind the next barrier
    if (t < kTile) {
      float z[NCLS];
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        const float(*b)[kTile][kPartRow] = part[tile & 1];
        z[c] = ((b[0][m][c] + b[1][m][c]) + b[2][m][c]) + b[3][m][c] + bout[c];
        mx = fmaxf(mx, z[c]);
      }
      float e[NCLS], se = 0.f;
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        z[c] -= mx;
        e[c] = expf(z[c]);
        se += e[c];
      }
      const float inv = 1.0f / se;
      const float w = (tile * kTile + m < T) ? 1.f : 0.f;  // a sample past T weighs exactly 0
      cnt += w;
      const float wrn = w / fmaxf(cnt, 1.f);
      float pz = 0.f;
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        // p is ONE rounded value: contracted into its uses (the build's -ffp-contract=fast ignores pragmas) the
        // product would be rounded differently in each, and the two differences of an M2 term would lose their
        // common sign. The empty asm pins it in a register.
        float p = e[c] * inv;
        asm volatile("" : "+v"(p));
        pz += p * z[c];
        const float d = p - mean[c];
        mean[c] += d * wrn;
        m2[c] += w * (d * (p - mean[c]));
      }
      hsum += w * (logf(se) - pz);
    }
  }
  // ---- merge the 16 sample lanes in lane order
  if (t < kTile) {
    fin[m][0] = cnt;
    fin[m][1] = hsum;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      fin[m][2 + c] = mean[c];
      fin[m][2 + NCLS + c] = m2[c];
    }
  }
  __syncthreads();
  const float rT = 1.0f / (float)T;
  if (t < NCLS) {  // thread c: class c. Lane 0 always holds sample 0.
    float na = fin[0][0], mu = fin[0][2 + t], M = fin[0][2 + NCLS + t];
    for (int i = 1; i < kTile; ++i) {
      const float nb = fin[i][0], d = fin[i][2 + t] - mu, n = na + nb;
      const float f = nb / n;
      mu += d * f;
      M += fin[i][2 + NCLS + t] + (d * d) * (na * f);
      na = n;
    }
    pbar_s[t] = mu;
    a.mean_prob[(size_t)row * NCLS + t] = mu;
    a.var_prob[(size_t)row * NCLS + t] = M * rT;
  }
  __syncthreads();
  if (t != 0) return;
  float ent = 0.f, best = pbar_s[0], pl = 0.f, eh = 0.f;
  int am = 0;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float p = pbar_s[c];
    if (p > 0.f) ent -= p * logf(p);
    if (c > 0 && p > best) { best = p; am = c; }
    if (c == lbl) pl = p;
  }
  for (int i = 0; i < kTile; ++i) eh += fin[i][1];
  eh *= rT;
  a.classes[row] = am;
  a.entropy[row] = ent;
  if (a.expected_entropy) a.expected_entropy[row] = eh;
  a.mutual_info[row] = fmaxf(ent - eh, 0.f);
  if (a.labels) {
    a.loss_row[row] = -logf(pl);  // a label outside [0, 10): +inf
    a.correct_row[row] = (am == lbl) ? 1.f : 0.f;
  }
}

}  // namespace

void mc_head(const McHeadArgs& a, hipStream_t s) {
  if (a.rows < 1) throw std::runtime_error("mc_head: rows >= 1");
  if (a.splits < 1 || a.splits > kInferMaxSplits) throw std::runtime_error("mc_head: 1 <= splits <= kInferMaxSplits");
  if (a.split_rows < a.rows) throw std::runtime_error("mc_head: split_rows below rows");
  if (a.samples < 1 || a.samples > kMcMaxSamples) throw std::runtime_error("mc_head: 1 <= samples <= kMcMaxSamples (4096)");
  if (!(a.keep_prob > 0.f && a.keep_prob <= 1.f)) throw std::runtime_error("mc_head: 0 < keep_prob <= 1");
  if (!a.fc1_slab || !a.p32 || !a.mean_prob || !a.classes || !a.entropy || !a.mutual_info || !a.var_prob)
    throw std::runtime_error("mc_head: slabs, parameters, mean_prob, classes, entropy, mutual_info, var_prob");
  if (a.labels && (!a.loss_row || !a.correct_row)) throw std::runtime_error("mc_head: labels need loss_row and correct_row");
  if (((reinterpret_cast<uintptr_t>(a.fc1_slab) | reinterpret_cast<uintptr_t>(a.p32)) & 15) != 0)
    throw std::runtime_error("mc_head: slabs and parameters must be 16-byte aligned");
  TFD_LAUNCH(mc_head_kernel<<<a.rows, 256, 0, s>>>(a));
}

}  // namespace tfd
