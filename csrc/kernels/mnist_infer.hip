// Device inference (csrc/mnist_infer.h): infer_head_kernel, the output layer of the MNIST CNN as a
// head that stores its logits and classes, and eval_reduce_kernel, the fold of one chunk's rows into
// an evaluation record. A code object of its own: the step's kernels are not touched. Both kernels
// are latency-bound (a head block reads 7 x 16 B of slab and 160 B of output weights per thread; the
// reduce reads at most 16 B per row); plain vector stores, no atomics, nothing to zero.
#include "../common.h"
#include "../launch_check.h"
#include "../mnist_infer.h"
#include "../mnist_layout.h"

namespace tfd {
using namespace mnist;
namespace {

// ---------------- the inference head ----------------
// One 256-thread block per row; thread t owns hidden units 4t..4t+3 (head_kernel's and f32_head's map).
template <bool FAST>
__global__ __launch_bounds__(256) void infer_head_kernel(InferHeadArgs a) {
  const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n0 = 4 * t;
  // the label-independent operands first, in one memory round trip (the training heads' order): the
  // slabs, this thread's 4 x 10 output-layer weights, the output bias and the fc1 bias; then the label,
  // a uniform address: a scalar load beside them
  f32x4 p[kInferMaxSplits];
#pragma unroll
  for (int s = 0; s < kInferMaxSplits; ++s)
    if (s < a.splits) p[s] = *reinterpret_cast<const f32x4*>(a.fc1_slab + ((size_t)s * a.split_rows + row) * HID + n0);
  f32x4 wo[NCLS];
#pragma unroll
  for (int q = 0; q < NCLS; ++q) wo[q] = reinterpret_cast<const f32x4*>(a.p32 + OFF_OUT + (size_t)n0 * NCLS)[q];
#define INFER_W(j, c) wo[((j) * NCLS + (c)) >> 2][((j) * NCLS + (c)) & 3]
  float bout[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) bout[c] = a.p32[OFF_BOUT + c];
  f32x4 h = *reinterpret_cast<const f32x4*>(a.p32 + OFF_BD1 + n0);
  const int lbl = a.labels ? a.labels[row] : -1;
#pragma unroll
  for (int s = 0; s < kInferMaxSplits; ++s)
    if (s < a.splits) h += p[s];
  float hd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) hd[j] = fmaxf(h[j], 0.f);  // keep_prob 1: the heads' scale is exactly 1
  float lp[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) lp[c] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < NCLS; ++c) lp[c] = fmaf(hd[j], INFER_W(j, c), lp[c]);
  }
#undef INFER_W
  __shared__ float red[4][NCLS];
  wave_sums_to_lane63(lp);
  if (lane == 63) {
#pragma unroll
    for (int c = 0; c < NCLS; ++c) red[wv][c] = lp[c];
  }
  __syncthreads();
  float logit[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) logit[c] = red[0][c] + red[1][c] + red[2][c] + red[3][c] + bout[c];
  float mx = logit[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < NCLS; ++c)
    if (logit[c] > mx) { mx = logit[c]; am = c; }
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
    if (t == c) a.logits[(size_t)row * NCLS + c] = logit[c];
  if (t == 0) a.classes[row] = am;
  if (!a.labels) return;
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) se += FAST ? __expf(logit[c] - mx) : expf(logit[c] - mx);
  const float lse = mx + (FAST ? __logf(se) : logf(se));
  // the label's logit by selects: a label outside [0, 10) reads no register that is not there
  float ll = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
    if (c == lbl) ll = logit[c];
  if (t == 0) {
    a.loss_row[row] = lse - ll;
    a.correct_row[row] = (am == lbl) ? 1.f : 0.f;
  }
}

// ---------------- the record fold ----------------
constexpr int kRedThreads = 256;
constexpr int kRedWaves = kRedThreads / kWave;
constexpr int kRedTile = 1024;  // rows whose keys one LDS tile holds (4 per thread)

// lane 0 ends with the wave's sum, in a fixed order (step_log.hip)
__device__ __forceinline__ double wave_sum_down(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}

// Thread c < 100 owns cell (t, p) = (c / 10, c % 10): it counts the rows of every tile whose key
// label * 10 + class is c, reading the tile's keys from LDS 16 at a time (every thread the same
// address: a broadcast). Integer counts: exact whatever the order.
__global__ __launch_bounds__(kRedThreads) void eval_reduce_kernel(EvalReduceArgs a) {
  __shared__ double part[kRedWaves][2];
  __shared__ __attribute__((aligned(16))) uint8_t key[kRedTile];
  const int t = threadIdx.x;
  double l = 0.0, k = 0.0;
  for (int i = t; i < a.rows; i += kRedThreads) {
    l += (double)a.loss_row[i];
    k += (double)a.correct_row[i];
  }
  int cnt = 0;
  for (int r0 = 0; r0 < a.rows; r0 += kRedTile) {
    if (r0) __syncthreads();  // the tile before this one has been counted
#pragma unroll
    for (int u = 0; u < kRedTile / kRedThreads; ++u) {
      const int j = u * kRedThreads + t, i = r0 + j;
      uint8_t kk = 255;  // no cell
      if (i < a.rows) {
        const int y = a.labels[i], c = a.classes[i];
        if (y >= 0 && y < NCLS && c >= 0 && c < NCLS) kk = (uint8_t)(y * NCLS + c);
      }
      key[j] = kk;
    }
    __syncthreads();
    if (t < NCLS * NCLS) {
      const int n16 = (min(a.rows - r0, kRedTile) + 15) >> 4;  // keys past the rows are 255
      for (int q = 0; q < n16; ++q) {
        const uint4 v = reinterpret_cast<const uint4*>(key)[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; ++b) cnt += (int)((w[b >> 2] >> (8 * (b & 3))) & 255u) == t ? 1 : 0;
      }
    }
  }
  l = wave_sum_down(l);
  k = wave_sum_down(k);
  if ((t & (kWave - 1)) == 0) {
    part[t / kWave][0] = l;
    part[t / kWave][1] = k;
  }
  __syncthreads();
  const bool add = a.mode == EVAL_ADD;
  if (t < NCLS * NCLS) {
    const double c = (double)cnt;
    a.rec[ERF_CM + t] = add ? a.rec[ERF_CM + t] + c : c;
  }
  if (t != 0) return;
  l = part[0][0];
  k = part[0][1];
#pragma unroll
  for (int i = 1; i < kRedWaves; ++i) {
    l += part[i][0];
    k += part[i][1];
  }
  const double n = (double)a.rows;
  a.rec[ERF_LOSS_SUM] = add ? a.rec[ERF_LOSS_SUM] + l : l;
  a.rec[ERF_ROWS] = add ? a.rec[ERF_ROWS] + n : n;
  a.rec[ERF_CORRECT] = add ? a.rec[ERF_CORRECT] + k : k;
  if (!add) a.rec[ERF_RESERVED] = 0.0;
}

}  // namespace

void infer_head(const InferHeadArgs& a, bool fast, hipStream_t s) {
  if (a.rows < 1) throw std::runtime_error("infer_head: rows >= 1");
  if (a.splits < 1 || a.splits > kInferMaxSplits) throw std::runtime_error("infer_head: 1 <= splits <= kInferMaxSplits");
  if (a.split_rows < a.rows) throw std::runtime_error("infer_head: split_rows below rows");
  if (!a.fc1_slab || !a.p32 || !a.logits || !a.classes) throw std::runtime_error("infer_head: slabs, parameters, logits, classes");
  if (a.labels && (!a.loss_row || !a.correct_row)) throw std::runtime_error("infer_head: labels need loss_row and correct_row");
  if (((reinterpret_cast<uintptr_t>(a.fc1_slab) | reinterpret_cast<uintptr_t>(a.p32)) & 15) != 0)
    throw std::runtime_error("infer_head: slabs and parameters must be 16-byte aligned");
  if (fast) TFD_LAUNCH(infer_head_kernel<true><<<a.rows, 256, 0, s>>>(a));
  else TFD_LAUNCH(infer_head_kernel<false><<<a.rows, 256, 0, s>>>(a));
}

void eval_reduce(const EvalReduceArgs& a, hipStream_t s) {
  if (a.rows < 1) throw std::runtime_error("eval_reduce: rows >= 1");
  if (!a.labels || !a.classes || !a.loss_row || !a.correct_row || !a.rec)
    throw std::runtime_error("eval_reduce: labels, classes, loss_row, correct_row, rec");
  if (a.mode != EVAL_STORE && a.mode != EVAL_ADD) throw std::runtime_error("eval_reduce: mode");
  TFD_LAUNCH(eval_reduce_kernel<<<1, kRedThreads, 0, s>>>(a));
}

}  // namespace tfd
