// Monte-Carlo dropout inference of the MNIST CNN (kernels/mnist_mc.hip): T stochastic passes of the
// output layer per row in ONE launch, behind the forward up to fc1 (where infer_head runs). Dropout
// sits behind fc1, so the T passes of a row share its hidden vector; what repeats is the mask and the
// 1024 x 10 output layer, and for one row that is a small GEMM,
//   logits [T][10] = (mask [T][1024] (.) relu(h) / keep_prob) [T][1024]  x  W_out [1024][10],
// on the fp32 matrix core (v_mfma_f32_16x16x4_f32), its A operand drawn in registers and never stored.
// Both engine precisions: the fc1 split-K slabs and the output layer are fp32 in both.
//
//   block     256 threads = 4 waves per row. Prologue as infer_head: slabs added to the fc1 bias in split
//             order, relu -> hr [1024] in LDS. Wave w owns hidden units [256 w, 256 w + 256).
//   tiles     samples in tiles of 16 (one MFMA M tile); per tile a wave runs 16 groups q of 4 MFMAs.
//   lane map  lane l: sample m = l & 15 of the tile, k slot kk = l >> 4, output column n = l & 15. In
//             group q the lane makes ONE Philox call for Philox group
//               g = 64 w + 4 q + kk                  (hidden units 4 g .. 4 g + 3)
//             and MFMA j = 0..3 of the group takes word j: A = kept(word j) ? hr[4 g + j] / keep_prob : 0,
//             B = W_out[4 g + j][n] (0 for n >= 10). Every call is made by exactly one lane and all four
//             of its words are consumed. hr / keep_prob and the B values of a lane do not depend on the
//             tile: 64 + 64 registers, loaded once per block.
//   draws     Philox4x32-10, counter (sample * 256 + g, row lo, row hi, rank), key (seed, kMcDropoutKey);
//             row = row0 + block, 64 bits: a row's masks depend neither on the chunking nor on B.
//             kept iff u01(word) < keep_prob (the training heads' rule and u01).
//   reduce    the four waves' [16][16] partial tiles meet in LDS and are added in wave order, then the
//             output bias; lane m < 16 of wave 0 takes sample m: softmax with expf / logf (both
//             precisions), H = log(se) - sum_c p_c (z_c - max). A sample past T has weight 0: it adds
//             exactly 0 to every statistic; no MFMA sits in a branch.
//   stats     lane m keeps, over its samples m, 16 + m, ...: count, sum H, and per class Welford's mean
//             and M2 (M2 += d * (p - mean'), a product of two differences of one sign: never negative).
//             The 16 lanes are merged in lane order (Chan's pairwise rule, every term >= 0), so
//             var_prob = M2 / T >= 0 and all sums run in one fixed order: bit-identical run to run.
//   outputs   mean_prob [rows][10], classes [rows] (first maximum of mean_prob: strict > in class order),
//             entropy = -sum p log p of mean_prob (0 log 0 = 0), expected_entropy = (1/T) sum_s H_s,
//             mutual_info = max(entropy - expected_entropy, 0) (Jensen: the exact value is >= 0, so the
//             clamp only ever moves a rounded value towards it), var_prob [rows][10]; with labels
//             loss_row = -log mean_prob[label] and correct_row. Plain stores, no atomics, nothing to zero.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tfd {

constexpr uint32_t kMcDropoutKey = 0x4D43D409u;  // second Philox key word (dropout's is 0x5EED1234)
constexpr int kMcMaxSamples = 4096;              // sample * 256 + g stays far inside 32 bits
constexpr int kMcSampleTile = 16;

struct McHeadArgs {
  int rows;                // grid: one block per row
  const float* fc1_slab;   // [splits][split_rows][1024] fp32
  int splits;              // 1 .. kInferMaxSplits
  int split_rows;          // rows between two splits of one row
  const float* p32;        // flat fp32 parameters (mnist_layout.h)
  const int* labels;       // [rows] or null
  int samples;             // T, 1 .. kMcMaxSamples
  float keep_prob;         // (0, 1]
  uint32_t seed, rank;
  uint64_t row0;           // global number of row 0 of this launch
  float* mean_prob;        // [rows][10]
  int* classes;            // [rows]
  float* entropy;          // [rows]
  float* expected_entropy; // [rows] or null
  float* mutual_info;      // [rows]
  float* var_prob;         // [rows][10]
  float* loss_row;         // [rows], with labels
  float* correct_row;      // [rows], with labels
};
void mc_head(const McHeadArgs& a, hipStream_t s);

}  // namespace tfd
