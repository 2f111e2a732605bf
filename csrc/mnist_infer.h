// Device inference of the MNIST CNN (kernels/mnist_infer.hip): the output layer as a head of its own
// that stores what the training heads keep in registers, and the fold of its per-row results into
// evaluation records. Both precisions: the fc1 split-K slabs are fp32 and the output layer is read
// from a flat fp32 parameter buffer in the bf16 and in the fp32 engine alike.
//
//   infer_head   one 256-thread block per row behind the forward up to fc1 (mnist_forward_nohead /
//                mnist_f32_forward_nohead). The logits are formed operation for operation as
//                head_kernel / f32_head form them at train = 0 -- slabs added to the fc1 bias in
//                split order, relu, four fmaf per class, the DPP wave sums, the four wave totals in
//                wave order plus the output bias -- so a row's logits are the numbers its loss was
//                taken from. Stores logits [rows][10] and classes [rows] (first maximum: strict > in
//                class order); with labels also loss_row = lse - logit[label] and correct_row, with
//                the fast exp / log of head_kernel (fast = true) or expf / logf of f32_head. No
//                dropout, no step read, none of the backward's operands.
//   eval_reduce  one 256-thread block folds the rows of one chunk into one record
//                  fp64 [104] = {loss_sum, rows, correct, 0, cm[10][10]}    cm[t][p]: label t, class p
//                EVAL_STORE writes the whole record (a group's first chunk), EVAL_ADD adds to it. No
//                atomics and nothing to zero; the sums run in a fixed order, so a record is bit-identical
//                run to run and replay to eager call. loss_sum is an fp64 sum of the fp32 rows; the
//                counts are exact. A row whose label or class is outside [0, 10) is in no cell.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tfd {

constexpr int kInferMaxSplits = 8;   // fc1 split-K slabs a head block can hold in registers
constexpr int kEvalRecFields = 104;  // {loss_sum, rows, correct, 0} + 10 x 10
enum EvalRecField { ERF_LOSS_SUM = 0, ERF_ROWS, ERF_CORRECT, ERF_RESERVED, ERF_CM };
enum EvalRecMode { EVAL_STORE = 0, EVAL_ADD = 1 };

struct InferHeadArgs {
  int rows;                // grid: one block per row
  const float* fc1_slab;   // [splits][split_rows][1024] fp32
  int splits;              // 1 .. kInferMaxSplits
  int split_rows;          // rows between two splits of one row (the forward's batch)
  const float* p32;        // flat fp32 parameters (mnist_layout.h): the master copy or the EMA shadow
  const int* labels;       // [rows] or null
  float* logits;           // [rows][10]
  int* classes;            // [rows]
  float* loss_row;         // [rows], with labels
  float* correct_row;      // [rows], with labels
};
void infer_head(const InferHeadArgs& a, bool fast, hipStream_t s);

struct EvalReduceArgs {
  int rows;                // >= 1
  const int* labels;       // [rows]
  const int* classes;      // [rows]
  const float* loss_row;   // [rows]
  const float* correct_row;
  double* rec;             // one record, [kEvalRecFields]
  int mode;                // EvalRecMode
};
void eval_reduce(const EvalReduceArgs& a, hipStream_t s);

}  // namespace tfd
