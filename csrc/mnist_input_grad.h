// Gradient of the step's cost with respect to the input image, and the FGSM adversarial batch made
// from it (kernels/mnist_input_grad.hip). The bf16 step computes every gradient of the reference's
// `cost` but this one: conv2_bwd_lds forms the conv1 pre-activation gradient dz1 in LDS for the conv1
// weight gradient and drops it. input_grad_kernel continues from what the step leaves in global
// memory after the forward and the fc1 data-gradient pass (mnist_backward_a part 2), per image:
//   1. conv2 dgrad   dp1[p][ci] = sum_{tap,co} dz2[p - tap][co] W2[tap][ci][co]      (p - tap: the SAME-padded
//                    shift p - (kh - 2, kw - 2); M = 196, N = 32, K = 1600 on v_mfma_f32_16x16x32_bf16, fp32 sums)
//   2. relu + pool   dz1[2q + wi][c] = bf16(dp1[q][c]) where p1[q][c] != 0 and wi = idx1[q][c] (row wi >> 1,
//                    column wi & 1 of the window), zero elsewhere: conv2_bwd_lds's rounding point
//   3. conv1 dgrad   T[p][tap] = sum_c dz1[p][c] W1[tap][c]   (M = 784, K = 32, N = 25 padded to 32; fp32, in LDS)
//                    dx[u][v]  = sum_{i,j} T[(u - i + 2, v - j + 2)][5 i + j] over the in-image terms, i then j
//                    ascending: col2im as a gather, a fixed order, no atomics
//   4. epilogue      xadv = min(max(x + eps_b * sign(dx), 0), 1), sign(0) = 0; eps_b = eps for rows b < adv_rows,
//                    else 0, and a row with eps_b == 0 is x bit for bit; yadv = the row's label
// training/adversarial.py input_grad_from_factors is phases 1 - 3 in numpy fp64.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tfd {

struct InputGradArgs {
  const uint16_t* dz2;   // [B][14][14][64] bf16, the dense conv2 pre-activation gradient; 16-byte aligned
  const uint16_t* p1;    // [B][14][14][32] bf16 pooled conv1 activations (relu live iff != 0)
  const uint8_t* idx1;   // [B][14][14][32] window position of the pooled value, 0..3
  const uint16_t* pbf;   // the flat bf16 parameters (mnist_layout.h): W1 and W2 are read; 16-byte aligned
  const float* data;     // input rows [n][784] fp32, 16-byte aligned: row perm[(*step * B + b) % n], or
  const int* labels;     // row b when perm is null (a fed batch), as the step kernels take theirs
  const int* perm;
  const int64_t* step;   // the device data cursor; read only with perm
  int n;
  int B;                 // grid: one 256-thread block per batch row, 1 <= B <= 65535
  float eps;             // >= 0
  int adv_rows;          // rows b < adv_rows are perturbed
  float* dx;             // [B][784] fp32 or null (not stored); 16-byte aligned
  float* xadv;           // [B][784] fp32 or null, 16-byte aligned; yadv [B] goes with it
  int* yadv;
};
// Raises the kernel's dynamic-LDS limit (149.5 KB: all of W2 resident). Called by the launcher as well,
// but a caller that captures the launch into a graph calls it once before the capture.
void input_grad_prepare();
void input_grad(const InputGradArgs& a, hipStream_t s);

}  // namespace tfd
