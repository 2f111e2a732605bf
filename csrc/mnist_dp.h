// DP-SGD (Abadi et al. 2016): per-example gradient norms, clip factors and the Gaussian noise, on the
// device (kernels/mnist_dp.hip). The step's weight-gradient kernels sum over the batch inside their K
// loops, so no per-example quantity of a weight gradient exists anywhere. dp_norm_kernel forms the squared
// L2 norm of every example's gradient g_i (of its OWN loss l_i, not divided by B) over the eight
// variables from the per-example factors the bf16 step leaves in global memory after the forward, the
// head and mnist_backward_a part 2, without ever storing a per-example gradient:
//   fc1 weight  ||p2_i||^2 ||dh_i||^2          fc1 bias  ||dh_i||^2           (outer products: the norm factors)
//   out weight  ||hd_i||^2 ||dlogits_i||^2     out bias  ||dlogits_i||^2
//   conv2       ||im2col(p1_i)^T dz2_i||_F^2 over [800][64],   bias ||sum_p dz2_i[p]||^2
//   conv1       dz1_i as input_grad_kernel phases 1 - 2 form it (conv2 dgrad on the matrix core, bf16 at
//               conv2_bwd_lds's rounding point), then ||im2col(bf16 x_i)^T dz1_i||_F^2 over [25][32] and
//               ||sum_p dz1_i[p]||^2
// each times B^2 (head_kernel folds 1/B into dlogits, and every factor behind it carries it).
//   sq[i][8]  in flat-layout order: wc1, bc1, wc2, bc2, wd1, bd1, out, out_b
//   norm[i] = sqrt(sum_k sq[i][k]),  c[i] = clip / norm[i] where norm[i] > clip, else 1 (a zero norm: 1)
// With `scale` set the kernel then multiplies row i of dlogits (fp32) and of dh and dz2 (bf16: one more
// rounding each) by c[i] in place; a row with c[i] == 1 is not stored and keeps its bits. The backward is
// linear in these rows, so the step's own weight-gradient kernels, unchanged, then produce
// sum_i c_i g_i / B. training/dp_sgd.py per_example_sqnorms_from_factors is the same in numpy fp64.
//
// dp_noise_kernel: grad[j] = fma(amp, z_j, grad[j]) (the exact grad + amp z, rounded once) over the
// elements j inside one of up to 8 real regions; pad elements are not touched. z is N(0, 1) by Box-Muller
// on Philox4x32-10: element group q = j / 4 draws once, counter (q, step lo, step hi, 0), key (seed,
// kDpNoiseKey) -- no rank: every rank of a later multi-rank DP must draw the same noise;
//   u_k = u01(word k);  r0 = sqrt(-2 log(1 - u_0)), r1 = sqrt(-2 log(1 - u_2))    (1 - u is in (0, 1], exact)
//   z[4q .. 4q + 3] = r0 cospi(2 u_1), r0 sinpi(2 u_1), r1 cospi(2 u_3), r1 sinpi(2 u_3)
// training/dp_sgd.py dp_noise_ref is the same in fp64.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace tfd {

constexpr uint32_t kDpNoiseKey = 0xD95A11CEu;  // second Philox key word (dropout's is 0x5EED1234)

struct DpNormArgs {
  const float* data;     // input rows [n][784] fp32, 16-byte aligned: row perm[(*step * B + b) % n], or row b
  const int* perm;       // when perm is null (a fed batch), as the step kernels take theirs
  const int64_t* step;   // the device data cursor; read only with perm
  int n;
  int B;                 // grid: one 256-thread block per batch row, 1 <= B <= 65535
  const uint16_t* p1;    // [B][14][14][32] bf16 pooled conv1 activations (relu live iff != 0)
  const uint8_t* idx1;   // [B][14][14][32] window position of the pooled value, 0..3
  uint16_t* dz2;         // [B][14][14][64] bf16; 16-byte aligned; scaled in place with `scale`
  const uint16_t* p2;    // [B][3136] bf16, 16-byte aligned
  const uint16_t* hd;    // [B][1024] bf16, 16-byte aligned
  uint16_t* dh;          // [B][1024] bf16, 16-byte aligned; scaled in place with `scale`
  float* dlogits;        // [B][10] fp32; scaled in place with `scale`
  const uint16_t* pbf;   // the flat bf16 parameters (mnist_layout.h): W2 is read; 16-byte aligned
  float clip;            // the L2 bound C > 0
  int scale;             // 0: norms only
  float* sq;             // [B][8]
  float* norm;           // [B]
  float* c;              // [B]
};
// Raises the kernel's dynamic-LDS limit (149.5 KB: all of W2 resident). Called by the launcher as well,
// but a caller that captures the launch into a graph calls it once before the capture.
void dp_norm_prepare();
void dp_norm(const DpNormArgs& a, hipStream_t s);

struct DpNoiseArgs {
  float* grad;           // flat fp32 buffer of n elements, 16-byte aligned, n a multiple of 4
  int64_t n;
  int nreg;              // 1..8 regions [beg, end) inside [0, n)
  int64_t beg[8], end[8];
  float amp;             // sigma * C / B
  const int64_t* step;   // device global_step
  uint32_t seed;
};
void dp_noise(const DpNoiseArgs& a, hipStream_t s);

}  // namespace tfd
