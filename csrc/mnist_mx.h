// Block-scaled (OCP MX) inference of fc1 (kernels/mnist_mx.hip): the [rows x 3136] x [3136 x 1024] product on
// gfx950's scaled matrix instruction, v_mfma_scale_f32_32x32x64_f8f6f4, with weights kept as MXFP8 or MXFP4 and
// activations quantised to MXFP8 in registers. The training step and the bf16 / fp32 forwards are not touched.
//
// The format (numpy: training/mx_quant.py). A block is 32 consecutive elements along K with one E8M0 scale byte s,
// scale 2^(s - 127); elements are e4m3 (finite-only, max 448; "mxfp8") or e2m1 (max 6; "mxfp4"). Encode, on the bits:
//   amax = max |x| over the block;  E = (bits(amax) >> 23) & 0xff;  s = clamp(E - emax, 0, 254), emax = 8 / 2;
//   code = rne(x * 2^(127 - s)) in the element format, saturated to the maximum ((448, 512) -> 448, (6, 8) -> 6).
// A zero block has s = 0 and zero codes. Inputs are finite (then s <= 252 and 2^(127 - s) is a normal fp32).
//
// The packed image of W1 (mx_pack_fc1), in the order the GEMM's lanes read it. K runs in 49 steps of 64 (two
// blocks), N in 32 tiles of 32, the K steps in kMxSplits = 7 splits of kMxSteps = 7. One B operand of one MFMA,
// lane l = column n = 32 nt + (l & 31), half h = l >> 5, in the instruction's own register order:
//   e2m1    K elements 64 ks + 32 h + [0, 32): one block, 16 bytes, element 2 i in the low nibble of byte i
//   e4m3    K elements 64 ks + 16 h + [0, 16), then 64 ks + 32 + 16 h + [0, 16): half of each block, 32 bytes
//   codes   [nt][ks][lane][16 B | 32 B]
//   scales  [nt][split][lane][8]: byte j < 7 the scale of block 2 (7 split + j) + h, byte 7 zero; behind the codes.
// So a lane's operand is one 16 / 32-byte load, and the seven scales of a split one 8-byte load, handed to the
// instruction four to a register with the byte chosen by its op_sel.
//
// mx_fc1_fwd: one wave per (32 rows, one split, kMxTilesPerWave N tiles), no LDS. The lane loads the 7 x 64 bytes
// of bf16 p2 that are its A operands (two runs of 32 bytes per step), takes each block's maximum over its half
// and its partner lane's (one cross-lane exchange per step), forms the scale bytes, converts to e4m3
// (v_cvt_pk_fp8_f32 behind a clamp to +-448) and keeps the 7 operands in 56 registers against all its N tiles.
// Rows past `rows` load as zero and are not stored. Output: split-K slabs [kMxSplits][rows][1024] fp32, the layout
// infer_head and mc_head read. Plain stores, no atomics, nothing to zero.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace tfd {

enum MxFormat { MX_FP8 = 0, MX_FP4 = 4 };  // the instruction's cbsz / blgp code of the element format

constexpr int kMxBlock = 32;         // elements per scale
constexpr int kMxSplits = 7;         // split-K slabs (<= kInferMaxSplits)
constexpr int kMxSteps = 7;          // K steps of 64 per split: 7 x 7 x 64 = 3136
constexpr int kMxNTiles = 32;        // 1024 / 32
constexpr int kMxTilesPerWave = 4;   // N tiles a wave runs its quantised A operands against
constexpr size_t kMxScaleBytes = (size_t)kMxNTiles * kMxSplits * 64 * 8;
constexpr size_t mx_code_bytes(int fmt) { return (size_t)3136 * 1024 / (fmt == MX_FP4 ? 2 : 1); }
constexpr size_t mx_packed_bytes(int fmt) { return mx_code_bytes(fmt) + kMxScaleBytes; }

// w: W1 [3136][1024] fp32 (the master copy or the EMA shadow); packed: mx_packed_bytes(fmt), 32-byte aligned
void mx_pack_fc1(const float* w, uint8_t* packed, int fmt, hipStream_t s);

struct MxFc1Args {
  int rows;               // 1 .. 65535
  const uint16_t* p2;     // [rows][3136] bf16, 16-byte aligned
  const uint8_t* packed;  // mx_pack_fc1's image in format fmt
  float* slab;            // [kMxSplits][rows][1024]
};
void mx_fc1_fwd(const MxFc1Args& a, int fmt, hipStream_t s);

}  // namespace tfd
