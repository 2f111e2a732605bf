// Block-scaled fc1 forward for inference (csrc/mnist_mx.h): mx_pack_fc1_kernel and mx_fc1_fwd_kernel<FMT> on
// v_mfma_scale_f32_32x32x64_f8f6f4. A code object of its own: the step's kernels are not touched.
//
// Operand layout of the 32x32x64 form (lane l: row / column l & 31, half h = l >> 5), of one K step of 64:
//   e4m3   registers 0-3 hold K elements 16 h + [0, 16), registers 4-7 hold 32 + 16 h + [0, 16)
//   e2m1   registers 0-3 hold K elements 32 h + [0, 32), eight to a register, low nibble first
//   scale  the byte of a lane of half h scales K elements [32 h, 32 h + 32) of its row / column: MX block h
// So an e2m1 operand is one block and needs no other lane's data; an e4m3 operand is a HALF of each of the two
// blocks, its partner lane l ^ 32 holding the other halves. The A quantiser therefore takes two partial maxima
// per step and completes them with one cross-lane exchange (both packed into one dword). No LDS is allocated:
// operands go global -> registers -> matrix core, and the packed B image is already in lane order.
#include "../common.h"
#include "../launch_check.h"
#include "../mnist_layout.h"
#include "../mnist_mx.h"

namespace tfd {
using namespace mnist;
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int kSteps = FEAT / 64;  // 49
static_assert(kMxSplits * kMxSteps == kSteps && FEAT % 64 == 0, "7 splits of 7 K steps of 64 cover fc1's K");
static_assert(kMxNTiles * 32 == HID && kMxNTiles % kMxTilesPerWave == 0, "N tiling");
static_assert(kMxSteps <= 8, "a split's scale bytes fit the 8-byte group");

// the scale byte of a block from the bits of its largest magnitude, and 2^(127 - s) as an fp32
__device__ __forceinline__ int mx_scale_byte(uint32_t amax_bits, int emax) {
  const int e = (int)((amax_bits >> 23) & 0xff) - emax;
  return min(max(e, 0), 254);
}
__device__ __forceinline__ float mx_inv_scale(int s) { return __uint_as_float((uint32_t)(254 - s) << 23); }
__device__ __forceinline__ float clamp_abs(float y, float m) { return fminf(fmaxf(y, -m), m); }

// e2m1 code of y, |y| <= 6: magnitude index by the seven midpoints, each tie going to the even mantissa
__device__ __forceinline__ uint32_t e2m1_code(float y) {
  const float a = fabsf(y);
  const uint32_t mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return mag | ((__float_as_uint(y) >> 28) & 8u);
}

// One thread per (block kb, column n): 32 strided reads of W1 (a wave reads 256 contiguous bytes per k), the
// block's codes at their place in the fragment (e2m1: one 16-byte run of lane (n, kb & 1); e4m3: 16 bytes in
// each of lanes (n, 0) and (n, 1), at byte 16 (kb & 1)), and its scale byte in lane (n, kb & 1)'s group.
template <int FMT>
__global__ __launch_bounds__(256) void mx_pack_fc1_kernel(const float* __restrict__ w, uint8_t* __restrict__ packed) {
  const int n = blockIdx.x * 256 + threadIdx.x, kb = blockIdx.y;
  float x[kMxBlock];
  uint32_t amax = 0;
#pragma unroll
  for (int i = 0; i < kMxBlock; ++i) {
    x[i] = w[(size_t)(kb * kMxBlock + i) * HID + n];
    amax = max(amax, __float_as_uint(x[i]) & 0x7fffffffu);
  }
  const int s = mx_scale_byte(amax, FMT == MX_FP4 ? 2 : 8);
  const float inv = mx_inv_scale(s);
  const int nt = n >> 5, ks = kb >> 1, lane = (n & 31) + 32 * (kb & 1);
  const size_t frag = ((size_t)nt * kSteps + ks) * 64 + lane;
  uint32_t q[8];
  if (FMT == MX_FP4) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      q[v] = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) q[v] |= e2m1_code(clamp_abs(x[8 * v + j] * inv, 6.0f)) << (4 * j);
    }
    *reinterpret_cast<uint4*>(packed + frag * 16) = make_uint4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = clamp_abs(x[4 * v + j] * inv, 448.0f);
      int c = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
      q[v] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], c, true);
    }
    uint8_t* lo = packed + (frag - 32 * (kb & 1)) * 32 + 16 * (kb & 1);  // lane (n, 0); lane (n, 1) is 32 operands on
    *reinterpret_cast<uint4*>(lo) = make_uint4(q[0], q[1], q[2], q[3]);
    *reinterpret_cast<uint4*>(lo + 32 * 32) = make_uint4(q[4], q[5], q[6], q[7]);
  }
  uint8_t* sc = packed + mx_code_bytes(FMT) + (((size_t)nt * kMxSplits + ks / kMxSteps) * 64 + lane) * 8;
  sc[ks % kMxSteps] = (uint8_t)s;
  if (ks % kMxSteps == kMxSteps - 1) sc[7] = 0;  // the group's unused byte: the image has no undefined byte
}

// the lane's A operand of one K step. raw[0..1]: its 16 bf16 of block 0, raw[2..3]: its 16 of block 1 -> 32 e4m3
// codes, and the scale byte of the block the lane's half answers for
__device__ __forceinline__ i32x8 mx_quant_a(const uint4 (&raw)[4], int kh, int& s) {
  const uint32_t* u = reinterpret_cast<const uint32_t*>(raw);
  uint32_t amax[2] = {0, 0};  // bf16 magnitudes order as their bits do
#pragma unroll
  for (int i = 0; i < 16; ++i) amax[i >> 3] = max(amax[i >> 3], max(u[i] & 0x7fffu, (u[i] >> 16) & 0x7fffu));
  const uint32_t other = (uint32_t)__shfl_xor((int)(amax[0] | (amax[1] << 16)), 32, 64);  // the partner's halves
  int sb[2];
  sb[0] = mx_scale_byte(max(amax[0], other & 0x7fffu) << 16, 8);
  sb[1] = mx_scale_byte(max(amax[1], other >> 16) << 16, 8);
  s = kh ? sb[1] : sb[0];
  i32x8 q;
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const float inv = mx_inv_scale(sb[v >> 2]);
    float y[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      y[2 * j] = clamp_abs(__uint_as_float(u[2 * v + j] << 16) * inv, 448.0f);
      y[2 * j + 1] = clamp_abs(__uint_as_float(u[2 * v + j] & 0xffff0000u) * inv, 448.0f);
    }
    const int c = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    q[v] = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], c, true);
  }
  return q;
}

// K steps ST .. 6 of one N tile: the step is a template argument because the scale's byte select (op_sel) is part
// of the instruction. bc: the lane's B operand of step 0; consecutive steps are 64 operands apart.
template <int FMT, int ST>
__device__ __forceinline__ void mx_k_steps(const i32x8 (&qa)[kMxSteps], const uint32_t (&sa)[2], const uint8_t* bc, uint2 sb,
                                           f32x16& acc) {
  if constexpr (ST < kMxSteps) {
    i32x8 b;
    if constexpr (FMT == MX_FP4) {
      const i32x4 h = *reinterpret_cast<const i32x4*>(bc + (size_t)ST * 64 * 16);
      b = i32x8{h[0], h[1], h[2], h[3], 0, 0, 0, 0};  // the instruction reads four registers of an e2m1 operand
    } else {
      b = *reinterpret_cast<const i32x8*>(bc + (size_t)ST * 64 * 32);
    }
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(qa[ST], b, acc, MX_FP8, FMT, ST & 3, (int)sa[ST >> 2], ST & 3,
                                                          (int)(ST < 4 ? sb.x : sb.y));
    mx_k_steps<FMT, ST + 1>(qa, sa, bc, sb, acc);
  }
}

// grid (N groups, M tiles, splits), one wave per block. Lane l: row / column l & 31, half l >> 5.
template <int FMT>
__global__ __launch_bounds__(64) void mx_fc1_fwd_kernel(MxFc1Args a) {
  constexpr int kB = FMT == MX_FP4 ? 16 : 32;  // bytes of a lane's B operand
  const int lane = threadIdx.x, r = lane & 31, kh = lane >> 5;
  const int ng = blockIdx.x, mt = blockIdx.y, sp = blockIdx.z;
  const int row = 32 * mt + r;
  // ---- A: all loads of the split first, then the quantiser
  uint4 raw[kMxSteps][4];
  const uint16_t* src = a.p2 + (size_t)row * FEAT + (size_t)sp * kMxSteps * 64 + 16 * kh;
#pragma unroll
  for (int st = 0; st < kMxSteps; ++st)
#pragma unroll
    for (int i = 0; i < 4; ++i)  // 16 elements at 16 kh, 16 at 32 + 16 kh
      raw[st][i] = row < a.rows ? *reinterpret_cast<const uint4*>(src + 64 * st + 32 * (i >> 1) + 8 * (i & 1)) : make_uint4(0, 0, 0, 0);
  i32x8 qa[kMxSteps];
  uint32_t sa[2] = {0, 0};  // the steps' scale bytes, four to a register
#pragma unroll
  for (int st = 0; st < kMxSteps; ++st) {
    int s;
    qa[st] = mx_quant_a(raw[st], kh, s);
    sa[st >> 2] |= (uint32_t)s << (8 * (st & 3));
  }
  // ---- the wave's N tiles
  const uint8_t* scales = a.packed + mx_code_bytes(FMT);
#pragma unroll
  for (int j = 0; j < kMxTilesPerWave; ++j) {
    const int nt = ng * kMxTilesPerWave + j;
    const uint8_t* bc = a.packed + (((size_t)nt * kSteps + (size_t)sp * kMxSteps) * 64 + lane) * kB;
    const uint2 sb = *reinterpret_cast<const uint2*>(scales + (((size_t)nt * kMxSplits + sp) * 64 + lane) * 8);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    mx_k_steps<FMT, 0>(qa, sa, bc, sb, acc);
    // C: register i holds row 8 (i / 4) + 4 kh + i % 4 of column r
    float* out = a.slab + (size_t)sp * a.rows * HID + 32 * nt + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int orow = 32 * mt + 8 * (i >> 2) + 4 * kh + (i & 3);
      if (orow < a.rows) out[(size_t)orow * HID] = acc[i];
    }
  }
}

}  // namespace

void mx_pack_fc1(const float* w, uint8_t* packed, int fmt, hipStream_t s) {
  if (fmt != MX_FP8 && fmt != MX_FP4) throw std::runtime_error("mx_pack_fc1: format is MX_FP8 or MX_FP4");
  if (!w || !packed || ((reinterpret_cast<uintptr_t>(packed) & 31) != 0)) throw std::runtime_error("mx_pack_fc1: w, and a 32-byte aligned image");
  const dim3 g(HID / 256, FEAT / kMxBlock);
  if (fmt == MX_FP4)
    TFD_LAUNCH(mx_pack_fc1_kernel<MX_FP4><<<g, 256, 0, s>>>(w, packed));
  else
    TFD_LAUNCH(mx_pack_fc1_kernel<MX_FP8><<<g, 256, 0, s>>>(w, packed));
}

void mx_fc1_fwd(const MxFc1Args& a, int fmt, hipStream_t s) {
  if (fmt != MX_FP8 && fmt != MX_FP4) throw std::runtime_error("mx_fc1_fwd: format is MX_FP8 or MX_FP4");
  if (a.rows < 1 || a.rows > 65535) throw std::runtime_error("mx_fc1_fwd: 1 <= rows <= 65535");
  if (!a.p2 || !a.packed || !a.slab) throw std::runtime_error("mx_fc1_fwd: p2, packed, slab");
  if (((reinterpret_cast<uintptr_t>(a.p2) & 15) | (reinterpret_cast<uintptr_t>(a.packed) & 31)) != 0)
    throw std::runtime_error("mx_fc1_fwd: p2 must be 16-byte and the packed image 32-byte aligned");
  const dim3 g(kMxNTiles / kMxTilesPerWave, (a.rows + 31) / 32, kMxSplits);
  if (fmt == MX_FP4)
    TFD_LAUNCH(mx_fc1_fwd_kernel<MX_FP4><<<g, 64, 0, s>>>(a));
  else
    TFD_LAUNCH(mx_fc1_fwd_kernel<MX_FP8><<<g, 64, 0, s>>>(a));
}

}  // namespace tfd
