// Write-through (sc1) vector stores for tensors that the NEXT kernel reads.
//
// A plain store leaves its line dirty in the storing XCD's write-back L2; what a kernel stores in its
// epilogue is still there when the kernel ends, and the end-of-kernel write-back of those lines is
// serialised in front of the dependent kernel (MI355X: about B / 6 TB/s for B dirty bytes). An sc1
// store goes through to memory while the block's other waves still run and leaves no dirty line
// behind. Its line is dropped from the storing XCD's L2, so it is for outputs the producer never
// re-reads. Visibility is the kernel boundary's, as for a plain store: no fence, no flag.
//
// Raw buffer stores through a descriptor over [base, base + nbytes) (both wave-uniform): a lane
// whose predicate is false gets an offset past the range and the hardware range check drops its
// store, the way buf_ld (gemm.h) zero-fills a load. nbytes < 2 GiB.
#pragma once
#include "common.h"

namespace tfd {

__device__ __forceinline__ uint4 f4_bits(f32x4 x) {
  return make_uint4(__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3]));
}

struct WtBuf {
  __amdgpu_buffer_rsrc_t r;
};
__device__ __forceinline__ WtBuf wt_buf(const void* base, int64_t nbytes) {
  return WtBuf{__builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)nbytes, 0x00020000)};
}
constexpr uint32_t kWtDrop = 0xFFFFFFF0u;  // past every range
constexpr int kWtSc1 = 16;                 // aux bit 4 = sc1 on gfx94x / gfx950
typedef int wt_i32x4 __attribute__((ext_vector_type(4)));
typedef int wt_i32x2 __attribute__((ext_vector_type(2)));

// 16 / 8 / 4 bytes at byte offset `off` of the buffer (a multiple of the size); ok == false: dropped
__device__ __forceinline__ void wt_store16(const WtBuf& b, uint32_t off, bool ok, uint4 v) {
  const wt_i32x4 x = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
  __builtin_amdgcn_raw_buffer_store_b128(x, b.r, ok ? off : kWtDrop, 0, kWtSc1);
}
__device__ __forceinline__ void wt_store8(const WtBuf& b, uint32_t off, bool ok, uint2 v) {
  const wt_i32x2 x = {(int)v.x, (int)v.y};
  __builtin_amdgcn_raw_buffer_store_b64(x, b.r, ok ? off : kWtDrop, 0, kWtSc1);
}
__device__ __forceinline__ void wt_store4(const WtBuf& b, uint32_t off, bool ok, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b32((int)v, b.r, ok ? off : kWtDrop, 0, kWtSc1);
}

}  // namespace tfd
