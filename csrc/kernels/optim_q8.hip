// 8-bit Adam over the flat buffer (csrc/optim_q8.h): a fused decode -> update -> reduce -> encode in
// registers, and the codec alone (q8_encode / q8_decode) on the same helpers. A code object of its own: the
// flat Adam / momentum / rules kernels (optim*.hip) and the fused MNIST tail stay what they were.
//
// How the work is split. One wave owns one 256-element block at a time; lane l holds elements 4l .. 4l + 3,
// so a block is one 16-B load of p and of g (8 B on the bf16 wire) and one 4-B load of each code word per
// lane, and its two scales are wave-uniform. The block's new maxima are wave reductions in registers: four
// DPP steps (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) leave every lane of a 16-lane row with its
// row's maximum, and four v_readlane (lanes 0, 16, 32, 48) finish on the scalar side. The operands are
// magnitudes (>= 0), so max is order-free and every run gives the same bits. No LDS, no barrier, no atomics,
// no memset. A lane's four codes are packed by two v_cvt_pk_{fp8,bf8}_f32 into one dword and stored as 4 B;
// lane 0 stores the two scales. A workgroup is 4 waves; the grid is capped as rule_blocks caps it and strides
// over the blocks, one block per wave and iteration (two in flight measured 8 - 11 % slower over MNIST's buffer).
//
// The first iteration's operands are requested before the step counter, the clip factor and the guard's ok
// are awaited; with ok == 0 the kernel returns before its first store (wave-uniform). The wire format and the
// EMA pointer are tested once, around the whole body. The ragged end: a lane whose four elements do not all
// lie below n loads and stores element by element, its missing elements contribute 0 to the maxima, and
// nothing at or past n is read or written in any buffer (the scales: nothing at or past q8_blocks(n)).
#include <math.h>

#include <stdexcept>
#include <string>

#include "../common.h"
#include "../ema.h"
#include "../launch_check.h"
#include "../optim_q8.h"

namespace tfd {
namespace {

constexpr int kQ8Threads = 256;
constexpr int kQ8Waves = kQ8Threads / 64;
constexpr int kQ8MaxBlocks = 2048;

typedef __attribute__((ext_vector_type(2))) float f32x2;

// ---- the wave's maximum of a non-negative value; all 64 lanes are active where it is called ----
template <int CTRL>
__device__ __forceinline__ float q8_dpp_max(float x) {
  // bound_ctrl: a lane without a source reads 0, the identity of max over magnitudes
  const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true);
  return fmaxf(x, __int_as_float(y));
}
__device__ __forceinline__ float q8_wave_max(float x) {
  x = q8_dpp_max<0xB1>(x);   // quad_perm [1,0,3,2]: lane ^ 1
  x = q8_dpp_max<0x4E>(x);   // quad_perm [2,3,0,1]: lane ^ 2
  x = q8_dpp_max<0x141>(x);  // row_half_mirror: the other quad of the 8
  x = q8_dpp_max<0x140>(x);  // row_mirror: the other 8 of the row
  const int b = __float_as_int(x);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// ---- four codes <-> four values: one conversion per pair; byte j of the word is element j ----
template <int KIND>
__device__ __forceinline__ f32x4 q8_unpack(uint32_t w) {
  f32x2 lo, hi;
  if (KIND == Q8_M) {
    lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  } else {
    lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
  }
  return f32x4{lo[0], lo[1], hi[0], hi[1]};
}
template <int KIND>
__device__ __forceinline__ uint32_t q8_pack(const f32x4& x) {
  int w;
  if (KIND == Q8_M) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(x[0], x[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(x[2], x[3], w, true);
  }
  return (uint32_t)w;
}
// a positive value whose code came out 0x00 takes 0x01 (kind v)
__device__ __forceinline__ uint32_t q8_floor(uint32_t w, const f32x4& x) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (x[j] > 0.f && ((w >> (8 * j)) & 0xFFu) == 0u) w |= 1u << (8 * j);
  return w;
}
// a block's codes of kind KIND from its values and its stored maximum (q8_absmax): inv is finite, and in the
// zero block (absmax == 0) every product is 0 and the codes stay 0
template <int KIND>
__device__ __forceinline__ uint32_t q8_encode4(const f32x4& x, float absmax) {
  const uint32_t w = q8_pack<KIND>(x * q8_inv(absmax, KIND));
  return KIND == Q8_V && absmax > 0.f ? q8_floor(w, x) : w;
}
template <int KIND>
__device__ __forceinline__ f32x4 q8_decode4(uint32_t w, float absmax) {
  return q8_unpack<KIND>(w) * q8_dscale(absmax, KIND);
}

// ---- a lane's four elements at e0 = 256 block + 4 lane, cnt (0..4) of them below n ----
__device__ __forceinline__ int q8_cnt(int64_t n, int64_t e0) {
  const int64_t left = n - e0;
  return left >= 4 ? 4 : (left > 0 ? (int)left : 0);
}
__device__ __forceinline__ f32x4 q8_ld_f4(const float* x, int64_t e0, int cnt) {
  f32x4 r{0.f, 0.f, 0.f, 0.f};
  if (cnt == 4) return *reinterpret_cast<const f32x4*>(x + e0);
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < cnt) r[j] = x[e0 + j];
  return r;
}
__device__ __forceinline__ void q8_st_f4(float* x, int64_t e0, int cnt, const f32x4& v) {
  if (cnt == 4) {
    *reinterpret_cast<f32x4*>(x + e0) = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < cnt) x[e0 + j] = v[j];
}
__device__ __forceinline__ uint32_t q8_ld_w(const uint8_t* c, int64_t e0, int cnt) {
  if (cnt == 4) return *reinterpret_cast<const uint32_t*>(c + e0);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < cnt) w |= (uint32_t)c[e0 + j] << (8 * j);
  return w;
}
__device__ __forceinline__ void q8_st_w(uint8_t* c, int64_t e0, int cnt, uint32_t w) {
  if (cnt == 4) {
    *reinterpret_cast<uint32_t*>(c + e0) = w;
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < cnt) c[e0 + j] = (uint8_t)(w >> (8 * j));
}
// the bf16 wire: four elements as two dwords, element j in half j & 1 of dword j >> 1
__device__ __forceinline__ uint2 q8_ld_bf4(const uint16_t* x, int64_t e0, int cnt) {
  if (cnt == 4) return *reinterpret_cast<const uint2*>(x + e0);
  uint32_t h[3] = {0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < cnt) h[j] = x[e0 + j];
  return make_uint2(h[0] | (h[1] << 16), h[2]);
}
__device__ __forceinline__ f32x4 q8_bf4_f32(const uint2& r) {
  return f32x4{bf2f((uint16_t)(r.x & 0xFFFF)), bf2f((uint16_t)(r.x >> 16)), bf2f((uint16_t)(r.y & 0xFFFF)),
               bf2f((uint16_t)(r.y >> 16))};
}
__device__ __forceinline__ void q8_st_bf4(uint16_t* x, int64_t e0, int cnt, const f32x4& v) {
  if (cnt == 4) {
    *reinterpret_cast<uint2*>(x + e0) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < cnt) x[e0 + j] = f2bf_bits(v[j]);
}

// one block's operands of one lane as loaded: the gradient keeps its wire form until the loads are issued
struct Q8Item {
  f32x4 p, g, e;
  uint2 gb;
  uint32_t m8, v8;
  float am, av;
  int cnt;
};
template <bool BF, bool EMA>
__device__ __forceinline__ Q8Item q8_load(const Adam8Args& a, int64_t qb, int lane) {  // qb < q8_blocks(n)
  Q8Item x{};
  const int64_t e0 = qb * kQ8Block + 4 * lane;
  x.cnt = q8_cnt(a.n, e0);
  x.p = q8_ld_f4(a.p, e0, x.cnt);
  if (BF) x.gb = q8_ld_bf4(a.gbf, e0, x.cnt);
  else x.g = q8_ld_f4(a.g, e0, x.cnt);
  x.m8 = q8_ld_w(a.m8, e0, x.cnt);
  x.v8 = q8_ld_w(a.v8, e0, x.cnt);
  x.am = a.am[qb];
  x.av = a.av[qb];
  if (EMA) x.e = q8_ld_f4(a.ema, e0, x.cnt);
  return x;
}

// decode, THE element update (optim_q8.h), the two maxima, encode, store. Wave-uniform call: all lanes active.
template <bool BF, bool EMA>
__device__ __forceinline__ void q8_apply(const Adam8Args& a, int64_t qb, int lane, const Q8Item& x, float mul, float lr_t,
                                         float c1, float c2, float omd) {
  const int64_t e0 = qb * kQ8Block + 4 * lane;
  const f32x4 g = (BF ? q8_bf4_f32(x.gb) : x.g) * mul;
  f32x4 m = q8_decode4<Q8_M>(x.m8, x.am);
  f32x4 v = q8_decode4<Q8_V>(x.v8, x.av);
  f32x4 p = x.p, e = x.e;
  float mx = 0.f, vx = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m[j] = adam8_m(m[j], g[j], c1);
    v[j] = adam8_v(v[j], g[j], c2);
    p[j] = adam8_p(p[j], m[j], v[j], lr_t, a.eps);
    if (EMA) e[j] = ema_step(e[j], p[j], omd);
    if (j >= x.cnt) {  // past n: contributes 0 to the maxima
      m[j] = 0.f;
      v[j] = 0.f;
    }
    mx = fmaxf(mx, fabsf(m[j]));
    vx = fmaxf(vx, fabsf(v[j]));
  }
  const float am = q8_absmax(q8_wave_max(mx)), av = q8_absmax(q8_wave_max(vx));
  const uint32_t wm = q8_encode4<Q8_M>(m, am), wv = q8_encode4<Q8_V>(v, av);
  if (x.cnt > 0) {
    q8_st_f4(a.p, e0, x.cnt, p);
    q8_st_w(a.m8, e0, x.cnt, wm);
    q8_st_w(a.v8, e0, x.cnt, wv);
    if (a.pbf) q8_st_bf4(a.pbf, e0, x.cnt, p);
    if (EMA) q8_st_f4(a.ema, e0, x.cnt, e);
  }
  if (lane == 0) {
    a.am[qb] = am;
    a.av[qb] = av;
  }
}

template <bool BF, bool EMA>
__device__ __forceinline__ void adam8_body(const Adam8Args& a) {
  const int lane = threadIdx.x & 63;
  const int64_t nb = q8_blocks(a.n);
  const int64_t nwaves = (int64_t)gridDim.x * kQ8Waves;
  const int64_t w0 = (int64_t)blockIdx.x * kQ8Waves + (threadIdx.x >> 6);
  Q8Item x{};
  if (w0 < nb) x = q8_load<BF, EMA>(a, w0, lane);
  // dependent loads, awaited behind the first iteration's requests
  const int64_t t = (a.step ? *a.step : 0) + a.t_offset;
  const float clip = *a.gscale;
  const float ok = a.ok ? *a.ok : 1.f;
  if (ok == 0.f) return;  // wave-uniform, before the first store: a skipped step writes nothing
  const float lr_t = adam8_lr_t(lr_at(a.sched, t - 1), a.beta1, a.beta2, t);
  const float mul = a.grad_scale * clip;
  const float c1 = 1.f - a.beta1, c2 = 1.f - a.beta2;
  const float omd = EMA ? ema_omd_at(a.ema_decay, a.ema_num_updates, t) : 0.f;
  for (int64_t qb = w0; qb < nb; qb += nwaves) {
    if (qb != w0) x = q8_load<BF, EMA>(a, qb, lane);
    q8_apply<BF, EMA>(a, qb, lane, x, mul, lr_t, c1, c2, omd);
  }
}

// the wire format and the EMA shadow are tested once, around the whole body
__global__ __launch_bounds__(kQ8Threads) void adam8_kernel(Adam8Args a) {
  if (a.gbf) {
    if (a.ema) adam8_body<true, true>(a);
    else adam8_body<true, false>(a);
  } else {
    if (a.ema) adam8_body<false, true>(a);
    else adam8_body<false, false>(a);
  }
}

// ---- the codec alone: checkpoint I/O and the tests use the kernels' own encode / decode ----
template <int KIND>
__device__ __forceinline__ void q8_encode_body(const Q8CodecArgs& a) {
  const int lane = threadIdx.x & 63;
  const int64_t nb = q8_blocks(a.n);
  const int64_t nwaves = (int64_t)gridDim.x * kQ8Waves;
  for (int64_t qb = (int64_t)blockIdx.x * kQ8Waves + (threadIdx.x >> 6); qb < nb; qb += nwaves) {
    const int64_t e0 = qb * kQ8Block + 4 * lane;
    const int cnt = q8_cnt(a.n, e0);
    const f32x4 x = q8_ld_f4(a.x, e0, cnt);  // 0 past n
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) mx = fmaxf(mx, fabsf(x[j]));
    const float am = q8_absmax(q8_wave_max(mx));
    const uint32_t w = q8_encode4<KIND>(x, am);
    if (cnt > 0) q8_st_w(a.codes, e0, cnt, w);
    if (lane == 0) a.absmax[qb] = am;
  }
}
__global__ __launch_bounds__(kQ8Threads) void q8_encode_kernel(Q8CodecArgs a) {
  if (a.kind == Q8_M) q8_encode_body<Q8_M>(a);
  else q8_encode_body<Q8_V>(a);
}
__global__ __launch_bounds__(kQ8Threads) void q8_decode_kernel(Q8CodecArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nb = q8_blocks(a.n);
  const int64_t nwaves = (int64_t)gridDim.x * kQ8Waves;
  for (int64_t qb = (int64_t)blockIdx.x * kQ8Waves + (threadIdx.x >> 6); qb < nb; qb += nwaves) {
    const int64_t e0 = qb * kQ8Block + 4 * lane;
    const int cnt = q8_cnt(a.n, e0);
    if (cnt == 0) continue;
    const uint32_t w = q8_ld_w(a.codes, e0, cnt);
    const float am = a.absmax[qb];
    q8_st_f4(a.x, e0, cnt, a.kind == Q8_M ? q8_decode4<Q8_M>(w, am) : q8_decode4<Q8_V>(w, am));
  }
}

// workgroups for n elements at one block per wave and iteration, capped as rule_blocks caps its grid
int q8_grid(int64_t n) {
  const int64_t b = (q8_blocks(n) + kQ8Waves - 1) / kQ8Waves;
  return (int)(b < 1 ? 1 : (b > kQ8MaxBlocks ? kQ8MaxBlocks : b));
}
bool q8_aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
void q8_need(bool ok, const char* who, const char* what) {
  if (!ok) throw std::runtime_error(std::string(who) + ": " + what);
}

}  // namespace

void adam8_apply(const Adam8Args& a, hipStream_t s) {
  const char* who = "adam8_apply";
  q8_need(a.n >= 1, who, "n >= 1");
  q8_need(a.p && a.m8 && a.v8 && a.am && a.av && a.gscale, who, "p, both code buffers, both scale buffers and gscale are required");
  q8_need((a.g != nullptr) != (a.gbf != nullptr), who, "exactly one of g and gbf");
  q8_need(q8_aligned(a.p, 16) && q8_aligned(a.g, 16) && q8_aligned(a.ema, 16) && q8_aligned(a.gbf, 8) && q8_aligned(a.pbf, 8) &&
              q8_aligned(a.m8, 4) && q8_aligned(a.v8, 4) && q8_aligned(a.am, 4) && q8_aligned(a.av, 4),
          who, "unaligned buffer (16 bytes for fp32, 8 for bf16, 4 for the codes and scales)");
  TFD_LAUNCH(adam8_kernel<<<q8_grid(a.n), kQ8Threads, 0, s>>>(a));
}
namespace {
void q8_codec_check(const Q8CodecArgs& a, const char* who) {
  q8_need(a.n >= 1, who, "n >= 1");
  q8_need(a.x && a.codes && a.absmax, who, "x, codes and absmax are required");
  q8_need(a.kind == Q8_M || a.kind == Q8_V, who, "kind is m (e4m3) or v (e5m2)");
  q8_need(q8_aligned(a.x, 16) && q8_aligned(a.codes, 4) && q8_aligned(a.absmax, 4), who,
          "unaligned buffer (16 bytes for fp32, 4 for the codes and scales)");
}
}  // namespace
void q8_encode_launch(const Q8CodecArgs& a, hipStream_t s) {
  q8_codec_check(a, "q8_encode");
  TFD_LAUNCH(q8_encode_kernel<<<q8_grid(a.n), kQ8Threads, 0, s>>>(a));
}
void q8_decode_launch(const Q8CodecArgs& a, hipStream_t s) {
  q8_codec_check(a, "q8_decode");
  TFD_LAUNCH(q8_decode_kernel<<<q8_grid(a.n), kQ8Threads, 0, s>>>(a));
}
int q8_max_blocks() { return kQ8MaxBlocks; }
int q8_threads() { return kQ8Threads; }

}  // namespace tfd
