// The one-GPU optimizer tail of the MNIST step (mnist_adam_kernel) as a template over its argument
// struct, with the device helpers it shares with csrc/kernels/mnist.hip. Two .hip files instantiate
// it: mnist.hip with MnistAdamConst (optim_const.h: a constant rate -- the default path, the kernel
// as it was before schedules) and mnist_tail_sched.hip with MnistAdamArgs (the LrSchedule evaluated
// from the head kernel's t). A third, mnist_tail_ema.hip, takes it over MnistAdamEmaArgs: the
// scheduled instantiation plus the moving average of the weights, updated from p' while the tail holds
// it in registers (ema.h). They are separate code objects on purpose: the scheduled instantiation
// is twice the size, and inside mnist.hip's code object it would move every hot kernel of the default
// step (docs/DESIGN.md section 9).
#pragma once
#include "common.h"
#include "launch_check.h"
#include "mnist_layout.h"
#include "optim_const.h"
#include "tfd_kernels.h"

// fc-region Adam: strides per lane with all loads issued up front (1: -0.5 us/step against 2 with the
// round-6 kernels, 4: +0.6; profiles/mnist_conv2_wgrad_grouping_r6.log)
constexpr int ADAM_U = 1;

namespace tfd {
using namespace mnist;
// the scheduled instantiation's launcher (mnist_tail_sched.hip)
void mnist_adam_fused_sched(const MnistStepArgs& a, const MnistAdamArgs& o, hipStream_t s, bool fc_region);

namespace {

// gather block b: the batch row b of step `next` into rows / xpre / ypre; block 0 also writes the
// tag (visibility to the next kernel is the kernel boundary)
__device__ __forceinline__ void gather_next(const MnistStepArgs& a, int64_t next, int b) {
  const int row = a.perm[(int)((next * (int64_t)a.B + b) % (int64_t)a.n_data)];
  const f32x4* src = reinterpret_cast<const f32x4*>(a.data + (size_t)row * 784);
  f32x4* dst = reinterpret_cast<f32x4*>(a.xpre + (size_t)b * 784);
  for (int i = threadIdx.x; i < 196; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) {
    a.rows[b] = row;
    a.ypre[b] = a.labels[row];
    if (b == 0) a.rows[a.B] = (int)next;
  }
}
// (counted by the launcher: the tail takes the number as a leading kernel parameter)
inline int gather_blocks(const MnistStepArgs& a) { return (a.perm && a.xpre) ? a.B : 0; }

// ---------------- one-GPU optimizer tail: K16 ApplyAdam with the K12/K14/K15 slab reduce fused ----------------
// Grid = [13 conv1 blocks | 201 conv2 blocks | MAD_FC_BLOCKS grid-stride blocks]:
//   conv1: block owns 16 float4 of the 832 conv1 weight/bias gradients; thread (q = t >> 4, x = t & 15)
//          sums slabs q, q + 16, ... of float4 x (16-lane groups read 256 contiguous bytes per slab,
//          every load issued before the first add), then the 16 partials are summed in LDS in q order;
//   conv2: block owns 64 float4; thread (q = t >> 6, x = t & 63) sums slabs q, q + 4, ... (each wave
//          reads 1 KiB contiguous per slab), then 4 partials in LDS in q order;
//   fc:    plain grid-stride Adam over the flat gradient buffer.
// Every gradient reduction is deterministic (fixed order). t comes from the head kernel
// (MnistStepArgs::t_out), so nothing here reads the global_step that the last block bumps.
// (The previous layout -- one 16-lane group per float4, each lane a different slab -- made every
//  wave instruction touch 64 scattered 16-B pieces: 7.6 us for the conv region alone.)
constexpr int MAD_NT = 256;
constexpr int MAD_C1F4 = (int)(OFF_WC2 / 4);   // 208
constexpr int MAD_C2END = (int)(OFF_WD1 / 4);  // 13024
constexpr int MAD_C1BLK = MAD_C1F4 / 16;       // 13
constexpr int MAD_C2BLK = (MAD_C2END - MAD_C1F4 + 63) / 64;  // 201
constexpr int MAD_FC_BLOCKS = 1024;  // grid-stride blocks of the fc-region Adam (512 / 2048: within noise)
constexpr int MAD_CONV = MAD_C1BLK + MAD_C2BLK;
static_assert(MAD_C1F4 % 16 == 0, "conv1 region: whole blocks");
constexpr int MAD_SL = 16;  // slab loads in flight per thread
// em / e / omd (adam4: em / omd): the moving average of the weights (optim_const.h, ema.h), updated
// from p' here -- empty tags unless the kernel's argument is the EMA wrapper
template <class Opt, class E, class EV, class EO>
__device__ __forceinline__ void adam4_pre(const Opt& o, int64_t i, f32x4 p, f32x4 m, f32x4 v, f32x4 g, float lr_t,
                                          float c1, float c2, const E& em, EV e, EO omd) {
  m = m + (g - m) * c1;
  v = v + (g * g - v) * c2;
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] -= lr_t * m[j] / (sqrtf(v[j]) + o.eps);
  reinterpret_cast<f32x4*>(o.p)[i] = p;
  reinterpret_cast<f32x4*>(o.m)[i] = m;
  reinterpret_cast<f32x4*>(o.v)[i] = v;
  if (o.pbf) reinterpret_cast<uint2*>(o.pbf)[i] = make_uint2(pack_bf2(p[0], p[1]), pack_bf2(p[2], p[3]));
  ema_store4(em, i, e, omd, p);
}
template <class Opt, class E, class EO>
__device__ __forceinline__ void adam4(const Opt& o, int64_t i, f32x4 g, float lr_t, float c1, float c2, const E& em,
                                      EO omd) {
  f32x4 p = reinterpret_cast<f32x4*>(o.p)[i];
  f32x4 m = reinterpret_cast<f32x4*>(o.m)[i];
  f32x4 v = reinterpret_cast<f32x4*>(o.v)[i];
  const auto e = ema_load4(em, i);
  m = m + (g - m) * c1;
  v = v + (g * g - v) * c2;
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] -= lr_t * m[j] / (sqrtf(v[j]) + o.eps);
  reinterpret_cast<f32x4*>(o.p)[i] = p;
  reinterpret_cast<f32x4*>(o.m)[i] = m;
  reinterpret_cast<f32x4*>(o.v)[i] = v;
  if (o.pbf) reinterpret_cast<uint2*>(o.pbf)[i] = make_uint2(pack_bf2(p[0], p[1]), pack_bf2(p[2], p[3]));
  ema_store4(em, i, e, omd, p);
}
// sum over slabs q, q + QS, ... (< ns) of float4 column x of a [ns][stride4] slab array; MAD_SL loads
// issued per batch before any add
template <int QS>
__device__ __forceinline__ f32x4 slab_sum(const f32x4* __restrict__ s4, int64_t stride4, int ns, int q, int x) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = q; k0 < ns; k0 += QS * MAD_SL) {
    f32x4 v[MAD_SL];
#pragma unroll
    for (int u = 0; u < MAD_SL; ++u) {
      const int k = k0 + u * QS;
      v[u] = k < ns ? s4[(size_t)k * stride4 + x] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < MAD_SL; ++u) acc += v[u];
  }
  return acc;
}
// the update's two scalars, both functions of t: Adam's rate and the shadow's 1 - d_t (an empty tag
// without EMA)
template <class EO> struct TailRates { float lr_t; EO omd; };
// Opt: MnistAdamConst, MnistAdamArgs or MnistAdamEmaArgs (o: the struct itself or the one the wrapper
// holds; em: the wrapper's shadow, else an empty tag)
// Leading parameters: what an fc-region block (1024 of the grid's ~1240) needs for its first loads --
// p / m / v, the bf16 gradient pointer its loop is chosen by (the default step's loop reads it), t's
// pointer, and the three ints of its first index (gb: the gather blocks in front, the launcher's count;
// nblk: the grid, read from the hidden arguments behind the structs when taken from gridDim) -- preloaded
// into SGPRs at wave launch by the kernel-argument preload these files are built with (docs/DESIGN.md
// section 8c). 13 dwords: the fp32 gradient's pointer has no room among them, so the fp32-gradient loop
// requests p / m / v and t first and fetches a.grad beside them. mnist_adam_launch alone forms these
// arguments, from the structs' own values (p0 = o.p, m0 = o.m, v0 = o.v, gbf0 = o.gbf, t0 = o.t); the
// fc-region loops address their loads through them, everything behind the first loads reads the structs as before. (The
// structs are not copied with the fields overwritten, as mnist.hip's kernels do with MnistStepArgs: a
// copy of the scheduled variant's LrSchedule, indexed at run time, would live in scratch.)
template <class Opt>
__global__ __launch_bounds__(MAD_NT) void mnist_adam_kernel(const float* p0, const float* m0, const float* v0,
                                                            const uint16_t* gbf0, const int64_t* t0, int gb,
                                                            int nblk, int fcb4, MnistStepArgs a, Opt oo) {
  const auto& o = tail_args(oo);
  const auto em = ema_of(oo);
  if ((int)blockIdx.x < gb) {  // the next step's batch; t = the step started next
    gather_next(a, *t0, blockIdx.x);
    return;
  }
  const int grid = nblk - gb;
  // grid == MAD_CONV: the conv region only; the last conv2 block bumps the step
  if (grid == MAD_CONV && (int)blockIdx.x - gb == grid - 1 && threadIdx.x == 0) *o.step += 1;
  // t (a dependent load of the head's step counter) is awaited only where the update needs it,
  // after this thread's first operand loads are out (the optimizer's first memory round trip)
  auto lr_of = [&](const int64_t t) __attribute__((always_inline)) {  // (a call would wait for every load in flight)
    const float b1p = powf(o.beta1, (float)t), b2p = powf(o.beta2, (float)t);
    return TailRates<decltype(ema_omd(em, t))>{base_lr(o, t) * sqrtf(1.f - b2p) / (1.f - b1p), ema_omd(em, t)};
  };
  // (c1 / c2 are formed in each branch behind its first loads: at the top, their scalar loads of the
  //  argument segment were awaited in front of every block's first vector load)
  const int bid = (int)blockIdx.x - gb, tid = threadIdx.x;
  if (bid < MAD_CONV) {
    // what either conv region's slab loads take from the argument segment, requested together and awaited
    // once (the compiler had sunk conv2's pair behind conv1's wait). t stays behind the reduction, read
    // through its preloaded pointer: requested in front of the slab loads, a uniform load is moved to SGPRs
    // at once, which awaits it before the first slab address
    asm volatile("" ::"s"(a.wg1_slab), "s"(a.wg2_slab), "s"(a.B), "s"(a.wg2_splits));
    __shared__ f32x4 red[MAD_NT];
    const bool one = bid < MAD_C1BLK;
    const int q = one ? tid >> 4 : tid >> 6, x = one ? tid & 15 : tid & 63;
    const int64_t i = one ? (int64_t)bid * 16 + x : MAD_C1F4 + (int64_t)(bid - MAD_C1BLK) * 64 + x;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    if (one) {
      g = slab_sum<16>(reinterpret_cast<const f32x4*>(a.wg1_slab) + i, 832 / 4, 2 * a.B, q, 0);
    } else if (i < MAD_C2END) {
      g = slab_sum<4>(reinterpret_cast<const f32x4*>(a.wg2_slab) + (i - MAD_C1F4), 801 * 64 / 4, a.wg2_splits, q, 0);
    }
    red[tid] = g;
    __syncthreads();
    if (q == 0 && i < MAD_C2END) {
      const int nq = one ? 16 : 4, qs = one ? 16 : 64;
      f32x4 s = red[x];
      for (int k = 1; k < nq; ++k) s += red[k * qs + x];
      const auto r = lr_of(*t0);
      const float c1 = 1.f - o.beta1, c2 = 1.f - o.beta2;
      adam4(o, i, s, r.lr_t, c1, c2, em, r.omd);
    }
  } else {
    const int64_t i0 = fcb4 + (int64_t)(bid - MAD_CONV) * MAD_NT + tid;  // fcb4: MAD_C2END, or the out layer
    const int64_t STRIDE = (int64_t)(grid - MAD_CONV) * MAD_NT;
    // ADAM_U strides' loads issued before any math/store, so U x 56 B per lane are in flight
    // (the one-at-a-time loop leaves the compiler no room: p/m/v stores may alias the next loads;
    // streaming non-temporal loads/stores were +0.9 us: the next step re-reads p/m/v from MALL)
    if (gbf0) {
      constexpr int U = ADAM_U;
      // the first item's p / gbf / m / v and t itself are requested side by side through the preloaded
      // pointers; t is awaited behind them, where the update needs it
      uint2 hf = {};
      f32x4 pf = {}, mf = {}, vf = {};
      decltype(ema_load4(em, 0)) e0{};
      if (i0 < TOTAL / 4) {
        pf = reinterpret_cast<const f32x4*>(p0)[i0];
        hf = reinterpret_cast<const uint2*>(gbf0)[i0];
        mf = reinterpret_cast<const f32x4*>(m0)[i0];
        vf = reinterpret_cast<const f32x4*>(v0)[i0];
      }
      const int64_t t = *t0;
      if (i0 < TOTAL / 4) e0 = ema_load4(em, i0);
      const auto r = lr_of(t);
      const float lr_t = r.lr_t, c1 = 1.f - o.beta1, c2 = 1.f - o.beta2;
      auto upd = [&](const int64_t i, f32x4 p, const uint2 h, f32x4 m, f32x4 v, const decltype(e0)& e)
                     __attribute__((always_inline)) {
        const f32x4 g = f32x4{__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xFFFF0000u),
                              __uint_as_float(h.y << 16), __uint_as_float(h.y & 0xFFFF0000u)};
        m = m + (g - m) * c1;
        v = v + (g * g - v) * c2;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] -= lr_t * m[j] / (sqrtf(v[j]) + o.eps);
        reinterpret_cast<f32x4*>(o.p)[i] = p;
        reinterpret_cast<f32x4*>(o.m)[i] = m;
        reinterpret_cast<f32x4*>(o.v)[i] = v;
        reinterpret_cast<uint2*>(o.pbf)[i] = make_uint2(pack_bf2(p[0], p[1]), pack_bf2(p[2], p[3]));
        ema_store4(em, i, e, r.omd, p);
      };
      if (i0 < TOTAL / 4) upd(i0, pf, hf, mf, vf, e0);
      for (int64_t base = i0 + STRIDE; base < TOTAL / 4; base += STRIDE * U) {
        uint2 h[U];
        f32x4 p[U], m[U], v[U];
        decltype(ema_load4(em, 0)) e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = base + (int64_t)u * STRIDE;
          if (i < TOTAL / 4) {
            p[u] = reinterpret_cast<const f32x4*>(p0)[i];
            h[u] = reinterpret_cast<const uint2*>(gbf0)[i];
            m[u] = reinterpret_cast<const f32x4*>(m0)[i];
            v[u] = reinterpret_cast<const f32x4*>(v0)[i];
            e[u] = ema_load4(em, i);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = base + (int64_t)u * STRIDE;
          if (i < TOTAL / 4) upd(i, p[u], h[u], m[u], v[u], e[u]);
        }
      }
    } else {
      // the first item's p / m / v and t are requested before anything is awaited; the gradient's and the
      // shadow's pointers are scalar loads of the argument segment, requested side by side behind them and
      // awaited once
      const float* const g0 = a.grad;
      f32x4 pf = {}, mf = {}, vf = {}, gf = {};
      decltype(ema_load4(em, 0)) e0{};
      if (i0 < TOTAL / 4) {
        pf = reinterpret_cast<const f32x4*>(p0)[i0];
        mf = reinterpret_cast<const f32x4*>(m0)[i0];
        vf = reinterpret_cast<const f32x4*>(v0)[i0];
      }
      const int64_t t = *t0;
      if (i0 < TOTAL / 4) {
        gf = reinterpret_cast<const f32x4*>(g0)[i0];
        e0 = ema_load4(em, i0);
      }
      const auto r = lr_of(t);
      const float lr_t = r.lr_t, c1 = 1.f - o.beta1, c2 = 1.f - o.beta2;
      if (i0 < TOTAL / 4) adam4_pre(o, i0, pf, mf, vf, gf, lr_t, c1, c2, em, e0, r.omd);
      for (int64_t i = i0 + STRIDE; i < TOTAL / 4; i += STRIDE)
        adam4(o, i, reinterpret_cast<const f32x4*>(g0)[i], lr_t, c1, c2, em, r.omd);
    }
    if (bid == grid - 1 && tid == 0) *o.step += 1;  // see MnistAdamArgs
  }
}

template <class Opt>
inline void mnist_adam_launch(const MnistStepArgs& a, const Opt& o, hipStream_t s, bool fc_region) {
  const int gb = gather_blocks(a);
  const int nblk = gb + MAD_CONV + (fc_region ? MAD_FC_BLOCKS : 0);
  const auto& oa = tail_args(o);
  TFD_LAUNCH(mnist_adam_kernel<<<nblk, MAD_NT, 0, s>>>(oa.p, oa.m, oa.v, oa.gbf, oa.t, gb, nblk, (int)(OFF_WD1 / 4), a, o));
}

}  // namespace
}  // namespace tfd
