// Layer-wise optimizers (LAMB, LARS): per-variable trust ratios over the flat parameter buffer. ONE
// definition for the host and the device, as ema.h is for the moving average and lr_schedule.h for the
// rate: the segment record, the two ratio functions, the per-element u of LAMB and the LARS
// accumulator step, and (host only) the builder of the block table the kernels of
// kernels/optim_layerwise.hip are launched over.
//
//   LAMB   m' = m + (g - m)(1 - b1);  v' = v + (g g - v)(1 - b2);  c_t = sqrt(1 - b2^t) / (1 - b1^t)
//          u  = c_t m' / (sqrt(v') + eps) + lambda p
//          r  = |p| / |u|  if |p| > 0 and |u| > 0, else 1;          p' = p - lr r u
//   LARS   r  = eeta |p| / (|g| + lambda |p| + eps)  if |p| > 0 and |g| > 0, else 1
//          accum' = mu accum + lr r (g + lambda p);                   p' = p - accum'
// The norms are over one variable (a segment of the flat buffer). A variable without LW_DECAY uses
// lambda = 0, one without LW_ADAPT uses r = 1. g is the gradient times grad_scale * clip factor.
//
// Segment table: sorted, disjoint, every begin a multiple of 4 (16-byte loads stay aligned), any
// length >= 1, gaps allowed. Block table: grid block b works on `count` elements from `first` of
// segment `seg`; a segment of length L becomes ceil(L / chunk) blocks, all but the last of `chunk`
// elements, so no block straddles two variables, every element of every segment belongs to exactly one
// block, and the table is a function of the segment table and the chunk alone. chunk is a multiple of
// 4, so every block starts on a 16-byte boundary and only a segment's last block has a scalar tail.
//
// Rounding (eps32 = 2^-24, the unit roundoff of fp32). A block's partial sum of squares is fp32: a
// square passes through 1 rounding (the product; 2 where the element is g * multiplier), at most 3 in
// its lane's component accumulator (4 vectors per lane), 2 across the four components, 1 for the
// scalar tail, 6 in the wave butterfly and 2 across the four waves: 15 (16) roundings of non-negative
// terms, so the partial is within 16 eps32 of the exact sum, relatively. The blocks' partials are
// summed in fp64 (nblocks * 2^-53: nothing). The square root halves the relative error and the cast to
// fp32 adds one rounding:
//     |norm_dev - norm| <= 9 eps32 norm                                              (kLwNormUlps)
// for the norm of the fp32 values the kernel squared. LARS squares p and g * mul, which are the
// definition's own operands, so its ratio eeta |p| / (fma(lambda, |p|, |g|) + eps) -- two norms, one
// product, one fma and one add of non-negative terms, one division -- is within
//     (9 + 1 + 9 + 2 + 1) eps32 = 22 eps32, stated as 24 eps32                       (kLwLarsRatioUlps)
// of the fp64 ratio. LAMB squares its own fp32 u, which differs from the fp64 u of the same fp32
// inputs by du, element by element, to first order:
//     |dm'| <= 4 eps32 (|g| + |m|)                g * mul, g - m, * (1 - b1), + m
//     |dv'| <= 5 eps32 (g g + v)                  g * mul twice, g g, - v, * (1 - b2), + v
//     den = sqrt(v') + eps:  |dden| <= |dv'| / (2 sqrt(v')) + 2 eps32 den
//     q = c_t m' / den:      |dq| <= |q| (E_ct + 2 eps32 + |dden| / den) + c_t |dm'| / den
//     u = fma(lambda, p, q): |du| <= |dq| + eps32 |u|
// with E_ct the relative error of c_t: powf is within 16 ulp (the OpenCL bound), 1 - b^t amplifies
// that by b^t / (1 - b^t), and the square root halves it:
//     E_ct = 16 eps32 (b2^t / (2 (1 - b2^t)) + b1^t / (1 - b1^t)) + 4 eps32.
// Then | |u|_dev - |u| | <= 9 eps32 |u| + ||du||_2, and the ratio |p| / |u| is within
//     E_r = (9 + 9 + 1) eps32 + ||du||_2 / |u|                                       (relative)
// and p' = fma(-(lr r), u, p) within lr r (|du| + |u| (E_r + E_lr + eps32)) + eps32 |p'|, E_lr the
// schedule's own error (0 for constant and piecewise rates). The LARS step has |daccum'| <= eps32
// (|accum'| + lr r (3 + 24) |g + lambda p| + lr r 2 (|g| + lambda |p|)) and |dp'| <= |daccum'| + eps32 |p'|.
#pragma once
#include <math.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "lr_schedule.h"  // TFD_HD

namespace tfd {

enum LwFlags : int { LW_DECAY = 1, LW_ADAPT = 2 };
constexpr int kLwChunk = 4096;  // elements per block: 256 lanes x 4 vectors x 4 elements
constexpr int kLwNormUlps = 9;
constexpr int kLwLarsRatioUlps = 24;

struct LwSegment {
  int64_t begin, length;
  int flags;  // LwFlags
};
// grid block -> its piece of a segment
struct LwBlock {
  int64_t first;  // first element (a multiple of 4)
  int seg;        // index into the segment table
  int count;      // 1..chunk elements
};
// segment -> its blocks [block0, block0 + nblocks) of the block table, and its flags
struct LwSegBlocks {
  int block0, nblocks, flags, pad_;
};
struct LwTable {
  std::vector<LwBlock> blocks;
  std::vector<LwSegBlocks> segs;
};

// ---- the ratio functions: fp64 sums of squares in, one fp32 out ----
TFD_HD inline float lw_norm(double sumsq) { return (float)sqrt(sumsq); }
TFD_HD inline float lamb_ratio(double p_sumsq, double u_sumsq, int flags) {
  const float pn = lw_norm(p_sumsq), un = lw_norm(u_sumsq);
  return ((flags & LW_ADAPT) && pn > 0.f && un > 0.f) ? pn / un : 1.f;
}
TFD_HD inline float lars_ratio(double p_sumsq, double g_sumsq, float eeta, float weight_decay, float eps, int flags) {
  const float pn = lw_norm(p_sumsq), gn = lw_norm(g_sumsq);
  if (!((flags & LW_ADAPT) && pn > 0.f && gn > 0.f)) return 1.f;
  const float lambda = (flags & LW_DECAY) ? weight_decay : 0.f;
  return eeta * pn / (fmaf(lambda, pn, gn) + eps);
}

// ---- the per-element updates: the only places that spell them. u, the step and the LARS accumulator
// are explicit fmaf / mul / div, so -ffp-contract cannot reshape them and stage 3 rebuilds stage 1's u
// bit for bit from the stored m', v'. m' and v' are formed once (stage 1) and stored; their inner
// g - m and g g are plain operations on the caller's g = gradient * multiplier, which the device
// compiler may contract with that multiply (fma(gradient, multiplier, -m)) where a host compiler does
// not: inside the bounds above (one rounding fewer), deterministic, and read back by nobody as a formula
// -- but m' on the host and on the device may differ in the last bit when the multiplier is not 1. ----
TFD_HD inline float lamb_ct(float beta1, float beta2, int64_t t) {
  return sqrtf(1.f - powf(beta2, (float)t)) / (1.f - powf(beta1, (float)t));
}
TFD_HD inline float lamb_m(float m, float g, float c1) { return fmaf(g - m, c1, m); }
TFD_HD inline float lamb_v(float v, float g, float c2) { return fmaf(fmaf(g, g, -v), c2, v); }
// u from the NEW slots; lambda is 0 for a variable without LW_DECAY
TFD_HD inline float lamb_u(float p, float m_new, float v_new, float ct, float eps, float lambda) {
  return fmaf(lambda, p, ct * m_new / (sqrtf(v_new) + eps));
}
TFD_HD inline float lamb_step(float p, float u, float lr_r) { return fmaf(-lr_r, u, p); }
// accum' (the rate folded in, as TF1's contrib LARS does); p' = p - accum'
TFD_HD inline float lars_accum(float accum, float p, float g, float mu, float lr_r, float lambda) {
  return fmaf(mu, accum, lr_r * fmaf(lambda, p, g));
}

// ---- host only: the block table ----
// numel >= 0: every segment must also end inside a buffer of that many elements
inline LwTable lw_build_table(const LwSegment* segs, size_t n_segs, int64_t chunk, int64_t numel = -1) {
  auto bad = [](size_t i, const std::string& what) {
    throw std::invalid_argument("layerwise segments: segment " + std::to_string(i) + " " + what);
  };
  if (chunk < 4 || chunk % 4 || chunk > (int64_t)1 << 30) throw std::invalid_argument("layerwise segments: chunk must be a multiple of 4 in [4, 2^30]");
  if (n_segs < 1) throw std::invalid_argument("layerwise segments: at least one segment");
  LwTable t;
  t.segs.reserve(n_segs);
  int64_t prev_end = 0, total_blocks = 0;
  for (size_t i = 0; i < n_segs; ++i) {
    const LwSegment& s = segs[i];
    if (s.length < 1) bad(i, "is empty (length >= 1)");
    if (s.begin < 0 || s.begin % 4) bad(i, "does not begin on a multiple of 4");
    if (s.begin < prev_end) bad(i, i ? "overlaps or precedes its predecessor (sorted, disjoint)" : "begins below 0");
    if (s.length > INT64_MAX - s.begin) bad(i, "overflows");
    if (numel >= 0 && s.begin + s.length > numel) bad(i, "ends outside the buffer");
    if (s.flags & ~(LW_DECAY | LW_ADAPT)) bad(i, "has unknown flags");
    prev_end = s.begin + s.length;
    const int64_t nb = (s.length + chunk - 1) / chunk;
    if (total_blocks + nb > (int64_t)INT32_MAX) bad(i, "needs more than 2^31 - 1 blocks");
    t.segs.push_back(LwSegBlocks{(int)total_blocks, (int)nb, s.flags, 0});
    total_blocks += nb;
  }
  t.blocks.reserve((size_t)total_blocks);
  for (size_t i = 0; i < n_segs; ++i)
    for (int64_t o = 0; o < segs[i].length; o += chunk) {
      const int64_t left = segs[i].length - o;
      t.blocks.push_back(LwBlock{segs[i].begin + o, (int)i, (int)(left < chunk ? left : chunk)});
    }
  return t;
}

}  // namespace tfd
