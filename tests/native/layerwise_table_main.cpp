// Host-side check of csrc/layerwise.h, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_layerwise_table_cpu.py: the block table of ragged, gapped, 300-segment and MNIST segment
// tables at several chunk sizes (every element of every segment covered exactly once, no block across
// two segments, none in a gap), the builder's refusals, and the guards of the ratio functions.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../csrc/layerwise.h"

using namespace tfd;

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static std::vector<LwSegment> table(const std::vector<int64_t>& lengths, const std::vector<int64_t>& gaps) {
  std::vector<LwSegment> s;
  int64_t pos = 0;
  for (size_t i = 0; i < lengths.size(); ++i) {
    s.push_back(LwSegment{pos, lengths[i], (int)(i % 4)});
    pos = (pos + lengths[i] + 3) / 4 * 4 + gaps[i % gaps.size()];
  }
  return s;
}

static void check_table(const std::vector<LwSegment>& segs, int64_t chunk) {
  const int64_t numel = segs.back().begin + segs.back().length + 5;
  const LwTable t = lw_build_table(segs.data(), segs.size(), chunk, numel);
  CHECK(t.segs.size() == segs.size());
  std::vector<unsigned char> cover((size_t)numel, 0);
  for (size_t b = 0; b < t.blocks.size(); ++b) {
    const LwBlock& k = t.blocks[b];
    CHECK(k.seg >= 0 && (size_t)k.seg < segs.size());
    const LwSegment& s = segs[(size_t)k.seg];
    CHECK(k.count >= 1 && k.count <= chunk && k.first % 4 == 0);
    CHECK(k.first >= s.begin && k.first + k.count <= s.begin + s.length);  // inside ONE segment: no gap, no straddle
    const LwSegBlocks& r = t.segs[(size_t)k.seg];
    CHECK((int64_t)b >= r.block0 && (int64_t)b < (int64_t)r.block0 + r.nblocks);
    CHECK(k.count == chunk || (int64_t)b == (int64_t)r.block0 + r.nblocks - 1);  // only a segment's last block is short
    for (int64_t e = k.first; e < k.first + k.count; ++e) ++cover[(size_t)e];
  }
  std::vector<unsigned char> want((size_t)numel, 0);
  int64_t blocks = 0;
  for (size_t i = 0; i < segs.size(); ++i) {
    for (int64_t e = segs[i].begin; e < segs[i].begin + segs[i].length; ++e) want[(size_t)e] = 1;
    CHECK(t.segs[i].block0 == blocks && t.segs[i].flags == segs[i].flags);
    CHECK(t.segs[i].nblocks == (segs[i].length + chunk - 1) / chunk);
    blocks += t.segs[i].nblocks;
  }
  CHECK((size_t)blocks == t.blocks.size());
  CHECK(cover == want);  // exactly once inside the segments, never outside
  // a function of the table and the chunk alone
  const LwTable again = lw_build_table(segs.data(), segs.size(), chunk);
  CHECK(again.blocks.size() == t.blocks.size());
  for (size_t b = 0; b < t.blocks.size(); ++b)
    CHECK(again.blocks[b].first == t.blocks[b].first && again.blocks[b].seg == t.blocks[b].seg &&
          again.blocks[b].count == t.blocks[b].count);
}

template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main() {
  const int64_t c = kLwChunk;
  const std::vector<LwSegment> ragged = table({1, 3, 4, 5, 255, c - 1, c, c + 1, 3 * c + 2}, {0, 4, 8, 0, 12});
  const std::vector<LwSegment> ones = table(std::vector<int64_t>(16, 1), {0});
  std::vector<int64_t> l300;
  for (int i = 0; i < 300; ++i) l300.push_back((37 * i) % 301 + 1);
  const std::vector<LwSegment> s300 = table(l300, {0, 4, 8, 0, 12});
  const std::vector<LwSegment> mnist = {{0, 800, 3},       {800, 32, 0},      {832, 51200, 3},    {52032, 64, 0},
                                        {52096, 3211264, 3}, {3263360, 1024, 0}, {3264384, 10240, 3}, {3274624, 10, 0}};
  for (int64_t chunk : {(int64_t)4, (int64_t)8, (int64_t)256, c, 4 * c}) {
    check_table(ragged, chunk);
    check_table(ones, chunk);
    check_table(s300, chunk);
  }
  for (int64_t chunk : {(int64_t)256, c, 4 * c}) check_table(mnist, chunk);
  CHECK(lw_build_table(mnist.data(), mnist.size(), c).blocks.size() == 1 + 1 + 13 + 1 + 784 + 1 + 3 + 1);

  auto build = [&](std::vector<LwSegment> s, int64_t chunk = kLwChunk, int64_t numel = -1) {
    return [=] { lw_build_table(s.data(), s.size(), chunk, numel); };
  };
  CHECK(throws(build({{8, 4, 3}, {0, 4, 3}})));   // unsorted
  CHECK(throws(build({{0, 8, 3}, {4, 4, 3}})));   // overlapping
  CHECK(throws(build({{2, 4, 3}})));              // misaligned
  CHECK(throws(build({{0, 0, 3}})));              // empty
  CHECK(throws(build({{0, -4, 3}})));
  CHECK(throws(build({{-4, 4, 3}})));
  CHECK(throws(build({{0, 4, 8}})));              // unknown flag
  CHECK(throws(build({})));                       // no segment
  CHECK(throws(build({{0, 4, 3}}, 6)));           // chunk not a multiple of 4
  CHECK(throws(build({{0, 4, 3}}, 0)));
  CHECK(throws(build({{0, 8, 3}}, kLwChunk, 7))); // ends outside the buffer
  CHECK(!throws(build({{0, 8, 3}}, kLwChunk, 8)));
  CHECK(!throws(build({{0, 5, 3}, {8, 1, 0}})));  // gaps and any length are fine

  // ratio guards
  CHECK(lamb_ratio(1024.0, 4096.0, LW_ADAPT) == 0.5f);
  CHECK(lamb_ratio(0.0, 4096.0, LW_ADAPT) == 1.f && lamb_ratio(1024.0, 0.0, LW_ADAPT) == 1.f);
  CHECK(lamb_ratio(1024.0, 4096.0, LW_DECAY) == 1.f);  // not adapted
  CHECK(lars_ratio(1024.0, 256.0, 0.125f, 0.f, 0.f, LW_ADAPT | LW_DECAY) == 0.25f);
  CHECK(lars_ratio(1024.0, 256.0, 0.125f, 0.5f, 0.f, LW_ADAPT | LW_DECAY) == 0.125f);
  CHECK(lars_ratio(1024.0, 256.0, 0.125f, 0.5f, 0.f, LW_ADAPT) == 0.25f);  // not decayed: lambda = 0
  CHECK(lars_ratio(0.0, 256.0, 0.125f, 0.5f, 0.f, 3) == 1.f && lars_ratio(1024.0, 0.0, 0.125f, 0.5f, 0.f, 3) == 1.f);
  CHECK(lars_ratio(1024.0, 256.0, 0.125f, 0.5f, 0.f, LW_DECAY) == 1.f);
  // the per-element helpers on the exact cases of the GPU tests
  CHECK(lamb_ct(0.5f, 0.75f, 1) == 1.f);
  const float m = lamb_m(0.f, 0.25f, 0.5f), v = lamb_v(0.f, 0.25f, 0.25f);
  CHECK(m == 0.125f && v == 0.015625f);
  CHECK(lamb_u(0.5f, m, v, 1.f, 0.f, 0.f) == 1.f && lamb_step(0.5f, 1.f, 0.25f * 0.5f) == 0.375f);
  CHECK(lars_accum(0.f, 0.5f, 0.25f, 0.f, 0.5f * 0.25f, 0.f) == 0.03125f);
  CHECK(lars_accum(0.f, 0.5f, 0.25f, 0.f, 0.5f * 0.125f, 0.5f) == 0.03125f);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
