// Host-side check of csrc/optim_launch.h, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_optim_launch_cpu.py: the variant table over the 8 combinations of (clip, ema, guard) against
// a table written out here, what every built wrapper carries for Adam and SGD, the refusals (a variant that
// needs the device 1.0f and has none, the guard on the ranges form), and apply_mods on RuleArgs and
// LayerwiseArgs. Only the header's inline part: no launcher is called, none is linked.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "../../csrc/layerwise_kernels.h"
#include "../../csrc/optim_launch.h"
#include "../../csrc/optim_rules.h"

using namespace tfd;

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++failures;                                                    \
    }                                                                \
  } while (0)

template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return true;
  }
  return false;
}
template <class T>
static bool same_bytes(const T& a, const T& b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// the table, written out: index = clip + 2 * ema + 4 * guard
static const OptVariant kTable[8] = {
    OptVariant::Plain,     // -     -    -
    OptVariant::Clip,      // clip  -    -
    OptVariant::Ema,       // -     ema  -
    OptVariant::Ema,       // clip  ema  -
    OptVariant::Guard,     // -     -    guard
    OptVariant::Guard,     // clip  -    guard
    OptVariant::EmaGuard,  // -     ema  guard
    OptVariant::EmaGuard,  // clip  ema  guard
};
static_assert(opt_variant(false, false, false) == OptVariant::Plain && opt_variant(true, true, true) == OptVariant::EmaGuard,
              "opt_variant is usable in constant expressions");

// stand-ins for device memory: the builders copy the pointers and never read through them
static float g_gscale, g_ok, g_one, g_shadow[4], g_buf[16];
static int64_t g_step;

static OptMods mods_of(bool clip, bool ema, bool guard, bool with_one = true) {
  OptMods m;
  if (clip) m.gscale = &g_gscale;
  if (guard) m.ok = &g_ok;
  if (ema) {
    m.ema = g_shadow + 1;
    m.ema_decay = 0.875f;
    m.ema_num_updates = 1;
  }
  if (with_one) m.one = &g_one;
  return m;
}

template <class E>
static void check_ema(const E& e, const OptMods& m) {
  CHECK(e.ema == m.ema && e.decay == m.ema_decay && e.num_updates == m.ema_num_updates);
}

// every wrapper of every combination, for A = AdamArgs or SgdArgs
template <class A>
static void check_wrappers(const A& a) {
  for (int i = 0; i < 8; ++i) {
    const bool clip = i & 1, ema = i & 2, guard = i & 4;
    const OptMods m = mods_of(clip, ema, guard);
    CHECK(opt_variant(clip, ema, guard) == kTable[i]);
    CHECK(opt_variant(m) == kTable[i]);
    const float* want_gscale = clip ? &g_gscale : &g_one;
    switch (kTable[i]) {
      case OptVariant::Plain:
        break;  // the bare struct is launched as it is
      case OptVariant::Clip: {
        const auto k = opt_clip_args(a, m);
        CHECK(same_bytes(k.a, a) && k.gscale == want_gscale);
        break;
      }
      case OptVariant::Ema: {
        const auto e = opt_ema_args(a, m);
        CHECK(same_bytes(e.k.a, a) && e.k.gscale == want_gscale);
        check_ema(e, m);
        break;
      }
      case OptVariant::Guard: {
        const auto g = opt_guard_args(a, m);
        CHECK(same_bytes(g.k.a, a) && g.k.gscale == want_gscale && g.ok == &g_ok);
        break;
      }
      case OptVariant::EmaGuard: {
        const auto g = opt_ema_guard_args(a, m);
        CHECK(same_bytes(g.k.k.a, a) && g.k.k.gscale == want_gscale && g.ok == &g_ok);
        check_ema(g.k, m);
        break;
      }
    }
    // a variant that reads a clip factor and has neither the step's nor the device 1.0f
    const OptMods bare = mods_of(clip, ema, guard, false);
    CHECK(throws([&] { opt_clip_args(a, bare); }) == !clip);
    CHECK(throws([&] { opt_ema_args(a, bare); }) == !clip);
    CHECK(throws([&] { opt_guard_args(a, bare); }) == !clip);
    CHECK(throws([&] { opt_ema_guard_args(a, bare); }) == !clip);
    // the ranges form: the table without the guard, a refusal with it
    if (guard) CHECK(throws([&] { opt_ranges_variant(m); }));
    else CHECK(opt_ranges_variant(m) == kTable[i]);
  }
}

template <class A>
static void check_apply_mods() {
  for (int i = 0; i < 8; ++i) {
    const bool clip = i & 1, ema = i & 2, guard = i & 4;
    const OptMods m = mods_of(clip, ema, guard);
    A a, want;
    std::memset(&a, 0, sizeof(A));
    std::memset(&want, 0, sizeof(A));
    apply_mods(a, m);
    CHECK(a.gscale == (clip ? &g_gscale : &g_one));
    CHECK(a.ok == (guard ? &g_ok : nullptr));
    CHECK(a.ema == (ema ? g_shadow + 1 : nullptr));
    CHECK(a.ema_decay == (ema ? 0.875f : 0.f) && a.ema_num_updates == (ema ? 1 : 0));
    // the five fields and nothing else: put them back and the struct is the zero-initialised one
    a.gscale = nullptr;
    a.ok = nullptr;
    a.ema = nullptr;
    a.ema_decay = 0.f;
    a.ema_num_updates = 0;
    CHECK(same_bytes(a, want));
    A b;
    std::memset(&b, 0, sizeof(A));
    CHECK(throws([&] { apply_mods(b, mods_of(clip, ema, guard, false)); }) == !clip);
  }
}

int main() {
  // zeroed first, so the padding compares equal too
  AdamArgs adam;
  std::memset(&adam, 0, sizeof(adam));
  adam.p = g_buf;
  adam.m = g_buf + 4;
  adam.v = g_buf + 8;
  adam.g = g_buf + 12;
  adam.n = 4;
  adam.sched = lr_constant(0.125f);
  adam.sched.kind = LR_EXPONENTIAL;
  adam.sched.rate = 0.5f;
  adam.beta1 = 0.75f;
  adam.beta2 = 0.875f;
  adam.eps = 0.25f;
  adam.step = &g_step;
  adam.t_offset = 3;
  adam.grad_scale = 0.5f;
  check_wrappers(adam);

  SgdArgs sgd;
  std::memset(&sgd, 0, sizeof(sgd));
  sgd.p = g_buf;
  sgd.mom = g_buf + 4;
  sgd.g = g_buf + 8;
  sgd.n = 4;
  sgd.sched = lr_constant(0.25f);
  sgd.momentum = 0.5f;
  sgd.weight_decay = 0.125f;
  sgd.grad_scale = 2.f;
  sgd.nesterov = 1;
  sgd.step = &g_step;
  sgd.t_offset = 1;
  check_wrappers(sgd);

  check_apply_mods<RuleArgs>();
  check_apply_mods<LayerwiseArgs>();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
