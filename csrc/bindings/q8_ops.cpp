// Torch ops of 8-bit Adam (csrc/optim_q8.h, csrc/kernels/optim_q8.hip): tfd::adam8_flat, tfd::q8_encode,
// tfd::q8_decode. A fragment of the `tfd` library, as rules_ops.cpp is. Ops run on the caller's current HIP
// stream. The trailing arguments are read by flat_op_args.h.
#include "../optim_q8.h"
#include "flat_op_args.h"

namespace tfd {
namespace {
using namespace flat_op;  // cur, flat_schedule, step_ptr, flat_mods

template <class F>
void launch(F&& f) {  // the launchers' own checks (alignment) as torch errors
  try {
    f();
  } catch (const std::runtime_error& e) {
    TORCH_CHECK(false, e.what());
  }
}
int q8_kind(const std::string& kind, const char* who) {
  TORCH_CHECK(kind == "m" || kind == "v", who, ": kind is \"m\" (e4m3, target 256) or \"v\" (e5m2, target 32768), got ", kind);
  return kind == "m" ? Q8_M : Q8_V;
}
uint8_t* codes_ptr(const at::Tensor& c, const at::Tensor& like, int64_t n, const char* who, const char* name) {
  TORCH_CHECK(on_device_of(c, like) && c.scalar_type() == at::kByte && c.is_contiguous() && c.numel() == n, who, ": ", name,
              " is a contiguous uint8 tensor of ", n, " elements on the same device");
  return (uint8_t*)c.data_ptr();
}
float* scales_ptr(const at::Tensor& a, const at::Tensor& like, int64_t n, const char* who, const char* name) {
  TORCH_CHECK(on_device_of(a, like) && a.scalar_type() == at::kFloat && a.is_contiguous() && a.numel() == q8_blocks(n), who,
              ": ", name, " is a contiguous fp32 tensor of ceil(n / 256) = ", q8_blocks(n), " elements on the same device");
  return (float*)a.data_ptr();
}

// One update of p and the 8-bit state (m8, am: e4m3 codes and block maxima of m; v8, av: e5m2, of v). guard: with
// its ok == 0 nothing is stored to p, the state, pbf or ema.
void adam8_flat(at::Tensor p, at::Tensor m8, at::Tensor v8, at::Tensor am, at::Tensor av, at::Tensor g,
                c10::optional<at::Tensor> pbf, double lr, double beta1, double beta2, double epsilon,
                c10::optional<at::Tensor> step, int64_t t_offset, double grad_scale, c10::optional<at::Tensor> gscale,
                c10::optional<at::Tensor> ema, double ema_decay, bool ema_num_updates, c10::optional<at::Tensor> guard,
                std::string lr_kind, std::vector<double> lr_params, std::vector<int64_t> lr_boundaries,
                std::vector<double> lr_values) {
  const char* who = "adam8_flat";
  const int64_t n = p.numel();
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat && p.is_contiguous() && n >= 1, who,
              ": p is a contiguous fp32 GPU tensor of at least one element");
  const bool gb = g.scalar_type() == at::kBFloat16;
  TORCH_CHECK(on_device_of(g, p) && (gb || g.scalar_type() == at::kFloat) && g.is_contiguous() && g.numel() == n, who,
              ": g is a contiguous fp32 or bf16 tensor of p's size on p's device");
  TORCH_CHECK(!pbf || (on_device_of(*pbf, p) && pbf->scalar_type() == at::kBFloat16 && pbf->is_contiguous() && pbf->numel() == n),
              who, ": pbf is a contiguous bf16 tensor of p's size on p's device");
  const LrSchedule sc = flat_schedule(lr, lr_kind, lr_params, lr_boundaries, lr_values);
  TORCH_CHECK(sc.kind == LR_CONSTANT || step, who, ": a schedule needs the device step tensor");
  TORCH_CHECK(!ema_num_updates || !ema || step, who, ": ema_num_updates needs the device step tensor");
  Adam8Args a{};
  a.p = (float*)p.data_ptr();
  a.m8 = codes_ptr(m8, p, n, who, "m8");
  a.v8 = codes_ptr(v8, p, n, who, "v8");
  a.am = scales_ptr(am, p, n, who, "am");
  a.av = scales_ptr(av, p, n, who, "av");
  a.g = gb ? nullptr : (const float*)g.data_ptr();
  a.gbf = gb ? (const uint16_t*)g.data_ptr() : nullptr;
  a.pbf = pbf ? (uint16_t*)pbf->data_ptr() : nullptr;
  a.n = n;
  a.sched = sc;
  a.beta1 = (float)beta1;
  a.beta2 = (float)beta2;
  a.eps = (float)epsilon;
  a.step = step_ptr(step, p, who);
  a.t_offset = (int)t_offset;
  a.grad_scale = (float)grad_scale;
  apply_mods(a, flat_mods(who, p, gscale, ema, ema_decay, ema_num_updates, guard, true));
  launch([&] { adam8_apply(a, cur()); });
}

std::tuple<at::Tensor, at::Tensor> q8_encode(at::Tensor x, std::string kind) {
  const char* who = "q8_encode";
  const int k = q8_kind(kind, who);
  const int64_t n = x.numel();
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous() && n >= 1, who,
              ": x is a contiguous fp32 GPU tensor of at least one element");
  at::Tensor codes = at::empty({n}, x.options().dtype(at::kByte));
  at::Tensor absmax = at::empty({q8_blocks(n)}, x.options());
  const Q8CodecArgs a{(float*)x.data_ptr(), (uint8_t*)codes.data_ptr(), (float*)absmax.data_ptr(), n, k};
  launch([&] { q8_encode_launch(a, cur()); });
  return {codes, absmax};
}
at::Tensor q8_decode(at::Tensor codes, at::Tensor absmax, std::string kind) {
  const char* who = "q8_decode";
  const int k = q8_kind(kind, who);
  const int64_t n = codes.numel();
  TORCH_CHECK(codes.is_cuda() && n >= 1, who, ": codes is a GPU tensor of at least one element");
  at::Tensor x = at::empty({n}, codes.options().dtype(at::kFloat));
  const Q8CodecArgs a{(float*)x.data_ptr(), codes_ptr(codes, codes, n, who, "codes"), scales_ptr(absmax, codes, n, who, "absmax"),
                      n, k};
  launch([&] { q8_decode_launch(a, cur()); });
  return x;
}
// the largest grid x waves x 256 of adam8_flat's launch: above it a buffer takes a second pass
int64_t q8_grid_elems() { return (int64_t)q8_max_blocks() * (q8_threads() / 64) * kQ8Block; }
}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("adam8_flat(Tensor(a!) p, Tensor(b!) m8, Tensor(c!) v8, Tensor(d!) am, Tensor(e!) av, Tensor g, Tensor(f!)? pbf, "
        "float lr, float beta1, float beta2, float epsilon, *, Tensor? step=None, int t_offset=1, float grad_scale=1.0, "
        "Tensor? gscale=None, Tensor(g!)? ema=None, float ema_decay=0.0, bool ema_num_updates=False, Tensor? guard=None, "
        "str lr_kind=\"constant\", float[] lr_params=[], int[] lr_boundaries=[], float[] lr_values=[]) -> ()");
  m.impl("adam8_flat", c10::DispatchKey::CUDA, &adam8_flat);
  m.def("q8_encode(Tensor x, str kind) -> (Tensor, Tensor)");
  m.impl("q8_encode", c10::DispatchKey::CUDA, &q8_encode);
  m.def("q8_decode(Tensor codes, Tensor absmax, str kind) -> Tensor");
  m.impl("q8_decode", c10::DispatchKey::CUDA, &q8_decode);
  m.def("q8_grid_elems() -> int");
  m.impl("q8_grid_elems", c10::DispatchKey::CompositeExplicitAutograd, &q8_grid_elems);
}

}  // namespace tfd
