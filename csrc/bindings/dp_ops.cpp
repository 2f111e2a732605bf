// Torch ops of the DP-SGD kernels (csrc/mnist_dp.h, csrc/kernels/mnist_dp.hip): tfd::mnist_per_example_norms and
// tfd::dp_noise_flat, the launches MnistEngine makes with set_dp_sgd on, on operands of the caller's. A fragment
// of the `tfd` library. Runs on the caller's current HIP stream.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <tuple>

#include "../mnist_dp.h"
#include "../mnist_layout.h"

namespace tfd {
namespace {

void check_operand(const char* who, const char* name, const at::Tensor& t, at::ScalarType dt, std::initializer_list<int64_t> shape,
                   int device) {
  TORCH_CHECK(t.is_cuda() && (device < 0 || t.get_device() == device), who, name, " must be a GPU tensor on dz2's device");
  TORCH_CHECK(t.scalar_type() == dt, who, name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == at::IntArrayRef(shape.begin(), shape.size()), who, name, " has shape ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), who, name, " must be contiguous");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, who, name, " must be 16-byte aligned");
}

// (sq [B,8], norm [B], c [B]) fp32 of fed rows x [B,784] fp32 and the step's factors p1 [B,14,14,32] bf16, idx1
// (uint8), dz2 [B,14,14,64] bf16, p2 [B,3136] bf16, hd / dh [B,1024] bf16, dlogits [B,10] fp32 and the flat bf16
// parameters pbf. scale: rows of dz2, dh and dlogits with c < 1 are multiplied by c in place.
std::tuple<at::Tensor, at::Tensor, at::Tensor> per_example_norms_op(const at::Tensor& x, const at::Tensor& p1, const at::Tensor& idx1,
                                                                     at::Tensor dz2, const at::Tensor& p2, const at::Tensor& hd,
                                                                     at::Tensor dh, at::Tensor dlogits, const at::Tensor& pbf,
                                                                     double clip, bool scale) {
  using namespace mnist;
  const char* who = "mnist_per_example_norms: ";
  TORCH_CHECK(dz2.dim() == 4 && dz2.size(0) >= 1 && dz2.size(0) <= 65535, who, "dz2 is [B,14,14,64], 1 <= B <= 65535");
  const int64_t B = dz2.size(0);
  const int dev = dz2.is_cuda() ? (int)dz2.get_device() : -1;
  check_operand(who, "dz2", dz2, at::kBFloat16, {B, P1H, P1H, C2}, -1);
  check_operand(who, "x", x, at::kFloat, {B, 784}, dev);
  check_operand(who, "p1", p1, at::kBFloat16, {B, P1H, P1H, C1}, dev);
  check_operand(who, "idx1", idx1, at::kByte, {B, P1H, P1H, C1}, dev);
  check_operand(who, "p2", p2, at::kBFloat16, {B, FEAT}, dev);
  check_operand(who, "hd", hd, at::kBFloat16, {B, HID}, dev);
  check_operand(who, "dh", dh, at::kBFloat16, {B, HID}, dev);
  check_operand(who, "dlogits", dlogits, at::kFloat, {B, NCLS}, dev);
  TORCH_CHECK(pbf.dim() == 1 && pbf.size(0) >= OFF_WD1, who, "pbf is the flat bf16 parameter buffer, at least ", OFF_WD1, " elements");
  check_operand(who, "pbf", pbf, at::kBFloat16, {pbf.size(0)}, dev);
  TORCH_CHECK(std::isfinite(clip) && clip > 0, who, "clip > 0, got ", clip);
  auto sq = at::empty({B, 8}, x.options());
  auto norm = at::empty({B}, x.options());
  auto c = at::empty({B}, x.options());
  DpNormArgs a{};
  a.data = (const float*)x.data_ptr();
  a.n = (int)B;
  a.B = (int)B;
  a.p1 = (const uint16_t*)p1.data_ptr();
  a.idx1 = (const uint8_t*)idx1.data_ptr();
  a.dz2 = (uint16_t*)dz2.data_ptr();
  a.p2 = (const uint16_t*)p2.data_ptr();
  a.hd = (const uint16_t*)hd.data_ptr();
  a.dh = (uint16_t*)dh.data_ptr();
  a.dlogits = (float*)dlogits.data_ptr();
  a.pbf = (const uint16_t*)pbf.data_ptr();
  a.clip = (float)clip;
  a.scale = scale ? 1 : 0;
  a.sq = (float*)sq.data_ptr();
  a.norm = (float*)norm.data_ptr();
  a.c = (float*)c.data_ptr();
  dp_norm(a, c10::hip::getCurrentHIPStream().stream());
  return {sq, norm, c};
}

// grad[j] += amp * z_j over the regions [[beg, end), ...] (int64 [R,2] on the host, R <= 8) of the flat fp32 buffer
// grad, in place; step: the int64 device counter the draws follow
void dp_noise_flat_op(at::Tensor grad, const at::Tensor& regions, double amp, const at::Tensor& step, int64_t seed) {
  const char* who = "dp_noise_flat: ";
  TORCH_CHECK(grad.is_cuda() && grad.scalar_type() == at::kFloat && grad.dim() == 1 && grad.is_contiguous(), who,
              "grad is a flat contiguous fp32 GPU tensor");
  TORCH_CHECK(grad.numel() >= 4 && grad.numel() % 4 == 0 && (reinterpret_cast<uintptr_t>(grad.data_ptr()) & 15) == 0, who,
              "grad holds a multiple of 4 elements and is 16-byte aligned");
  TORCH_CHECK(!regions.is_cuda() && regions.scalar_type() == at::kLong && regions.dim() == 2 && regions.size(1) == 2 &&
                  regions.size(0) >= 1 && regions.size(0) <= 8, who, "regions is a host int64 [R,2], 1 <= R <= 8");
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kLong && step.numel() == 1 && step.get_device() == grad.get_device(), who,
              "step is one int64 on grad's device");
  TORCH_CHECK(std::isfinite(amp), who, "amp must be finite, got ", amp);
  const at::Tensor r = regions.contiguous();
  DpNoiseArgs a{};
  a.grad = (float*)grad.data_ptr();
  a.n = grad.numel();
  a.nreg = (int)r.size(0);
  for (int k = 0; k < a.nreg; ++k) {
    a.beg[k] = r.data_ptr<int64_t>()[2 * k];
    a.end[k] = r.data_ptr<int64_t>()[2 * k + 1];
    TORCH_CHECK(a.beg[k] >= 0 && a.beg[k] <= a.end[k] && a.end[k] <= a.n, who, "region ", k, " is outside [0, ", a.n, ")");
  }
  a.amp = (float)amp;
  a.step = (const int64_t*)step.data_ptr();
  a.seed = (uint32_t)seed;
  dp_noise(a, c10::hip::getCurrentHIPStream().stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("mnist_per_example_norms(Tensor x, Tensor p1, Tensor idx1, Tensor(a!) dz2, Tensor p2, Tensor hd, Tensor(b!) dh, "
        "Tensor(c!) dlogits, Tensor pbf, float clip, bool scale=False) -> (Tensor, Tensor, Tensor)");
  m.impl("mnist_per_example_norms", c10::DispatchKey::CUDA, &per_example_norms_op);
  m.def("dp_noise_flat(Tensor(a!) grad, Tensor regions, float amp, Tensor step, int seed) -> ()");
  m.impl("dp_noise_flat", c10::DispatchKey::CUDA, &dp_noise_flat_op);
}

}  // namespace tfd
