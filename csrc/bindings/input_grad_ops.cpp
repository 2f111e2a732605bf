// Torch op of the input gradient / FGSM kernel (csrc/mnist_input_grad.h, csrc/kernels/mnist_input_grad.hip):
// tfd::mnist_input_grad, the launch MnistEngine makes in input_gradient / fgsm / the adversarial step head,
// on operands of the caller's. A fragment of the `tfd` library. Runs on the caller's current HIP stream.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <tuple>

#include "../mnist_input_grad.h"
#include "../mnist_layout.h"

namespace tfd {
namespace {

void check_operand(const char* name, const at::Tensor& t, at::ScalarType dt, std::initializer_list<int64_t> shape, int device) {
  const char* who = "mnist_input_grad: ";
  TORCH_CHECK(t.is_cuda() && (device < 0 || t.get_device() == device), who, name, " must be a GPU tensor on dz2's device");
  TORCH_CHECK(t.scalar_type() == dt, who, name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == at::IntArrayRef(shape.begin(), shape.size()), who, name, " has shape ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), who, name, " must be contiguous");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, who, name, " must be 16-byte aligned");
}

// (dx [B,784] fp32, xadv [B,784] fp32, yadv [B] int32) of dz2 [B,14,14,64] bf16, p1 [B,14,14,32] bf16, idx1
// [B,14,14,32] uint8, the flat bf16 parameters pbf [>= OFF_WD1], fed rows x [B,784] fp32 and labels y [B] int32;
// rows b < adv_rows are perturbed by eps (adv_rows = -1: all)
std::tuple<at::Tensor, at::Tensor, at::Tensor> input_grad_op(const at::Tensor& dz2, const at::Tensor& p1, const at::Tensor& idx1,
                                                             const at::Tensor& pbf, const at::Tensor& x, const at::Tensor& y,
                                                             double eps, int64_t adv_rows) {
  using namespace mnist;
  TORCH_CHECK(dz2.dim() == 4 && dz2.size(0) >= 1 && dz2.size(0) <= 65535, "mnist_input_grad: dz2 is [B,14,14,64], 1 <= B <= 65535");
  const int64_t B = dz2.size(0);
  const int dev = dz2.is_cuda() ? (int)dz2.get_device() : -1;
  check_operand("dz2", dz2, at::kBFloat16, {B, P1H, P1H, C2}, -1);
  check_operand("p1", p1, at::kBFloat16, {B, P1H, P1H, C1}, dev);
  check_operand("idx1", idx1, at::kByte, {B, P1H, P1H, C1}, dev);
  TORCH_CHECK(pbf.dim() == 1 && pbf.size(0) >= OFF_WD1, "mnist_input_grad: pbf is the flat bf16 parameter buffer, at least ",
              OFF_WD1, " elements");
  check_operand("pbf", pbf, at::kBFloat16, {pbf.size(0)}, dev);
  check_operand("x", x, at::kFloat, {B, 784}, dev);
  check_operand("y", y, at::kInt, {B}, dev);
  TORCH_CHECK(std::isfinite(eps) && eps >= 0, "mnist_input_grad: eps >= 0, got ", eps);
  TORCH_CHECK(adv_rows >= -1 && adv_rows <= B, "mnist_input_grad: adv_rows in [0, B] or -1 (all), got ", adv_rows);
  auto dx = at::empty({B, 784}, x.options());
  auto xadv = at::empty({B, 784}, x.options());
  auto yadv = at::empty({B}, y.options());
  InputGradArgs a{};
  a.dz2 = (const uint16_t*)dz2.data_ptr();
  a.p1 = (const uint16_t*)p1.data_ptr();
  a.idx1 = (const uint8_t*)idx1.data_ptr();
  a.pbf = (const uint16_t*)pbf.data_ptr();
  a.data = (const float*)x.data_ptr();
  a.labels = (const int*)y.data_ptr();
  a.n = (int)B;
  a.B = (int)B;
  a.eps = (float)eps;
  a.adv_rows = (int)(adv_rows < 0 ? B : adv_rows);
  a.dx = (float*)dx.data_ptr();
  a.xadv = (float*)xadv.data_ptr();
  a.yadv = (int*)yadv.data_ptr();
  input_grad(a, c10::hip::getCurrentHIPStream().stream());
  return {dx, xadv, yadv};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("mnist_input_grad(Tensor dz2, Tensor p1, Tensor idx1, Tensor pbf, Tensor x, Tensor y, float eps=0.0, int adv_rows=-1) "
        "-> (Tensor, Tensor, Tensor)");
  m.impl("mnist_input_grad", c10::DispatchKey::CUDA, &input_grad_op);
}

}  // namespace tfd
