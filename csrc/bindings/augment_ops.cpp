// Torch op of the device data augmentation (csrc/mnist_augment.h, csrc/kernels/mnist_augment.hip):
// tfd::augment_batch, the launch MnistEngine makes at the head of a training step, on operands of the
// caller's. A fragment of the `tfd` library. Runs on the caller's current HIP stream.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <limits>
#include <stdexcept>
#include <tuple>

#include "../mnist_augment.h"

namespace tfd {
namespace {

// (x [B,784] fp32, y [B] int32): batch `step` of B rows of data [n,784] / labels [n] through perm [n]
// (checked here to hold row numbers: one synchronisation), warped by the draws of (seed, rank, step, b)
std::tuple<at::Tensor, at::Tensor> augment_batch_op(const at::Tensor& data, const at::Tensor& labels, const at::Tensor& perm,
                                                    int64_t step, int64_t B, int64_t seed, int64_t rank, double shift_px,
                                                    double rotate_deg, double scale, double elastic_alpha,
                                                    double elastic_sigma) {
  const char* who = "augment_batch";
  TORCH_CHECK(data.is_cuda() && data.scalar_type() == at::kFloat && data.dim() == 2 && data.size(1) == 784 &&
                  data.size(0) >= 1 && data.is_contiguous(),
              who, ": data is a contiguous [n,784] fp32 GPU tensor, n >= 1");
  const int64_t n = data.size(0);
  TORCH_CHECK(n <= std::numeric_limits<int>::max(), who, ": n fits an int32");
  for (const at::Tensor* t : {&labels, &perm})
    TORCH_CHECK(t->is_cuda() && t->get_device() == data.get_device() && t->scalar_type() == at::kInt && t->dim() == 1 &&
                    t->size(0) == n && t->is_contiguous(),
                who, ": labels and perm are contiguous [n] int32 tensors on data's device");
  TORCH_CHECK(step >= 0 && B >= 1 && B <= 65535, who, ": step >= 0 and 1 <= B <= 65535, got ", step, " and ", B);
  TORCH_CHECK(step <= (std::numeric_limits<int64_t>::max() - B) / B, who, ": step * B + B overflows int64");
  TORCH_CHECK(perm.min().item<int64_t>() >= 0 && perm.max().item<int64_t>() < n, who, ": perm holds row numbers in [0, n)");
  AugmentArgs a{};
  try {
    a.cfg = make_augment_config(shift_px, rotate_deg, scale, elastic_alpha, elastic_sigma);
  } catch (const std::invalid_argument& e) {
    TORCH_CHECK(false, e.what());
  }
  auto cursor = at::full({1}, step, data.options().dtype(at::kLong));
  auto x = at::empty({B, 784}, data.options());
  auto y = at::empty({B}, labels.options());
  a.data = (const float*)data.data_ptr();
  a.labels = (const int*)labels.data_ptr();
  a.perm = (const int*)perm.data_ptr();
  a.step = (const int64_t*)cursor.data_ptr();
  a.n = (int)n;
  a.B = (int)B;
  a.seed = (uint32_t)seed;
  a.rank = (uint32_t)rank;
  a.xaug = (float*)x.data_ptr();
  a.yaug = (int*)y.data_ptr();
  augment_batch(a, c10::hip::getCurrentHIPStream().stream());
  return {x, y};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("augment_batch(Tensor data, Tensor labels, Tensor perm, int step, int B, int seed, int rank, float shift_px=0.0, "
        "float rotate_deg=0.0, float scale=0.0, float elastic_alpha=0.0, float elastic_sigma=0.0) -> (Tensor, Tensor)");
  m.impl("augment_batch", c10::DispatchKey::CUDA, &augment_batch_op);
}

}  // namespace tfd
