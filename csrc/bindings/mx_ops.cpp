// Torch ops of the block-scaled fc1 forward (csrc/mnist_mx.h, csrc/kernels/mnist_mx.hip): tfd::mx_pack_fc1 and
// tfd::mnist_fc1_mx, the two launches MnistEngine makes in an MX inference format, on tensors of the caller's.
// A fragment of the `tfd` library. Runs on the caller's current HIP stream.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <string>

#include "../mnist_layout.h"
#include "../mnist_mx.h"

namespace tfd {
namespace {

int mx_format(const char* who, const std::string& fmt) {
  TORCH_CHECK(fmt == "mxfp8" || fmt == "mxfp4", who, "fmt is 'mxfp8' or 'mxfp4', got '", fmt, "'");
  return fmt == "mxfp4" ? MX_FP4 : MX_FP8;
}

// w: W1 [3136, 1024] fp32. Returns the packed image, uint8 [mx_packed_bytes(fmt)] (codes, then scales).
at::Tensor mx_pack_fc1_op(const at::Tensor& w, const std::string& fmt) {
  using namespace mnist;
  const char* who = "mx_pack_fc1: ";
  const int f = mx_format(who, fmt);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 2 && w.is_contiguous() && w.size(0) == FEAT &&
                  w.size(1) == HID, who, "w is a contiguous fp32 GPU tensor [3136, 1024]");
  auto packed = at::empty({(int64_t)mx_packed_bytes(f)}, w.options().dtype(at::kByte));
  mx_pack_fc1((const float*)w.data_ptr(), (uint8_t*)packed.data_ptr(), f, c10::hip::getCurrentHIPStream().stream());
  return packed;
}

// p2: [rows, 3136] bf16, packed: mx_pack_fc1's image in the same fmt. Returns the split-K slabs [7, rows, 1024] fp32.
at::Tensor fc1_mx_op(const at::Tensor& p2, const at::Tensor& packed, const std::string& fmt) {
  using namespace mnist;
  const char* who = "mnist_fc1_mx: ";
  const int f = mx_format(who, fmt);
  TORCH_CHECK(p2.is_cuda() && p2.scalar_type() == at::kBFloat16 && p2.dim() == 2 && p2.is_contiguous() && p2.size(1) == FEAT,
              who, "p2 is a contiguous bf16 GPU tensor [rows, 3136]");
  TORCH_CHECK(p2.size(0) >= 1 && p2.size(0) <= 65535, who, "1 <= rows <= 65535, got ", p2.size(0));
  TORCH_CHECK(packed.is_cuda() && packed.get_device() == p2.get_device() && packed.scalar_type() == at::kByte && packed.dim() == 1 &&
                  packed.is_contiguous() && packed.size(0) == (int64_t)mx_packed_bytes(f),
              who, "packed is mx_pack_fc1's uint8 image in format ", fmt, " (", mx_packed_bytes(f), " bytes) on p2's device");
  auto slab = at::empty({kMxSplits, p2.size(0), HID}, p2.options().dtype(at::kFloat));
  MxFc1Args a{};
  a.rows = (int)p2.size(0);
  a.p2 = (const uint16_t*)p2.data_ptr();
  a.packed = (const uint8_t*)packed.data_ptr();
  a.slab = (float*)slab.data_ptr();
  mx_fc1_fwd(a, f, c10::hip::getCurrentHIPStream().stream());
  return slab;
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("mx_pack_fc1(Tensor w, str fmt) -> Tensor");
  m.impl("mx_pack_fc1", c10::DispatchKey::CUDA, &mx_pack_fc1_op);
  m.def("mnist_fc1_mx(Tensor p2, Tensor packed, str fmt) -> Tensor");
  m.impl("mnist_fc1_mx", c10::DispatchKey::CUDA, &fc1_mx_op);
}

}  // namespace tfd
