// Torch op of the Monte-Carlo dropout head (csrc/mnist_mc.h, csrc/kernels/mnist_mc.hip): tfd::mnist_mc_head, the
// launch MnistEngine.predict_mc makes behind its forward, on hidden-layer slabs of the caller's. A fragment of the
// `tfd` library. Runs on the caller's current HIP stream.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cmath>
#include <tuple>

#include "../mnist_infer.h"
#include "../mnist_layout.h"
#include "../mnist_mc.h"

namespace tfd {
namespace {

// fc1_slab [splits, split_rows, 1024] fp32 (the fc1 split-K partial sums, bias not added), rows = the first
// split_rows rows; p32: the flat fp32 parameters; labels: empty or [rows] int32. Row r draws as global row row0 + r.
// Returns (mean_prob [rows,10], classes [rows] int32, entropy, expected_entropy, mutual_info [rows], var_prob [rows,10],
// loss_row, correct_row [rows] or empty).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> mc_head_op(
    const at::Tensor& fc1_slab, int64_t split_rows, const at::Tensor& p32, const at::Tensor& labels, int64_t samples,
    double keep_prob, int64_t seed, int64_t rank, int64_t row0) {
  using namespace mnist;
  const char* who = "mnist_mc_head: ";
  TORCH_CHECK(fc1_slab.is_cuda() && fc1_slab.scalar_type() == at::kFloat && fc1_slab.dim() == 3 && fc1_slab.is_contiguous() &&
                  fc1_slab.size(2) == HID, who, "fc1_slab is a contiguous fp32 GPU tensor [splits, split_rows, 1024]");
  TORCH_CHECK(fc1_slab.size(0) >= 1 && fc1_slab.size(0) <= kInferMaxSplits, who, "1 <= splits <= ", kInferMaxSplits);
  TORCH_CHECK(split_rows >= 1 && split_rows == fc1_slab.size(1) && split_rows <= 65535, who, "split_rows is fc1_slab's second extent, 1 .. 65535");
  TORCH_CHECK(p32.is_cuda() && p32.get_device() == fc1_slab.get_device() && p32.scalar_type() == at::kFloat && p32.dim() == 1 &&
                  p32.is_contiguous() && p32.size(0) >= OFF_BOUT + NCLS, who, "p32 is the flat fp32 parameter buffer on fc1_slab's device");
  const int64_t rows = split_rows;
  const bool labelled = labels.numel() > 0;
  if (labelled)
    TORCH_CHECK(labels.is_cuda() && labels.get_device() == fc1_slab.get_device() && labels.scalar_type() == at::kInt &&
                    labels.dim() == 1 && labels.is_contiguous() && labels.size(0) == rows, who, "labels is empty or int32 [rows]");
  TORCH_CHECK(samples >= 1 && samples <= kMcMaxSamples, who, "1 <= samples <= ", kMcMaxSamples, ", got ", samples);
  TORCH_CHECK(std::isfinite(keep_prob) && keep_prob > 0 && keep_prob <= 1, who, "0 < keep_prob <= 1, got ", keep_prob);
  TORCH_CHECK(row0 >= 0, who, "row0 >= 0");
  auto f = fc1_slab.options();
  auto mean_prob = at::empty({rows, NCLS}, f), var_prob = at::empty({rows, NCLS}, f);
  auto classes = at::empty({rows}, f.dtype(at::kInt));
  auto entropy = at::empty({rows}, f), expected = at::empty({rows}, f), mi = at::empty({rows}, f);
  auto loss = at::empty({labelled ? rows : 0}, f), correct = at::empty({labelled ? rows : 0}, f);
  McHeadArgs a{};
  a.rows = (int)rows;
  a.fc1_slab = (const float*)fc1_slab.data_ptr();
  a.splits = (int)fc1_slab.size(0);
  a.split_rows = (int)split_rows;
  a.p32 = (const float*)p32.data_ptr();
  a.labels = labelled ? (const int*)labels.data_ptr() : nullptr;
  a.samples = (int)samples;
  a.keep_prob = (float)keep_prob;
  a.seed = (uint32_t)seed;
  a.rank = (uint32_t)rank;
  a.row0 = (uint64_t)row0;
  a.mean_prob = (float*)mean_prob.data_ptr();
  a.classes = (int*)classes.data_ptr();
  a.entropy = (float*)entropy.data_ptr();
  a.expected_entropy = (float*)expected.data_ptr();
  a.mutual_info = (float*)mi.data_ptr();
  a.var_prob = (float*)var_prob.data_ptr();
  a.loss_row = labelled ? (float*)loss.data_ptr() : nullptr;
  a.correct_row = labelled ? (float*)correct.data_ptr() : nullptr;
  mc_head(a, c10::hip::getCurrentHIPStream().stream());
  return {mean_prob, classes, entropy, expected, mi, var_prob, loss, correct};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(tfd, m) {
  m.def("mnist_mc_head(Tensor fc1_slab, int split_rows, Tensor p32, Tensor labels, int samples, float keep_prob, int seed, "
        "int rank, int row0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.impl("mnist_mc_head", c10::DispatchKey::CUDA, &mc_head_op);
}

}  // namespace tfd
