// Probe pair for the cost of a kernel's first kernel-argument fetch (tools/debug/kernarg_probe.py,
// docs/DESIGN.md section 8c). Both kernels do the same work: every lane issues ONE vector load whose
// address comes from an argument, adds one and stores. They differ only in how the pointers arrive:
//   kernarg_probe_struct   through a 320-byte by-value struct (the shape of MnistStepArgs: five 64-B
//                          lines of the argument segment), the source pointer in its third line: the
//                          wave's first instruction is a scalar load, the vector load waits for it;
//   kernarg_probe_preload  as leading pointer parameters, which this file's build flag
//                          (-amdgpu-kernarg-preload-count) has the packet processor place in SGPRs at
//                          wave launch: the vector load is issued with no scalar wait in front.
// The struct follows the preloaded pointers too, so both argument segments have the same size.
#include "../common.h"
#include "../tfd_kernels.h"

namespace tfd {
namespace {
struct ProbeArgs {  // 320 B
  int64_t pad0[17];
  const float* src;  // offset 0x88 (MnistStepArgs::fc1_slab's)
  int64_t pad1[21];
  float* dst;        // offset 0x138, the last line
};
static_assert(sizeof(ProbeArgs) == 320, "the probe's struct spans five 64-B lines");
__global__ __launch_bounds__(64) void kernarg_probe_struct(ProbeArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  a.dst[i] = a.src[i] + 1.f;
}
__global__ __launch_bounds__(64) void kernarg_probe_preload(const float* src, float* dst, ProbeArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  dst[i] = src[i] + 1.f;
  (void)a;
}
}  // namespace

void kernarg_probe(const float* src, float* dst, int blocks, bool preload, hipStream_t s) {
  ProbeArgs a{};
  a.src = src;
  a.dst = dst;
  if (preload) kernarg_probe_preload<<<blocks, 64, 0, s>>>(src, dst, a);
  else kernarg_probe_struct<<<blocks, 64, 0, s>>>(a);
}
}  // namespace tfd
