// Host-side checks for the kernel launch wrappers (hipcc-compiled sources: no torch headers here; the
// runtime layer has its own HIP_OK over TORCH_CHECK, csrc/runtime/hip_util.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>

#ifndef HIP_OK
#define HIP_OK(x)                                                                                   \
  do {                                                                                              \
    const hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#x " failed: ") + hipGetErrorString(e_)); \
  } while (0)
#endif

// A kernel launch that raises when the runtime refuses it (too much dynamic LDS, a bad grid): without
// the check a refused launch is silent, the buffers keep the previous step's values and the optimizer
// applies them. The error slot is cleared first so that an earlier, unrelated call's leftover (an
// event query's "not ready") is not blamed on this launch. Host-only: nothing is added to the stream,
// so a captured graph holds the same nodes.
#define TFD_LAUNCH(...)                \
  do {                                 \
    (void)hipGetLastError();           \
    __VA_ARGS__;                       \
    HIP_OK(hipGetLastError());         \
  } while (0)
