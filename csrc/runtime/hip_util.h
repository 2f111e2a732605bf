// Host-side HIP helpers shared by the runtime sources: the error check, move-only owners for
// events and streams, and a guard around stream capture.
#pragma once
#include <c10/util/Exception.h>
#include <hip/hip_runtime.h>

#include <utility>

#define HIP_OK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    TORCH_CHECK(e_ == hipSuccess, #x, " failed: ", hipGetErrorString(e_));                 \
  } while (0)

namespace tfd {

// Owns one hipEvent_t. Default-constructed it is empty; HipEvent(timing) creates the event on the
// current device (timing = false: hipEventDisableTiming, for ordering only).
class HipEvent {
 public:
  HipEvent() = default;
  explicit HipEvent(bool timing) {
    HIP_OK(hipEventCreateWithFlags(&ev_, timing ? hipEventDefault : hipEventDisableTiming));
  }
  HipEvent(HipEvent&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
  HipEvent& operator=(HipEvent&& o) noexcept {
    std::swap(ev_, o.ev_);
    return *this;
  }
  ~HipEvent() {
    if (ev_) (void)hipEventDestroy(ev_);
  }
  operator hipEvent_t() const { return ev_; }

 private:
  hipEvent_t ev_ = nullptr;
};

// Owns one non-blocking hipStream_t (empty until create()).
class HipStream {
 public:
  HipStream() = default;
  static HipStream create() {
    HipStream s;
    HIP_OK(hipStreamCreateWithFlags(&s.s_, hipStreamNonBlocking));
    return s;
  }
  HipStream(HipStream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  HipStream& operator=(HipStream&& o) noexcept {
    std::swap(s_, o.s_);
    return *this;
  }
  ~HipStream() {
    if (s_) (void)hipStreamDestroy(s_);
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// Stream capture in relaxed mode. end() finishes the capture and returns the graph, which the guard
// keeps owning and destroys with itself; a guard destroyed before end() (an exception while
// capturing) ends the capture and discards whatever it produced, leaving the stream usable.
class StreamCapture {
 public:
  explicit StreamCapture(hipStream_t s) : s_(s) {
    HIP_OK(hipStreamBeginCapture(s_, hipStreamCaptureModeRelaxed));
    capturing_ = true;
  }
  StreamCapture(const StreamCapture&) = delete;
  StreamCapture& operator=(const StreamCapture&) = delete;
  ~StreamCapture() {
    if (capturing_) (void)hipStreamEndCapture(s_, &g_);
    if (g_) (void)hipGraphDestroy(g_);
  }
  hipGraph_t end() {
    capturing_ = false;
    HIP_OK(hipStreamEndCapture(s_, &g_));
    return g_;
  }

 private:
  hipStream_t s_;
  hipGraph_t g_ = nullptr;
  bool capturing_ = false;
};

}  // namespace tfd
