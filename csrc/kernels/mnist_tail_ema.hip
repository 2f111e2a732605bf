// The fused MNIST optimizer tail with the moving average of the weights (csrc/mnist_tail.h,
// csrc/ema.h): the instantiation over MnistAdamEmaArgs -- the scheduled tail plus the shadow's 4-B load
// and 4-B store per element, in the conv-region blocks and both fc-region loops -- in a code object
// of its own so that mnist.hip's and mnist_tail_sched.hip's stay what the steps without EMA always ran.
#include "../mnist_tail.h"

namespace tfd {

void mnist_adam_fused_ema(const MnistStepArgs& a, const MnistAdamEmaArgs& o, hipStream_t s, bool fc_region) {
  if (!o.ema) mnist_adam_fused(a, o.o, s, fc_region);  // no shadow: the tail itself
  else mnist_adam_launch(a, o, s, fc_region);
}

}  // namespace tfd
