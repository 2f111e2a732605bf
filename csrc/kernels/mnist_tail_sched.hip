// The fused MNIST optimizer tail with a learning-rate schedule evaluated on the device
// (csrc/mnist_tail.h, csrc/lr_schedule.h): the instantiation over MnistAdamArgs, in a code object of
// its own so that mnist.hip's stays what the default (constant-rate) step always ran.
#include "../mnist_tail.h"

namespace tfd {

void mnist_adam_fused_sched(const MnistStepArgs& a, const MnistAdamArgs& o, hipStream_t s, bool fc_region) {
  mnist_adam_launch(a, o, s, fc_region);
}

}  // namespace tfd
