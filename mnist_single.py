'''
Single-process MNIST CNN trainer -- the reference's mnist_single.py on the MI355X-native stack
(/root/reference/mnist_single.py:1-134).

Same constants (learning_rate 0.01, training_iters 4000, batch_size 128, display_step 10,
dropout 0.75), same model (conv5x5x32-pool-conv5x5x64-pool-fc1024-dropout-fc10, N(0,1) init),
same loop (`while step * batch_size < training_iters`, a keep_prob=1 minibatch-loss forward every
display_step), same 50 x 100 validation pass and the same stdout lines. On a GPU it runs the
native HIP engine (one captured hipGraph per step); without one, fp32 PyTorch on the CPU.
Optional overrides: --training_iters --batch_size --learning_rate --optimizer --rmsprop_* --adagrad_init_accum --weight_decay --clip_norm --skip_nonfinite --ema_decay --grad_accum_steps --steps_per_call --device_eval --confusion_matrix --logdir --cpu --data_dir --seed.
'''
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from tensorflow_distributed_amd.models import mnist_cnn as M  # noqa: E402
from tensorflow_distributed_amd.models.mnist_runner import make_runner  # noqa: E402
from tensorflow_distributed_amd.training import checkpoint, inference  # noqa: E402
from tensorflow_distributed_amd.training.step_calls import call_lengths, multiples  # noqa: E402
from tensorflow_distributed_amd.training.optimizers import (AdagradOptimizer, AdamOptimizer, LAMBOptimizer,  # noqa: E402
                                                            LARSOptimizer, RMSPropOptimizer)
from tensorflow_distributed_amd.utils import input_data  # noqa: E402

# Parameters (mnist_single.py:17-21)
learning_rate = 0.01
training_iters = 4000
batch_size = 128
display_step = 10

# Network Parameters (mnist_single.py:23-26)
n_input = 784  # MNIST data input (img shape: 28*28)
n_classes = 10  # MNIST total classes (0-9 digits)
dropout = 0.75  # Dropout, probability to keep units


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--training_iters", type=int, default=training_iters)
    ap.add_argument("--batch_size", type=int, default=batch_size)
    ap.add_argument("--learning_rate", type=float, default=learning_rate)
    ap.add_argument("--display_step", type=int, default=display_step)
    ap.add_argument("--data_dir", default="MNIST_data/")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu", action="store_true", help="force the fp32 PyTorch CPU path")
    ap.add_argument("--no_graph", action="store_true", help="GPU: launch kernels per step (no hipGraph)")
    ap.add_argument("--eval_batches", type=int, default=50)
    ap.add_argument("--train_flag", type=int, default=1, help="1 = train, else evaluation only (mnist_single.py:103)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="GPU compute precision (fp32 = the "
                    "reference's)")
    ap.add_argument("--host_feed", action="store_true", help="GPU: feed every batch from the host (next_batch + "
                    "H2D) instead of the device-resident split with a per-epoch device shuffle")
    ap.add_argument("--clip_norm", type=float, default=0.0, help="tf.clip_by_global_norm on the gradient before "
                    "Adam (GPU: norm and clip factor taken on the device inside the step graph); 0 = off")
    ap.add_argument("--skip_nonfinite", action="store_true", help="non-finite guard: a step whose gradient is not "
                    "finite (an inf / NaN element, or a norm beyond fp32) is skipped -- parameters, optimizer slots and "
                    "moving averages keep their bits (GPU: decided on the device inside the step graph)")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "lamb", "lars", "rmsprop", "adagrad"],
                    help="adam (the reference); lamb / lars, layer-wise optimizers: every variable's update scaled by a "
                    "trust ratio of two per-variable norms; rmsprop / adagrad (tf.train.RMSPropOptimizer / "
                    "AdagradOptimizer)")
    ap.add_argument("--rmsprop_decay", type=float, default=0.9, help="--optimizer rmsprop: decay of the averages")
    ap.add_argument("--rmsprop_momentum", type=float, default=0.0, help="--optimizer rmsprop: momentum")
    ap.add_argument("--rmsprop_epsilon", type=float, default=1e-10, help="--optimizer rmsprop: epsilon")
    ap.add_argument("--rmsprop_centered", type=int, default=0, help="--optimizer rmsprop: 1 = the centered rule")
    ap.add_argument("--adagrad_init_accum", type=float, default=0.1, help="--optimizer adagrad: "
                    "initial_accumulator_value (> 0)")
    ap.add_argument("--weight_decay", type=float, default=-1.0, help="--optimizer lamb / lars: weight decay "
                    "(default: 0 for lamb, 1e-4 for lars)")
    ap.add_argument("--lars_eeta", type=float, default=1e-3, help="--optimizer lars: the trust coefficient")
    ap.add_argument("--layerwise_skip_bias", type=int, default=1, help="--optimizer lamb / lars: 1 = the biases take "
                    "neither the weight decay nor the trust ratio")
    ap.add_argument("--ema_decay", type=float, default=0.0, help="tf.train.ExponentialMovingAverage of the weights, "
                    "updated inside the optimizer after every step; 0 = off")
    ap.add_argument("--ema_num_updates", type=int, default=1, help="--ema_decay: 1 = TF's num_updates=global_step, "
                    "the decay of update t is min(ema_decay, (1 + t) / (10 + t))")
    ap.add_argument("--ema_eval", type=int, default=1, help="--ema_decay: 1 = the final accuracy reads the averages")
    ap.add_argument("--grad_accum_steps", type=int, default=1, help="gradient accumulation: every optimizer step sums "
                    "this many micro-batches of --batch_size rows (GPU: on the device, inside the step graph); steps "
                    "and Iter count optimizer steps of grad_accum_steps * batch_size images; 1 = off")
    ap.add_argument("--steps_per_call", type=int, default=1, help="TF's iterations_per_loop: optimizer steps per host "
                    "round trip. N > 1 replays N steps as one captured graph and reads their losses once per call from "
                    "the device step log; a call also ends at every --display_step multiple (the minibatch-loss forward "
                    "needs the last batch). GPU with the device-resident split only; 1 = one step per call")
    ap.add_argument("--device_eval", action="store_true", help="upload the validation split once and evaluate it on "
                    "the device: the --eval_batches x 100 rows in split order (not next_batch's shuffle: the same mean "
                    "whenever they are the whole split, as the default 50 x 100 are), one record per batch folded by the "
                    "engine (GPU: one replayed graph, one read-back); off = the host-fed loop")
    ap.add_argument("--confusion_matrix", action="store_true", help="--device_eval: print the 10 x 10 confusion matrix "
                    "and the per-class recall and precision of the validation pass")
    ap.add_argument("--logdir", default="", help="write a TF-format checkpoint here after training (with --ema_decay "
                    "it carries <var>/ExponentialMovingAverage) and restore the latest one found here at start")
    a = ap.parse_args(argv)
    if a.ema_decay < 0 or a.ema_decay >= 1:
        ap.error("--ema_decay must be in (0, 1) (0 = off)")
    if a.grad_accum_steps < 1:
        ap.error("--grad_accum_steps must be >= 1 (1 = off)")
    if a.steps_per_call < 1 or a.steps_per_call > 1000:
        ap.error("--steps_per_call must be in [1, 1000] (1 = off)")
    if a.steps_per_call > 1:
        if a.cpu or not torch.cuda.is_available():
            ap.error("--steps_per_call > 1 needs the GPU engine (the CPU path steps from the host)")
        if a.host_feed:
            ap.error("--steps_per_call > 1 with --host_feed: a host-fed batch crosses to the device before every step")
        if a.no_graph:
            ap.error("--steps_per_call > 1 with --no_graph: the steps of a call are one captured graph")
    if a.confusion_matrix and not a.device_eval:
        ap.error("--confusion_matrix is folded by --device_eval: give both")
    step_rows = a.batch_size * a.grad_accum_steps  # images per optimizer step

    # Import MNIST data (mnist_single.py:14-15)
    mnist = input_data.read_data_sets(a.data_dir, one_hot=True, seed=a.seed)
    dev = torch.device("cuda", 0) if (torch.cuda.is_available() and not a.cpu) else torch.device("cpu")
    ema = dict(ema_decay=a.ema_decay, ema_num_updates=bool(a.ema_num_updates)) if a.ema_decay > 0 else {}
    if a.optimizer not in ("lamb", "lars") and a.weight_decay >= 0:
        ap.error("--weight_decay belongs to --optimizer lamb / lars")
    common = dict(clip_norm=a.clip_norm if a.clip_norm > 0 else None, accum_steps=a.grad_accum_steps,
                  skip_nonfinite=bool(a.skip_nonfinite), **ema)
    if a.optimizer in ("lamb", "lars"):
        common.update(skip_bias=bool(a.layerwise_skip_bias), **({} if a.weight_decay < 0 else dict(weight_decay=a.weight_decay)))
    if a.optimizer == "lamb":
        opt = LAMBOptimizer(a.learning_rate, **common)
    elif a.optimizer == "lars":
        opt = LARSOptimizer(a.learning_rate, eeta=a.lars_eeta, **common)
    elif a.optimizer == "rmsprop":
        opt = RMSPropOptimizer(a.learning_rate, a.rmsprop_decay, a.rmsprop_momentum, a.rmsprop_epsilon,
                               bool(a.rmsprop_centered), **common)
    elif a.optimizer == "adagrad":
        opt = AdagradOptimizer(a.learning_rate, a.adagrad_init_accum, **common)
    else:
        opt = AdamOptimizer(a.learning_rate, **common)
    runner = make_runner(a.batch_size, opt, dev, keep_prob=dropout, seed=a.seed,
                         use_graph=not a.no_graph, dtype=a.dtype)
    runner.load_flat(M.flat_from_dict(M.init_params(a.seed)), {}, 0)  # init = initialize_all_variables()
    saver = checkpoint.Saver()
    latest = checkpoint.latest_checkpoint(a.logdir) if a.logdir else None
    if latest:
        runner.load_state_dict_tf(saver.restore(latest))
        print("Restored %s (global step %d)" % (latest, runner.global_step()))
    device_input = dev.type == "cuda" and not a.host_feed
    if device_input:  # upload the split once; batches are gathered on the GPU (no per-step feed)
        runner.set_device_dataset(mnist.train.images, mnist.train.labels, seed=a.seed + 101)

    start_time = time.time()
    train_flag = a.train_flag
    step = 1
    if train_flag == 1:
        if a.steps_per_call > 1:
            # the same steps, --steps_per_call at a time: one replayed graph, one read of the step log
            total = max(0, -(-a.training_iters // step_rows) - 1)  # the steps the loop below would take
            first = runner.global_step()
            runner.set_step_log(1024)
            recs = []
            for k in call_lengths(0, a.steps_per_call, total, multiples(a.display_step, 0, total)):
                runner.train_steps(k)
                recs = runner.read_step_log(first + step, first + step + k - 1)
                step += k
                if (step - 1) % a.display_step == 0:
                    batch_x, batch_y = runner.last_device_batch()
                    loss_sum, _ = runner.evaluate(batch_x, batch_y)
                    print("Iter " + str((step - 1) * step_rows) + ", Minibatch Loss= " + "{:.6f}".format(loss_sum / len(batch_x)))
            if recs:
                print("Last call of %d step(s): training loss %.6f, training accuracy %.4f (dropout on)" % (
                    len(recs), sum(r["loss"] for r in recs) / len(recs),
                    sum(r["correct"] for r in recs) / float(sum(r["rows"] for r in recs))))
        # Keep training until reach max iterations
        while step * step_rows < a.training_iters:
            if device_input:
                runner.train_step(None, None)  # next_batch happens on the device
            else:
                batch_x, batch_y = mnist.train.next_batch(step_rows)
                # Run optimization op (backprop)
                runner.train_step(batch_x, batch_y)
            if step % a.display_step == 0:
                if device_input:
                    batch_x, batch_y = runner.last_device_batch()
                # Calculate batch loss (keep_prob = 1)
                loss_sum, _ = runner.evaluate(batch_x, batch_y)
                loss = loss_sum / len(batch_x)
                print("Iter " + str(step * step_rows) + ", Minibatch Loss= " + "{:.6f}".format(loss))
            step += 1
        print("Optimization Finished!")
        training_end_time = time.time()
        print("--- %s seconds Time for Training ---" % (training_end_time - start_time))
        if a.grad_accum_steps > 1:
            print("%d optimizer steps of %d micro-batches x %d images: %.1f images/sec" % (
                step - 1, a.grad_accum_steps, a.batch_size, (step - 1) * step_rows / max(training_end_time - start_time, 1e-9)))
        if a.skip_nonfinite and runner.skipped_steps() > 0:
            print("--skip_nonfinite skipped %d of %d optimizer steps (gradient not finite)" % (runner.skipped_steps(), step - 1))
        if a.logdir:
            print("Saved %s" % saver.save(a.logdir, runner.state_dict_tf(), global_step=runner.global_step()))
    else:
        training_end_time = start_time
    # Calculate accuracy for 5000 mnist validation images
    nt = a.eval_batches
    use_ema = a.ema_decay > 0 and bool(a.ema_eval)
    if a.ema_decay > 0:
        print("Accuracy from the %s" % ("moving averages (decay %g)" % a.ema_decay if use_ema else "variables"))
    accuracy_arr = []
    if a.device_eval:
        # the split uploaded once, rows in split order; one record per batch of 100 from one call
        runner.set_eval_dataset(mnist.validation.images, mnist.validation.labels)
        recs = runner.evaluate_dataset(0, min(nt * 100, mnist.validation.num_examples), 100, use_ema=use_ema)
        accuracy_arr = [r["correct"] / float(r["rows"]) for r in recs]
    else:
        for counter in range(1, nt + 1):
            val_x, val_y = mnist.validation.next_batch(100)
            _, correct = runner.evaluate(val_x, val_y, use_ema=use_ema)
            accuracy_arr.append(correct / float(len(val_x)))
    mean_accuracy = sum(accuracy_arr) / len(accuracy_arr)
    print("Mean Accuracy : %f" % mean_accuracy)
    if a.confusion_matrix:
        print(inference.format_confusion(inference.merge_records(recs)["confusion"]))
    testing_end_time = time.time()
    print("--- %s seconds Time for Inference ---" % (testing_end_time - training_end_time))
    return 0


if __name__ == '__main__':
    sys.exit(main())
