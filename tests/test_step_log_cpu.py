"""Step log, the parts that need no GPU: the cut points of --steps_per_call (one pure function, checked
against a step-by-step simulation), the CPU runner's three methods (train_steps(4) against four
train_step calls) and the start-up refusals of the driver flag."""
import itertools

import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.models.mnist_runner import make_runner
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.step_calls import call_lengths, multiples


# ---------------------------------------------------------------- call_lengths
def _simulate(step, n, train_steps, cuts):
    """One step at a time: a call ends when it holds n steps, at a cut, or at the end."""
    cuts = set(cuts)
    out, cur = [], 0
    while step < train_steps:
        step += 1
        cur += 1
        if cur == n or step in cuts or step == train_steps:
            out.append(cur)
            cur = 0
    return out


GRID = list(itertools.product((0, 3, 17), (1, 2, 4, 20), (0, 1, 5, 21, 40)))


@pytest.mark.parametrize("step,n,more", GRID)
def test_call_lengths_match_the_step_by_step_simulation(step, n, more):
    train_steps = step + more
    cut_sets = [(), (step + 1,), (train_steps,), (step + 1, train_steps), (step, step - 2, train_steps + 3),
                tuple(range(step + 3, train_steps + 1, 7)), (step + 2, step + 3, step + 4, step + n, step + n + 1),
                (step + 5, step + 5, step + 2 * n)]
    for cuts in cut_sets:
        got = call_lengths(step, n, train_steps, cuts)
        assert got == _simulate(step, n, train_steps, cuts), (step, n, train_steps, cuts)
        assert sum(got) == train_steps - step
        assert all(1 <= k <= n for k in got)
        ends = set(itertools.accumulate(got, initial=step))
        assert all(c in ends for c in cuts if step < c <= train_steps), (cuts, sorted(ends))


def test_call_lengths_edges():
    assert call_lengths(0, 4, 10) == [4, 4, 2]  # train_steps no multiple of n
    assert call_lengths(0, 1, 3, (2,)) == [1, 1, 1]
    assert call_lengths(5, 8, 5) == [] and call_lengths(7, 8, 5) == []
    assert call_lengths(0, 8, 12, (6,)) == [6, 6]  # the eval at 6 ends a call; the next one starts there
    with pytest.raises(ValueError):
        call_lengths(0, 0, 4)
    assert multiples(4, 0, 12) == [4, 8, 12] and multiples(4, 4, 11) == [8] and multiples(0, 0, 9) == []
    assert multiples(3, 10, 20, origin=10) == [13, 16, 19]


# ---------------------------------------------------------------- the CPU runner
def _cpu_runner(opt, B, seed=3):
    r = make_runner(B, opt, torch.device("cpu"), keep_prob=0.75, seed=seed)
    r.load_flat(M.flat_from_dict(M.init_params(1)), {}, 0)
    return r


def _feeder(B, rows=24, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(rows, 784, generator=g)
    y = torch.randint(0, 10, (rows,), generator=g)
    pos = [0]

    def next_batch():
        i = pos[0]
        pos[0] = (i + B) % rows
        return x[i:i + B], y[i:i + B]

    return next_batch


@pytest.mark.parametrize("opt,B", [
    (O.AdamOptimizer(0.01), 8),
    (O.AdamOptimizer(O.ExponentialDecay(0.01, 4, 0.5, False, 2), clip_norm=0.5, skip_nonfinite=True), 4),
    (O.MomentumOptimizer(0.01, 0.9, accum_steps=2), 4),
])
def test_cpu_runner_four_steps_per_call_equals_one(opt, B):
    rows = B * getattr(opt, "accum_steps", 1)
    one, four = _cpu_runner(opt, B), _cpu_runner(opt, B)
    one.set_step_log(16)
    four.set_step_log(16)
    fa, fb = _feeder(rows), _feeder(rows)
    losses = []
    for _ in range(8):
        one.train_step(*fa())
        losses.append(one.last_loss())
    four.train_steps(4, fb)
    first = four.read_step_log(1, 4)
    four.train_steps(4, fb)
    got = first + four.read_step_log(5, 8)
    want = one.read_step_log(1, 8)
    assert len(got) == len(want) == 8
    for a, b in zip(got, want):  # every field of every step (grad_norm is NaN without clip_norm)
        assert a.keys() == b.keys() == set(one.STEP_LOG_KEYS)
        assert all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (a, b)
    assert [r["step"] for r in got] == list(range(1, 9)) and all(r["rows"] == rows for r in got)
    if getattr(opt, "accum_steps", 1) == 1:
        assert [r["loss"] for r in got] == pytest.approx(losses, rel=1e-6)
    assert all(0 <= r["correct"] <= rows for r in got)
    assert [r["lr"] for r in got] == [O.lr_at(opt.learning_rate, t) for t in range(8)]
    assert torch.equal(one.params(), four.params())
    assert one.global_step() == four.global_step() == 8


def test_cpu_ring_and_refusals():
    r = _cpu_runner(O.AdamOptimizer(0.01), 4)
    with pytest.raises(ValueError, match="set_step_log"):
        r.read_step_log(1, 1)
    r.set_step_log(4)
    with pytest.raises(ValueError, match="not in the log"):
        r.read_step_log(1, 1)
    with pytest.raises(ValueError, match="next_batch"):
        r.train_steps(2)
    r.train_steps(10, _feeder(4))
    assert [x["step"] for x in r.read_step_log(7, 10)] == [7, 8, 9, 10]
    with pytest.raises(ValueError, match="capacity"):
        r.read_step_log(6, 10)
    with pytest.raises(ValueError, match="not in the log"):
        r.read_step_log(5, 6)


# ---------------------------------------------------------------- the driver flag
def _with_flags(argv, fn):
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog"] + argv)
        return fn(dist_main)
    finally:
        F.FLAGS.reset()


def test_supported_combinations_pass():
    _with_flags([], lambda d: d.check_steps_per_call_flags(2))  # off: no complaint, whatever the mode
    _with_flags(["--sync_replicas=False"], lambda d: d.check_steps_per_call_flags(2))
    _with_flags(["--steps_per_call=20", "--num_gpus=1"], lambda d: d.check_steps_per_call_flags(1))
    _with_flags(["--steps_per_call=20", "--num_gpus=2", "--dp_schedule=sfb+zero+mr"],
                lambda d: d.check_steps_per_call_flags(2))


@pytest.mark.parametrize("argv,word", [
    (["--steps_per_call=4", "--num_gpus=1", "--sync_replicas=False"], "steps_per_call=4 with --sync_replicas=False"),
    (["--steps_per_call=4", "--num_gpus=1", "--replicas_to_aggregate=1"], "steps_per_call=4 with backup workers"),
    (["--steps_per_call=4", "--num_gpus=1", "--model=resnet18"], "steps_per_call=4 with --model resnet18"),
    (["--steps_per_call=4", "--num_gpus=1", "--device_input=False"], "steps_per_call=4 with --device_input=False"),
    (["--steps_per_call=4", "--num_gpus=1", "--use_graph=False"], "steps_per_call=4 with --use_graph=False"),
    (["--steps_per_call=4"], "steps_per_call=4 with --num_gpus=0"),
    (["--steps_per_call=0"], "steps_per_call=0"),
    (["--steps_per_call=1001", "--num_gpus=1"], "steps_per_call=1001"),
])
def test_unsupported_combinations_are_flag_errors(argv, word):
    with pytest.raises(ValueError, match=word):
        _with_flags(argv, lambda d: d.check_steps_per_call_flags(2))


@pytest.mark.parametrize("extra,word", [
    (["--sync_replicas=False"], "sync_replicas"),   # a parameter-server mode
    (["--device_input=False"], "device_input"),     # host feed
    (["--model=resnet18"], "resnet18"),
])
def test_flag_errors_come_before_any_worker_starts(monkeypatch, extra, word):
    from tensorflow_distributed_amd.parallel import cluster
    from tensorflow_distributed_amd.training import dist_main
    from tensorflow_distributed_amd.utils import flags as F

    def no_server(*a, **k):
        raise AssertionError("a Server was built before the flag check")

    monkeypatch.setattr(cluster, "Server", no_server)
    dist_main.define_flags(0, "worker")
    F.FLAGS.reset()
    try:
        F.FLAGS.parse(["prog", "--steps_per_call=4", "--num_gpus=1", "--synthetic_data", "--data_dir=/nonexistent",
                       "--job_name=worker", "--task_index=0"] + extra)
        with pytest.raises(ValueError, match="steps_per_call=4.*" + word):
            dist_main.main()
    finally:
        F.FLAGS.reset()


def test_mnist_single_refuses_what_it_cannot_run(capsys):
    import mnist_single

    for argv in (["--steps_per_call", "4", "--cpu"], ["--steps_per_call", "0"]):
        with pytest.raises(SystemExit):
            mnist_single.main(argv)
        assert "--steps_per_call" in capsys.readouterr().err
