"""The device step log (csrc/step_log.h, kernels/step_log.hip, MnistEngine.set_step_log) and what is built
on it: NativeMnistRunner.train_steps / read_step_log and --steps_per_call of the two drivers.

The record of update t holds the loss and the correct count of that step's batch, its learning rate and,
with clipping or the guard, {norm, scale, ok}; it is written inside the step, eagerly and in one-step
and n-step graphs alike, and nothing on the device reads it back. Engines at batch 5 unless the batch is
what the case is about; "bit-identical" is torch.equal on integer views, so NaNs compare by their bits.
"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import schedule_args

import grad_accum_util as GA

pytestmark = pytest.mark.gpu

INF = float("inf")
B, SEED = 5, 1234
LR, B1, B2, EPS = 2.0 ** -7, 0.9, 0.999, 1e-8
LOSS, CORRECT, LRF, GNORM, CSCALE, OK, ROWS = range(7)  # the record's fields (csrc/step_log.h)
# tests/test_lr_schedule_gpu.py's bound for rates evaluated on the device: 4 x the worst relative error
# of the fp32 lr_at() measured there (1.130e-07)
LR_REL_BOUND = 4 * 1.130e-07


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _params0():
    return M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(13).items()})


def _engine(cuda, batch=B, dtype="bf16", log=16, keep=0.75):
    e = torch.classes.tfd.MnistEngine(batch, 0, keep, SEED, 0)
    e.set_dtype(dtype)
    e.set_adam(LR, B1, B2, EPS)
    e.params().copy_(_params0().to(cuda))
    e.sync_shadow()
    if log:
        e.set_step_log(log)
    return e


def _dataset(cuda, n, seed=21):
    gen = torch.Generator().manual_seed(seed)
    data = torch.rand(n, 784, generator=gen)
    labels = torch.randint(0, 10, (n,), generator=gen, dtype=torch.int32)
    perm = torch.randperm(n, generator=gen).to(torch.int32)
    return data, labels, perm


def _on_dataset(e, ds, cuda):
    e.set_dataset(*(t.to(cuda) for t in ds))
    e.set_input_mode(1)
    return e


def _log(e):
    """(t int64 [C], records float32 [C][8]) on the host"""
    torch.cuda.synchronize()
    t, rec = e.step_log()
    assert t.dtype == torch.int64 and rec.dtype == torch.float32 and rec.shape == (t.numel(), 8)
    return t.cpu().numpy(), rec.cpu().numpy()


def _rows(e):
    torch.cuda.synchronize()
    return e.loss_rows().cpu().numpy().copy(), e.correct_rows().cpu().numpy().copy()


def _ulp(x):
    return float(np.spacing(np.abs(np.float32(x))))


def _loss_ok(got, rows):
    """within ONE fp32 ulp of float32(fp64 sum / rows): the kernel sums in fp64, so the only rounding is the
    final conversion (and a different fp64 summation order can move that rounding by at most one place)"""
    want = np.float32(np.sum(rows.astype(np.float64)) / rows.size)
    return abs(float(got) - float(want)) <= _ulp(want)


def _check_record(t_arr, rec, t, cap, loss_rows, correct_rows):
    slot = (t - 1) % cap
    r = rec[slot]
    print("step %d slot %d: loss %.9g (fp64 mean %.9g) correct %g rows %g" % (
        t, slot, r[LOSS], np.sum(loss_rows.astype(np.float64)) / loss_rows.size, r[CORRECT], r[ROWS]))
    assert t_arr[slot] == t
    assert r[ROWS] == loss_rows.size
    assert r[CORRECT] == int(np.sum(correct_rows.astype(np.int64)))
    assert set(np.unique(correct_rows)) <= {0.0, 1.0}
    assert _loss_ok(r[LOSS], loss_rows), (t, r[LOSS])


# ================================================================ 1. record against read-back, eager
@pytest.mark.parametrize("dtype,batch", [("bf16", b) for b in (1, 2, 63, 65, 130, 257, 3840)]
                         + [("fp32", b) for b in (1, 65, 257, 3840)])
def test_record_is_the_fp64_mean_of_the_rows_read_back(cuda, dtype, batch):
    """63 / 65 straddle a wave, 257 is one row past the block, 3840 is the largest batch"""
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(batch, 784, generator=gen)
    y = torch.randint(0, 10, (batch,), generator=gen, dtype=torch.int32)
    seen = []
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, batch, dtype)
        assert e.step_log_capacity() == 16
        e.feed_x().copy_(x.to(cuda))
        e.feed_y().copy_(y.to(cuda))
        for _ in range(3):
            e.train_step()
            seen.append(_rows(e))
    t_arr, rec = _log(e)
    for t, (lr_, cr_) in enumerate(seen, 1):
        _check_record(t_arr, rec, t, 16, lr_, cr_)
        r = rec[t - 1]
        assert r[LRF] == np.float32(LR) and math.isnan(r[GNORM]) and r[CSCALE] == 1.0 and r[OK] == 1.0
    assert (t_arr[3:] == 0).all()  # no other slot was touched
    if batch == 3840:
        # the check is tighter than one row in 3840: 5 % on the largest row of the host copy is rejected
        rows = seen[-1][0].copy()
        i = int(np.argmax(rows))
        assert rows[i] > 0
        rows[i] *= 1.05
        assert not _loss_ok(rec[2][LOSS], rows)


# ================================================================ 2. eager = one-step graph = n-step graph
def test_eager_one_step_graph_and_n_step_graph_write_the_same_log(cuda):
    ds = _dataset(cuda, 4 * B)
    seen = []
    with torch.cuda.stream(torch.cuda.Stream()):
        eager, one, five = (_on_dataset(_engine(cuda), ds, cuda) for _ in range(3))
        for _ in range(10):
            eager.train_step()
            seen.append(_rows(eager))
        one.capture_train_step("g")
        one.replay("g", 10)
        five.capture_train_steps("g", 5)
        five.replay("g", 2)
    logs = [_log(e) for e in (eager, one, five)]
    for t_arr, rec in logs[1:]:
        assert np.array_equal(t_arr, logs[0][0])
        assert np.array_equal(rec.view(np.int32), logs[0][1].view(np.int32))
    for e in (one, five):
        assert torch.equal(_bits(e.params()), _bits(eager.params())) and int(e.step_tensor().item()) == 10
    # every step of the graphs -- the middle ones no host read could see -- against the eager read-backs
    t_arr, rec = logs[2]
    assert list(t_arr[:10]) == list(range(1, 11)) and (t_arr[10:] == 0).all()
    for t, (lr_, cr_) in enumerate(seen, 1):
        _check_record(t_arr, rec, t, 16, lr_, cr_)
        assert math.isnan(rec[t - 1][GNORM]) and rec[t - 1][CSCALE] == 1.0 and rec[t - 1][OK] == 1.0
    assert len({float(r[LOSS]) for r in rec[:10]}) > 1  # the steps differ: a stale record would show


# ================================================================ 3. observation only
# capture_topology(1) of the default one-GPU step (bf16, fused Adam tail, device input, B = 5) as the parent
# commit of the step log lists it (recorded from a run of that commit): six kernel nodes in one chain
TOPOLOGY_AT_PARENT = ['node 0 0', 'node 1 0', 'node 2 0', 'node 3 0', 'node 4 0', 'node 5 0', 'edge 0 1', 'edge 1 2',
                      'edge 2 3', 'edge 3 4', 'edge 4 5', 'tag conv_fwd@0 0', 'tag fc_fwd@0 1 2', 'tag fc_bwd@0 3',
                      'tag conv_bwd@0 4', 'tag opt@0 5']


def _state(e):
    return {"params": e.params(), "params_bf16": e.params_bf16(), "adam_m": e.adam_m(), "adam_v": e.adam_v(),
            "step": e.step_tensor()}


def _configure(e, cfg, cuda):
    """-> the transport to close, or None"""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    if cfg == "unfused":
        e.set_fused_tail(0)
    elif cfg == "momentum":
        e.set_momentum(LR, 0.9, False)
    elif cfg == "rmsprop":
        e.set_rmsprop(LR, 0.9, 0.0, 1e-10, False)
    elif cfg == "lamb":
        e.set_lamb(LR, B1, B2, 1e-6, 0.01, True)
    elif cfg == "dp_allreduce":
        return attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True)
    elif cfg == "dp_sfb":
        return attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, sfb=True)
    elif cfg == "dp_zero":
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True)
        e.set_zero(True)
        return tr
    return None


@pytest.mark.parametrize("cfg", ["fused", "unfused", "fp32", "dp_allreduce", "dp_sfb", "dp_zero", "momentum", "rmsprop",
                                 "lamb"])
def test_the_log_only_observes(cuda, cfg):
    """6 steps -- two eager, then two replays of a 2-step graph -- with the log on and off: the same bits.
    The forced-DP schedules run at the small batches tests/test_dp_transport_gpu.py runs them at."""
    batch = {"dp_sfb": 37, "dp_allreduce": 32, "dp_zero": 32}.get(cfg, B)
    ds = _dataset(cuda, 4 * batch)
    engines, trs = [], []
    with torch.cuda.stream(torch.cuda.Stream()):
        for log in (0, 16):
            e = _on_dataset(_engine(cuda, batch, "fp32" if cfg == "fp32" else "bf16", log=log), ds, cuda)
            trs.append(_configure(e, cfg, cuda))
            e.train_step()
            e.train_step()
            e.capture_train_steps("g", 2)
            e.replay("g", 2)
            engines.append(e)
    torch.cuda.synchronize()
    off, on = engines
    if cfg == "dp_zero":
        with torch.cuda.stream(torch.cuda.Stream()):
            off.sync_params()
            on.sync_params()
        torch.cuda.synchronize()
    a, b = _state(off), _state(on)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (cfg, k)
    assert int(on.step_tensor().item()) == 6 and off.step_log_capacity() == 0
    t_arr, rec = _log(on)
    assert list(t_arr[:6]) == [1, 2, 3, 4, 5, 6] and (t_arr[6:] == 0).all()
    assert (rec[:6, ROWS] == batch).all() and np.isfinite(rec[:6, LOSS]).all() and (rec[:6, LOSS] > 0).all()
    assert (rec[:6, LRF] == np.float32(LR)).all() and (rec[:6, OK] == 1.0).all()
    with pytest.raises(RuntimeError, match="set_step_log"):
        off.step_log()
    for tr in trs:
        if tr is not None:
            tr.check()
            tr.close()


def test_log_off_is_the_parent_commits_graph_and_on_keeps_the_fused_tail(cuda):
    ds = _dataset(cuda, 4 * B)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _on_dataset(_engine(cuda, log=0), ds, cuda)
        e.train_step()
        off = list(e.capture_topology(1))
        e.set_step_log(16)
        on = list(e.capture_topology(1))
        e.set_step_log(0)
        off_again = list(e.capture_topology(1))
    torch.cuda.synchronize()
    print("\n".join(off))
    assert off == TOPOLOGY_AT_PARENT
    assert off_again == TOPOLOGY_AT_PARENT
    # on: one more kernel node, tagged; Adam still ends the step in ONE launch that also reduces the slabs
    tags = {ln.split()[1]: ln.split()[2:] for ln in on if ln.startswith("tag ")}
    assert len([ln for ln in on if ln.startswith("node ")]) == len([ln for ln in off if ln.startswith("node ")]) + 1
    assert len(tags["step_log@0"]) == 1 and "opt@0" in tags and "slab_reduce@0" not in tags
    assert set(tags) == {ln.split()[1] for ln in off if ln.startswith("tag ")} | {"step_log@0"}


# ================================================================ 4. ring
def _runner(cuda, opt=None, batch=B, dtype="bf16", n_rows=4 * B, log=None, seed=3):
    from tensorflow_distributed_amd.models.mnist_runner import NativeMnistRunner

    r = NativeMnistRunner(batch, opt or O.AdamOptimizer(LR), keep_prob=0.75, seed=seed, device=cuda, dtype=dtype)
    r.load_flat(_params0(), {}, 0)
    data, labels, _ = _dataset(cuda, n_rows)
    r.set_device_dataset(data, labels, seed=17)
    if log is not None:
        r.set_step_log(log)
    return r


def test_ring_of_four(cuda):
    fresh = _runner(cuda)
    with pytest.raises(ValueError, match="set_step_log"):
        fresh.read_step_log(1, 1)
    fresh.set_step_log()
    assert fresh.eng.step_log_capacity() == 1024
    with pytest.raises(ValueError, match="not in the log"):  # never written
        fresh.read_step_log(1, 1)
    r = _runner(cuda, log=4)
    r.train_steps(10)
    recs = r.read_step_log(7, 10)
    assert [x["step"] for x in recs] == [7, 8, 9, 10]
    assert all(set(x) == set(r.STEP_LOG_KEYS) and x["rows"] == B and x["ok"] is True for x in recs)
    with pytest.raises(ValueError, match="capacity"):
        r.read_step_log(6, 10)
    with pytest.raises(ValueError, match="not in the log"):  # overwritten by steps 9 and 10
        r.read_step_log(5, 6)
    with pytest.raises(ValueError, match="not in the log"):  # not taken yet
        r.read_step_log(10, 11)
    with pytest.raises(ValueError):
        r.read_step_log(0, 2)


# ================================================================ 5. schedule, clip, guard
def test_record_lr_follows_the_schedule(cuda):
    sched = O.ExponentialDecay(0.1, 4, 0.5, warmup_steps=3)
    ds = _dataset(cuda, 4 * B)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _on_dataset(_engine(cuda), ds, cuda)
        e.set_lr_schedule(*schedule_args(sched))
        e.train_step()
        e.capture_train_steps("g", 5)
        e.replay("g", 1)
    t_arr, rec = _log(e)
    assert list(t_arr[:6]) == [1, 2, 3, 4, 5, 6]
    want = [e.lr_at_step(t - 1) for t in range(1, 7)]
    assert len(set(want)) == 6  # warm-up, then decay: every step has its own rate
    for t in range(1, 7):
        got, ref = float(rec[t - 1][LRF]), want[t - 1]
        print("lr of record %d: %.9g, lr_at_step(%d) = %.9g" % (t, got, t - 1, ref))
        assert abs(got - ref) / abs(ref) <= LR_REL_BOUND, (t, got, ref)
        assert abs(got - O.lr_at(sched, t - 1)) / O.lr_at(sched, t - 1) <= LR_REL_BOUND


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_record_carries_the_bits_of_the_clip_and_the_guard(cuda, dtype):
    ds = _dataset(cuda, 4 * B)
    seen = []
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _on_dataset(_engine(cuda, dtype=dtype), ds, cuda)
        e.set_clip_norm(0.01)
        e.set_skip_nonfinite(True)
        for _ in range(4):
            e.train_step()
            torch.cuda.synchronize()
            seen.append((e.grad_norm().cpu().numpy().copy(), e.last_step_ok(), _rows(e)))
    t_arr, rec = _log(e)
    for t, (pair, ok, (lr_, cr_)) in enumerate(seen, 1):
        r = rec[t - 1]
        assert np.array_equal(r[GNORM:CSCALE + 1].view(np.int32), pair.view(np.int32)), (t, r, pair)
        assert (r[OK] != 0) == ok and r[OK] in (0.0, 1.0)
        _check_record(t_arr, rec, t, 16, lr_, cr_)
    assert any(r[CSCALE] < 1.0 for r in rec[:4])  # the clip was active: the fields are not the defaults


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_the_log_places_the_skipped_step_of_an_epoch_graph(cuda, dtype):
    """tests/test_nonfinite_guard_gpu.py's epoch graph -- 4 * B images, one poisoned, one graph of 4 steps --
    could count the skip; the log says which step it was: the one whose batch holds the image."""
    gen = torch.Generator().manual_seed(21)
    data = torch.rand(4 * B, 784, generator=gen)
    data = _poison(data, 13)
    labels = torch.randint(0, 10, (4 * B,), generator=gen, dtype=torch.int32)
    perm = torch.randperm(4 * B, generator=gen).to(torch.int32)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _on_dataset(_engine(cuda, dtype=dtype), (data, labels, perm), cuda)
        e.set_skip_nonfinite(True)
        e.capture_train_steps("epoch", 4)
        e.replay("epoch", 1)
    t_arr, rec = _log(e)
    assert list(t_arr[:4]) == [1, 2, 3, 4] and (t_arr[4:] == 0).all()
    # step s (0-based) trains on perm[s * B .. (s + 1) * B)
    where = int((perm == 13).nonzero()[0, 0]) // B
    oks = [float(r[OK]) for r in rec[:4]]
    assert oks == [0.0 if s == where else 1.0 for s in range(4)], (oks, where)
    assert e.skipped_steps() == 1
    bad = rec[where]
    assert not np.isfinite(bad[GNORM]) and bad[CSCALE] == 0.0
    assert all(np.isfinite(r[GNORM]) and r[CSCALE] == 1.0 for s, r in enumerate(rec[:4]) if s != where)


def _poison(x, row):
    x = x.clone()
    x[row, 14 * 28 + 14] = INF  # one pixel of one image
    return x


# ================================================================ 6. accumulation
def _micro_rows(cuda, dtype, k, params, x, y):
    """Per-row losses / correct flags of k micro-batches of B rows, the way grad_accum_util.micro_grads
    drives a plain engine micro-batch by micro-batch (forward, backward_a, backward_b: the step bump)."""
    out = []
    with torch.cuda.stream(torch.cuda.Stream()):
        e = GA._engine(cuda, dtype, B, params)
        for j in range(k):
            e.feed_x().copy_(x[j * B:(j + 1) * B].to(cuda))
            e.feed_y().copy_(y[j * B:(j + 1) * B].to(cuda))
            e.forward(True)
            e.backward_a()
            e.backward_b()
            out.append(_rows(e))
    return np.concatenate([a for a, _ in out]), np.concatenate([c for _, c in out])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_accumulated_step_logs_the_mean_over_its_micro_batches(cuda, dtype):
    k = 3
    params, x, y = GA.O.random_case(k * B, seed=4)
    loss_rows, correct_rows = _micro_rows(cuda, dtype, k, params, x, y)
    assert loss_rows.size == 15
    with torch.cuda.stream(torch.cuda.Stream()):
        e = GA._engine(cuda, dtype, B, params)  # a zero rate: every step sees the same parameters
        e.set_grad_accum(k)
        e.set_step_log(8)
        e.feed_x().copy_(x.to(cuda))
        e.feed_y().copy_(y.to(cuda))
        e.train_step()
        e.capture_train_steps("g", 2)
        e.replay("g", 1)
    t_arr, rec = _log(e)
    assert list(t_arr[:3]) == [1, 2, 3] and (t_arr[3:] == 0).all()
    assert int(e.step_tensor().item()) == 3 and int(e.micro_step_tensor().item()) == 9
    for t in (1, 2, 3):  # eager, then the two steps of the graph
        _check_record(t_arr, rec, t, 8, loss_rows, correct_rows)
        assert rec[t - 1][ROWS] == 15
    rows = loss_rows.copy()
    rows[int(np.argmax(rows))] *= 1.05  # one row of the fifteen off by 5 %: rejected
    assert not _loss_ok(rec[0][LOSS], rows)


# ================================================================ 7. runner and drivers
def _same_log(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), (k, x, y)


@pytest.mark.parametrize("n_rows,n,calls", [(3 * B, 7, 1), (8 * B, 4, 3)])
def test_train_steps_is_n_train_step_calls(cuda, n_rows, n, calls):
    """3 * B rows: an epoch boundary -- a reshuffle -- every third step, inside the call. 8 * B rows, three
    calls of 4: the second and third replay the 4-step graph, the reshuffle falls between calls."""
    one, many = (_runner(cuda, n_rows=n_rows, log=32) for _ in range(2))
    for _ in range(n * calls):
        one.train_step(None, None)
    for _ in range(calls):
        many.train_steps(n)
    assert (n in many._multi_ready) == (n_rows == 8 * B)
    assert one.global_step() == many.global_step() == n * calls
    torch.cuda.synchronize()
    assert torch.equal(one._dev_perm, many._dev_perm)
    for k, v in _state(one.eng).items():
        assert torch.equal(_bits(v), _bits(_state(many.eng)[k])), k
    log = many.read_step_log(1, n * calls)
    _same_log(log, one.read_step_log(1, n * calls))
    assert [x["step"] for x in log] == list(range(1, n * calls + 1))
    host = _runner(cuda)
    host._dev_data = None
    with pytest.raises(ValueError, match="device"):
        host.train_steps(2)


def test_mnist_single_prints_the_same_lines(cuda, tmp_path, capsys):
    import mnist_single

    outs = []
    for n in (1, 8):
        rc = mnist_single.main(["--batch_size=16", "--training_iters=336", "--display_step=4", "--eval_batches=3",
                                f"--data_dir={tmp_path}/none", f"--steps_per_call={n}"])
        assert rc == 0
        outs.append(capsys.readouterr().out)
    keep = [[ln for ln in o.splitlines() if ln.startswith("Iter ") or ln.startswith("Mean Accuracy")] for o in outs]
    assert len(keep[0]) == 6 and keep[0][0].startswith("Iter 64, Minibatch Loss= ") and keep[0][4].startswith("Iter 320,")
    assert keep[0] == keep[1], keep
    assert "Last call of 4 step(s): training loss" in outs[1] and "Last call" not in outs[0]


def test_dist_main_four_steps_per_call_logs_what_one_logs(cuda, tmp_path):
    """--batch_size=2 and a rate that fp32 holds exactly, so that what the N = 1 loop logs -- the fp32 mean
    of two rows and the host's lr -- and what the step log holds are the same numbers, not neighbours."""
    from tensorflow_distributed_amd import launch

    runs = {}
    for n in (1, 4):
        mf = os.path.join(tmp_path, "m%d.jsonl" % n)
        args = ["--num_gpus=1", "--train_steps=8", f"--logdir={tmp_path}/log{n}", "--synthetic_data", "--eval_batches=1",
                "--data_dir=/nonexistent", f"--metrics_file={mf}", "--batch_size=2", "--learning_rate=0.0078125",
                "--clip_norm=0.5", "--skip_nonfinite", "--eval_at_steps=6", f"--steps_per_call={n}"]
        r = launch.launch(1, 1, args, echo=False, timeout_s=300)
        assert r["ok"], r["outputs"]
        out = "".join(v for k, v in r["outputs"].items() if k.startswith("worker:0#"))
        done = [(int(a), int(b)) for a, b in re.findall(r"training step (\d+) done \(global step: (\d+)\)", out)]
        assert done == [(i, i) for i in range(1, 9)], out[-3000:]
        runs[n] = [json.loads(line) for line in open(mf) if line.strip()]
    steps = {n: [x for x in recs if "step_ms" in x] for n, recs in runs.items()}
    assert [x["global_step"] for x in steps[4]] == list(range(1, 9)) == [x["global_step"] for x in steps[1]]
    for a, b in zip(steps[1], steps[4]):
        for k in ("loss", "lr", "grad_norm", "clip_scale", "step_ok", "skipped_steps", "step", "accum_steps"):
            assert a[k] == b[k], (k, a, b)
        assert 0.0 <= b["train_accuracy"] <= 1.0 and "steps_in_call" not in a
    assert [x["steps_in_call"] for x in steps[4]] == [4, 4, 4, 4, 2, 2, 2, 2]  # the eval at 6 ends a call
    assert ["step_ms_gpu" in x for x in steps[4]] == [False, False, False, True, False, True, False, True]
    for n in (1, 4):  # the performance row sits behind step 6 and before step 7
        kinds = [x.get("event", x.get("global_step")) for x in runs[n]]
        i = kinds.index("performance")
        assert kinds[i - 1] == 6 and kinds[i + 1] == 7 and runs[n][i]["steps"] == 6, kinds
