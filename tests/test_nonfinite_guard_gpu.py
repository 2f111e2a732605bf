"""The non-finite guard on the device (csrc/kernels/grad_guard.hip, optim_guard.hip, the guarded stages of
optim_layerwise.hip, MnistEngine.set_skip_nonfinite): a step whose aggregated gradient is not finite
stores nothing -- parameters, slots, the bf16 shadow and the moving average keep their bits -- and a
device counter goes up by one; a finite step is the clip instantiation's, bit for bit.

Flat ops on a few thousand elements; engines at batch 5. "Bit-identical" is torch.equal on integer views,
so NaNs compare by their bits. The poison is always a floating-point value in input data.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M

import mnist_oracle as MO
from dist_util import run_ranks

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
LR, B1, B2, EPS, MOM, WD, EETA = 2.0 ** -7, 0.9, 0.999, 1e-8, 0.9, 0.01, 1e-3
DECAY = 0.9
SCHED = ("constant", [], [], [])


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


# ================================================================ flat ops
SIZES = [3, 4099, 16385]  # scalar tail only; two stage-1 blocks with n % 4 == 3; n % 4 == 1


def _positions(n):
    """element 0; the last lane of the last float4; the scalar tail; an element of stage 1's second block
    (its first batch of vectors is 256..511) -- those that exist at this n"""
    pos = {0}
    if n >= 4:
        pos.add(4 * (n // 4) - 1)
    if n % 4:
        pos.add(n - 1)
    if n > 4 * 256 + 5:
        pos.add(4 * 256 + 5)
    return sorted(pos)


def _segs(n):
    rows = [(0, n, 3)] if n < 4096 else [(0, 2048, 3), (2048, n - 2048, 0)]
    return torch.tensor(rows, dtype=torch.int64)


def _grad(cuda, n, dt, seed=1):
    g = torch.randn(n, device=cuda, generator=torch.Generator(device=cuda).manual_seed(seed)) * 1e-2
    return g.to(dt)


def _buffers(cuda, n, seed=2):
    gen = torch.Generator(device=cuda).manual_seed(seed)
    p = torch.randn(n, device=cuda, generator=gen)
    return {"p": p, "m": torch.randn(n, device=cuda, generator=gen) * 1e-2,
            "v": torch.rand(n, device=cuda, generator=gen) * 1e-4, "pbf": p.to(torch.bfloat16), "ema": p * 0.5}


def _run_op(op, b, g, step, **kw):
    """One of the five flat ops on the buffers b (in place), Adam's t = *step + 1"""
    ops = torch.ops.tfd
    n = g.numel()
    if op == "adam":
        ops.adam_flat(b["p"], b["m"], b["v"], g, b["pbf"], LR, B1, B2, EPS, step, 0.5, 1, *SCHED, ema=b["ema"],
                      ema_decay=DECAY, **kw)
    elif op == "momentum":
        ops.momentum_flat(b["p"], b["m"], g, b["pbf"], LR, MOM, 0.0, False, 0.5, step, 1, *SCHED, **kw)
    elif op == "momentum_ema":
        ops.momentum_ema_flat(b["p"], b["m"], g, b["pbf"], LR, MOM, 0.0, True, 0.5, step, 1, *SCHED, kw.pop("gscale", None),
                              ema=b["ema"], ema_decay=DECAY, **kw)
    elif op == "lamb":
        ops.lamb_flat(b["p"], b["m"], b["v"], g, b["pbf"], _segs(n), LR, B1, B2, 1e-6, WD, step, 1, 0.5, *SCHED,
                      ema=b["ema"], ema_decay=DECAY, **kw)
    else:
        ops.lars_flat(b["p"], b["m"], g, b["pbf"], _segs(n), LR, MOM, WD, EETA, 0.0, step, 1, 0.5, *SCHED, ema=b["ema"],
                      ema_decay=DECAY, **kw)


OPS = ["adam", "momentum", "momentum_ema", "lamb", "lars"]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_poisoned_gradient_gives_ok_0_and_every_flat_op_stores_nothing(cuda, n, dt):
    ops = torch.ops.tfd
    skipped = torch.zeros(1, dtype=torch.int64, device=cuda)
    step = torch.full((1,), 3, dtype=torch.int64, device=cuda)
    clean = _grad(cuda, n, dt)
    count = 0
    for pos in _positions(n):
        for bad in (NAN, INF, -INF):
            g = clean.clone()
            g[pos] = bad
            out = ops.grad_guard(g, 0.5, 1.0, skipped)
            count += 1
            norm, scale, ok = out.tolist()
            assert out.dtype == torch.float32 and out.shape == (3,)
            assert ok == 0.0 and scale == 0.0 and not np.isfinite(norm), (n, pos, bad, norm, scale, ok)
            assert int(skipped.item()) == count, (n, pos, bad)
            for op in OPS:
                b = _buffers(cuda, n)
                before = {k: v.clone() for k, v in b.items()}
                _run_op(op, b, g, step, gscale=out[1:2], guard=out)
                _same_bits(b, before, (op, n, pos, bad))
                _run_op(op, b, g, step, guard=out[2:3])  # the ok element alone, no clip factor
                _same_bits(b, before, (op, n, pos, bad, "ok view"))
    assert int(skipped.item()) == count == 3 * len(_positions(n))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_finite_gradient_gives_ok_1_and_the_clip_instantiations_update(cuda, n, dt):
    """{norm, scale} are grad_global_norm's bits; every op with guard= equals the same op with gscale= alone."""
    ops = torch.ops.tfd
    skipped = torch.zeros(1, dtype=torch.int64, device=cuda)
    step = torch.full((1,), 3, dtype=torch.int64, device=cuda)
    g = _grad(cuda, n, dt)
    raw = float(g.double().norm().item())
    for clip in (0.25 * raw, 1e30):  # 0.5 * raw is the scaled norm: an active clip, and an inactive one
        out = ops.grad_guard(g, 0.5, clip, skipped)
        ref = ops.grad_global_norm(g, clip, 0.5)
        assert torch.equal(_bits(out[:2]), _bits(ref)), (out.tolist(), ref.tolist())
        assert out[2].item() == 1.0 and int(skipped.item()) == 0
        assert (out[1].item() < 1.0) == (clip < 1e30)
        for op in OPS:
            a, b = _buffers(cuda, n), _buffers(cuda, n)
            start = {k: v.clone() for k, v in a.items()}
            _run_op(op, a, g, step, gscale=out[1:2], guard=out)
            _run_op(op, b, g, step, gscale=ref[1:2])
            _same_bits(a, b, (op, n, clip))
            assert not torch.equal(a["p"], start["p"]), op
    one = ops.grad_guard(g, 0.5, INF, skipped)  # no clipping: scale is exactly 1, not inf / inf
    assert one.tolist() == [ref[0].item(), 1.0, 1.0]


def test_guard_skips_a_norm_that_overflows_fp32(cuda):
    ops = torch.ops.tfd
    skipped = torch.zeros(1, dtype=torch.int64, device=cuda)
    g = torch.full((67,), 1e-3, device=cuda)
    g[40] = 1e20  # finite, its square is not: skipped as well
    norm, scale, ok = ops.grad_guard(g, 1.0, INF, skipped).tolist()
    assert norm == INF and scale == 0.0 and ok == 0.0 and int(skipped.item()) == 1
    g[40] = 1e18
    norm, scale, ok = ops.grad_guard(g, 1.0, INF, skipped).tolist()
    assert abs(norm - 1e18) <= 1e18 * 2.0 ** -22 and scale == 1.0 and ok == 1.0 and int(skipped.item()) == 1
    norm, scale, ok = ops.grad_guard(g, 1e30, INF, skipped).tolist()  # the scaled norm overflows the fp32 result
    assert norm == INF and scale == 0.0 and ok == 0.0 and int(skipped.item()) == 2
    with pytest.raises(RuntimeError):
        ops.grad_guard(g, 1.0, INF, torch.zeros(1, dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError):
        ops.grad_guard(g, 1.0, 0.0, skipped)
    with pytest.raises(RuntimeError):  # a guard is [3] or one element
        b = _buffers(cuda, 67)
        ops.momentum_flat(b["p"], b["m"], g, None, LR, MOM, 0.0, False, 1.0, None, 1, *SCHED, None, torch.zeros(2, device=cuda))


def test_captured_guard_counts_on_every_replay(cuda):
    """grad_guard + adam_flat captured once, replayed on a finite, a poisoned and a finite gradient: the
    counter reads 1 and p is two finite eager updates, at t and t + 2."""
    ops = torch.ops.tfd
    n = 4099
    fin = [_grad(cuda, n, torch.float32, seed=s) for s in (5, 6)]
    bad = _grad(cuda, n, torch.float32, seed=7)
    bad[n - 1] = NAN
    g = fin[0].clone()
    skipped = torch.zeros(1, dtype=torch.int64, device=cuda)
    step = torch.full((1,), 3, dtype=torch.int64, device=cuda)
    b = _buffers(cuda, n)
    start = {k: v.clone() for k, v in b.items()}
    out = torch.zeros(3, device=cuda)

    def body():
        out.copy_(ops.grad_guard(g, 0.5, 1e30, skipped))
        ops.adam_flat(b["p"], b["m"], b["v"], g, b["pbf"], LR, B1, B2, EPS, step, 0.5, 1, *SCHED, gscale=out[1:2],
                      ema=b["ema"], ema_decay=DECAY, guard=out)
        step.add_(1)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()  # warm-up: allocations
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in b:
        b[k].copy_(start[k])
    step.fill_(3)
    skipped.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    oks = []
    for src in (fin[0], bad, fin[1]):
        g.copy_(src)
        graph.replay()
        oks.append(out[2].item())
    torch.cuda.synchronize()
    assert oks == [1.0, 0.0, 1.0] and int(skipped.item()) == 1 and int(step.item()) == 6
    e = {k: v.clone() for k, v in start.items()}
    one = torch.ones(1, device=cuda)
    for t0, src in ((3, fin[0]), (5, fin[1])):
        ops.adam_flat(e["p"], e["m"], e["v"], src, e["pbf"], LR, B1, B2, EPS, torch.full((1,), t0, dtype=torch.int64, device=cuda),
                      0.5, 1, *SCHED, gscale=one, ema=e["ema"], ema_decay=DECAY)
    torch.cuda.synchronize()
    _same_bits(b, e, "graph vs eager")


# ================================================================ engine
B = 5
SEED = 1234


def _batches(k, rows=B, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(rows, 784, generator=g), torch.randint(0, 10, (rows,), generator=g, dtype=torch.int32))
            for _ in range(k)]


def _poison(x, row):
    x = x.clone()
    x[row, 14 * 28 + 14] = INF  # one pixel of one image
    return x


def _params0():
    return {k: v * 0.05 for k, v in M.init_params(13).items()}


def _engine(cuda, dtype, cfg, guard):
    """cfg: plain / ema / lamb / lars / clip / accum / momentum. The twin (guard False) is the same engine
    with the guard off and, where cfg sets no clip, set_clip_norm(1e30): the same path with scale exactly 1."""
    e = torch.classes.tfd.MnistEngine(B, 0, 0.75, SEED, 0)
    e.set_dtype(dtype)
    if cfg == "lamb":
        e.set_lamb(LR, B1, B2, 1e-6, WD, True)
    elif cfg == "lars":
        e.set_lars(LR, MOM, WD, EETA, 0.0, True)
    elif cfg == "momentum":
        e.set_momentum(LR, MOM, False)
    else:
        e.set_adam(LR, B1, B2, EPS)
    if cfg == "clip":
        e.set_clip_norm(1.0)
    elif not guard:
        e.set_clip_norm(1e30)
    e.set_skip_nonfinite(guard)
    assert e.skip_nonfinite() == guard
    e.params().copy_(M.flat_from_dict(_params0()).to(cuda))
    e.sync_shadow()
    if cfg == "ema":
        e.set_ema(DECAY, True)
    if cfg == "accum":
        e.set_grad_accum(2)
    return e


def _rows(cfg):
    return 2 * B if cfg == "accum" else B


def _feed(e, xy, cuda):
    e.feed_x().copy_(xy[0].to(cuda))
    e.feed_y().copy_(xy[1].to(cuda))


def _state(e, cfg):
    s = {"params": e.params().clone(), "m": e.adam_m().clone(), "v": e.adam_v().clone(), "pbf": e.params_bf16().clone(),
         "step": e.step_tensor().clone()}
    if cfg == "ema":
        s["ema"] = e.ema_params().clone()
    return s


_ORACLE = {}


def _oracle_dw1_is_non_finite(dtype):
    """On the CPU, in fp64 with the kernels' rounding points: this poisoned batch gives a non-finite conv1
    weight gradient, so a device norm that stays finite has lost the poison in a step kernel."""
    if dtype not in _ORACLE:
        x, y = _batches(2)[1]
        res = MO.oracle_step(_params0(), _poison(x, 2), y, dtype)
        _ORACLE[dtype] = not bool(torch.isfinite(res["grads"]["wc1"]).all())
    return _ORACLE[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_finite_steps_equal_the_inactive_clip_twin(cuda, dtype):
    with torch.cuda.stream(torch.cuda.Stream()):
        e, twin = _engine(cuda, dtype, "ema", True), _engine(cuda, dtype, "ema", False)
        for xy in _batches(3):
            for eng in (e, twin):
                _feed(eng, xy, cuda)
                eng.train_step()
    torch.cuda.synchronize()
    _same_bits(_state(e, "ema"), _state(twin, "ema"))
    assert int(e.step_tensor().item()) == 3 and e.skipped_steps() == 0 and e.last_step_ok()
    assert not torch.equal(e.params(), M.flat_from_dict(_params0()).to(cuda))
    pair = e.grad_norm()
    assert pair.shape == (2,) and np.isfinite(pair[0].item()) and pair[1].item() == 1.0  # reported without clipping
    assert torch.equal(_bits(pair), _bits(twin.grad_norm()))
    assert twin.skipped_steps() == 0 and int(e.skipped_steps_tensor().item()) == 0


@pytest.mark.parametrize("cfg", ["plain", "ema", "lamb", "lars", "clip", "accum", "momentum"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_poisoned_step_is_an_identity_update_that_consumes_its_step(cuda, dtype, cfg):
    assert _oracle_dw1_is_non_finite(dtype)
    rows = _rows(cfg)
    b0, b1, b2 = _batches(3, rows)
    # accum: the poison sits in the second micro-batch only
    b1 = (_poison(b1[0], rows - B + 2), b1[1])
    with torch.cuda.stream(torch.cuda.Stream()):
        e, twin = _engine(cuda, dtype, cfg, True), _engine(cuda, dtype, cfg, False)
        for eng in (e, twin):
            _feed(eng, b0, cuda)
            eng.train_step()
        torch.cuda.synchronize()
        before = _state(e, cfg)
        _same_bits(before, _state(twin, cfg), "finite step 0")
        _feed(e, b1, cuda)
        e.train_step()
        torch.cuda.synchronize()
        norm = e.grad_norm()[0].item()
        print(f"guard {dtype} {cfg}: poisoned step norm {norm!r}")
        assert not np.isfinite(norm), "a step kernel lost the poison: the aggregated gradient's norm is finite"
        after = _state(e, cfg)
        assert int(after.pop("step").item()) == int(before.pop("step").item()) + 1 == 2
        _same_bits(after, before, "poisoned step")
        assert e.skipped_steps() == 1 and not e.last_step_ok() and e.grad_norm()[1].item() == 0.0
        # the next finite step: the twin's from the same state and global_step
        twin.step_tensor().copy_(e.step_tensor())
        twin.sync_micro_step()
        for eng in (e, twin):
            _feed(eng, b2, cuda)
            eng.train_step()
    torch.cuda.synchronize()
    _same_bits(_state(e, cfg), _state(twin, cfg), "finite step after the skip")
    assert e.skipped_steps() == 1 and e.last_step_ok() and int(e.step_tensor().item()) == 3
    assert not torch.equal(e.params(), before["params"])
    assert torch.isfinite(e.params()).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_one_poisoned_image_in_an_epoch_graph_skips_one_step(cuda, dtype):
    """Device input: 4 * B images, one poisoned, one graph of 4 steps = the epoch. Whatever the shuffle,
    exactly one step holds the image."""
    gen = torch.Generator().manual_seed(21)
    data = torch.rand(4 * B, 784, generator=gen)
    data[13, 300] = INF
    labels = torch.randint(0, 10, (4 * B,), generator=gen, dtype=torch.int32)
    perm = torch.randperm(4 * B, generator=gen).to(torch.int32)
    ds = tuple(t.to(cuda) for t in (data, labels, perm))
    with torch.cuda.stream(torch.cuda.Stream()):
        engines = []
        for _ in range(2):
            e = _engine(cuda, dtype, "plain", True)
            e.set_dataset(*ds)
            e.set_input_mode(1)
            engines.append(e)
        eager, graph = engines
        oks = []
        for _ in range(4):
            eager.train_step()
            oks.append(eager.last_step_ok())
        graph.capture_train_steps("epoch", 4)
        graph.replay("epoch", 1)
    torch.cuda.synchronize()
    assert sorted(oks) == [False, True, True, True], oks
    assert eager.skipped_steps() == 1 and graph.skipped_steps() == 1
    assert int(graph.step_tensor().item()) == 4
    _same_bits(_state(graph, "plain"), _state(eager, "plain"))
    assert torch.isfinite(graph.params()).all()
    assert not torch.equal(graph.params(), M.flat_from_dict(_params0()).to(cuda))


def test_guard_off_is_the_default_step(cuda):
    xy = _batches(1)[0]
    with torch.cuda.stream(torch.cuda.Stream()):
        engines = []
        for switch in (False, True):
            e = torch.classes.tfd.MnistEngine(B, 0, 0.75, SEED, 0)
            e.set_adam(LR, B1, B2, EPS)
            if switch:
                e.set_skip_nonfinite(True)
                e.set_skip_nonfinite(False)
            e.params().copy_(M.flat_from_dict(_params0()).to(cuda))
            e.sync_shadow()
            _feed(e, xy, cuda)
            e.train_step()
            engines.append(e)
    torch.cuda.synchronize()
    never, off = engines
    _same_bits(_state(never, "plain"), _state(off, "plain"))
    for e in engines:
        assert not e.skip_nonfinite() and e.skipped_steps() == 0 and e.last_step_ok()
        assert e.grad_norm().tolist() == [0.0, 1.0]  # never written: the fused step ran


@pytest.mark.parametrize("which", ["sfb", "zero"])
def test_guard_with_a_sharded_schedule_raises_before_launching(cuda, which):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, "bf16", "plain", True)
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, sfb=which == "sfb", zero=which == "zero")
        if which == "zero":
            e.set_zero(True)
        with pytest.raises(RuntimeError, match="set_skip_nonfinite conflicts with"):
            e.train_step()
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 0 and e.skipped_steps() == 0
    tr.check()
    tr.close()


# ================================================================ two ranks sharing the GPU over IPC
def _ipc_worker(rank, world):
    from tensorflow_distributed_amd.parallel.ipc import make_ipc_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = make_ipc_comm(rank, world, 0, M.TOTAL)
    eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 5, rank)
    eng.set_adam(LR, B1, B2, EPS)
    eng.set_ipc(comm, 1 << 30, True)  # the all-reduce schedule, bf16 wire
    eng.set_skip_nonfinite(True)
    b0, b1 = _batches(2, world * B, seed=7)
    b0 = (_poison(b0[0], B + 2), b0[1])  # a row of rank 1's half
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.params().copy_(M.flat_from_dict(_params0()).to(dev))
        eng.sync_shadow()
        start = {k: t.clone() for k, t in (("p", eng.params()), ("m", eng.adam_m()), ("v", eng.adam_v()),
                                           ("pbf", eng.params_bf16()))}
        _feed(eng, (b0[0][rank * B:(rank + 1) * B], b0[1][rank * B:(rank + 1) * B]), dev)
        eng.train_step()
        torch.cuda.current_stream().synchronize()
        kept = all(torch.equal(_bits(t), _bits(start[k])) for k, t in (("p", eng.params()), ("m", eng.adam_m()),
                                                                      ("v", eng.adam_v()), ("pbf", eng.params_bf16())))
        skipped, ok0, norm0 = eng.skipped_steps(), eng.last_step_ok(), eng.grad_norm()[0].item()
        _feed(eng, (b1[0][rank * B:(rank + 1) * B], b1[1][rank * B:(rank + 1) * B]), dev)
        eng.train_step()
        torch.cuda.current_stream().synchronize()
    torch.cuda.synchronize()
    out = (kept, skipped, ok0, norm0, eng.skipped_steps(), eng.last_step_ok(), eng.params().cpu(),
           int(eng.step_tensor().item()), comm.error(), eng.world(), bool((eng.params() != start["p"]).any().item()))
    comm.close()
    return out


@pytest.mark.timeout(300)
def test_two_ranks_over_ipc_skip_the_poisoned_step_together(cuda):
    """Rank 1's batch is poisoned, rank 0's is clean: the guard reads the all-reduced gradient, so both
    skip. run_ranks waits for each child under a timeout, raises at the first failure and ends the others."""
    res = run_ranks(_ipc_worker, 2, timeout=120)
    for kept, skipped, ok0, norm0, skipped_end, ok1, p, st, err, w, moved in res:
        assert err == 0 and w == 2 and st == 2
        assert not np.isfinite(norm0), "the all-reduced gradient's norm is finite: the poison was lost"
        assert kept and skipped == 1 and ok0 is False
        assert skipped_end == 1 and ok1 is True and moved
        assert torch.isfinite(p).all()
        assert torch.equal(_bits(p), _bits(res[0][6])), "replicas diverged"
