"""Exponential moving average of the weights, updated inside the optimizer kernels (csrc/ema.h,
csrc/kernels/optim_ema.hip, mnist_tail_ema.hip, MnistEngine.set_ema): exact cases through the flat
ops, d_t on the device, that EMA changes nothing else, the fused variants against the stand-alone
kernel bit for bit and against the fp64 definition, captured graphs, the step's topology, the forced
data-parallel schedules at world 1, two ranks over IPC, evaluation from the averages and the runner's
checkpoint round trip.

Engines run at batch 5 on a synthetic 64-row dataset, on a side stream.
"""
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import schedule_args

from dist_util import run_ranks

pytestmark = pytest.mark.gpu

B, ROWS = 5, 64
LR, MOM = 1e-2, 0.9
DECAY = 0.9  # with num_updates d_t = min(0.9, (1 + t) / (10 + t)) moves over the first 8 steps (0.18 .. 0.5)
SCHED = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])  # both boundaries inside a 4-step graph
U = 2.0 ** -24  # fp32 unit roundoff


# ---------------------------------------------------------------- helpers
def _dataset(cuda, rows=ROWS, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(rows, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=cuda, generator=g)
    perm = torch.randperm(rows, device=cuda, generator=g).to(torch.int32)
    return data, labels, perm


def _engine(cuda, ds, dtype="bf16", opt="adam", ema=None, nu=True, clip=None, keep=0.75, batch=B):
    e = torch.classes.tfd.MnistEngine(batch, 0, keep, 1234, 0)
    e.set_dtype(dtype)
    if opt == "momentum":
        e.set_momentum(LR, MOM, False)
    else:
        e.set_adam(LR, 0.9, 0.999, 1e-8)
    if opt == "adam_piecewise":
        e.set_lr_schedule(*schedule_args(SCHED))
    if clip is not None:
        e.set_clip_norm(clip)
    e.params().copy_(M.flat_from_dict(M.init_params(13)).to(cuda) * 0.05)
    e.sync_shadow()
    e.set_dataset(*ds)
    e.set_input_mode(1)
    if ema is not None:
        e.set_ema(ema, nu)  # after the parameters: the shadow starts as their copy
    return e


def _state(e, ema=False):
    s = {"params": e.params().clone(), "adam_m": e.adam_m().clone(), "adam_v": e.adam_v().clone(),
         "params_bf16": e.params_bf16().clone(), "step": e.step_tensor().clone(), "loss": e.loss_rows().clone()}
    if ema:
        s["ema"] = e.ema_params().clone()
    return s


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())


_NORM0 = {}


def _norm0(cuda, dtype):
    """Step-0 gradient norm of an unclipped engine (computed once per dtype, shared by the tests)."""
    if dtype not in _NORM0:
        with torch.cuda.stream(torch.cuda.Stream()):
            e = _engine(cuda, _dataset(cuda), dtype)
            e.set_fused_tail(0)
            e.train_step()
        torch.cuda.synchronize()
        _NORM0[dtype] = float(e.grads().double().norm().item())
    return _NORM0[dtype]


# ---------------------------------------------------------------- 1. exact case through the flat ops
# 3,274,634 is above one grid pass of 2048 x 256 x 4 and has n % 4 == 2: the stride loop and the scalar tail
N_PARAMS = 3274634
LENGTHS = [1, 3, 4, 5, 255, 1025, 262147, N_PARAMS, M.TOTAL]


def _exact_inputs(cuda, n, seed):
    """p and e0 small integers times 2^-3: p - e and every halving of it are exact in fp32."""
    g = torch.Generator(device=cuda).manual_seed(seed)
    p = torch.randint(-8, 9, (n,), device=cuda, generator=g).float() * 0.125
    e0 = torch.randint(-8, 9, (n,), device=cuda, generator=g).float() * 0.125
    grad = torch.randn(n, device=cuda, generator=g)
    return p, e0, grad


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
@pytest.mark.parametrize("op", ["adam", "momentum"])
def test_flat_ops_exact_case(cuda, op, gdt):
    """lr = 0 leaves p' = p bit for bit, decay 0.5: after n updates e = p + (e0 - p) 2^-n exactly.
    adam_flat takes the shadow as trailing arguments, momentum_flat through momentum_ema_flat."""
    ops = torch.ops.tfd
    assert N_PARAMS % 4 == 2 and N_PARAMS > 2048 * 256 * 4
    for n in LENGTHS:
        p0, e0, grad = _exact_inputs(cuda, n, n % 1000)
        grad = grad.to(gdt)
        for with_pbf in (False, True):
            run = {}
            for ema in (False, True):
                p, m, v = p0.clone(), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
                pbf = torch.zeros(n, device=cuda, dtype=torch.bfloat16) if with_pbf else None
                e = e0.clone()
                tail = (e, 0.5, False) if ema else ()
                for i in range(6):
                    step = torch.tensor([i], device=cuda)
                    if op == "adam":
                        ops.adam_flat(p, m, v, grad, pbf, 0.0, 0.9, 0.999, 1e-8, step, 1.0, 1, "constant", [], [], [],
                                      None, *tail)
                    elif ema:  # momentum_flat with the shadow: an op of its own
                        ops.momentum_ema_flat(p, m, grad, pbf, 0.0, MOM, 0.0, False, 1.0, None, 1, "constant", [], [], [],
                                              None, ema=e, ema_decay=0.5, ema_num_updates=False)
                    else:
                        ops.momentum_flat(p, m, grad, pbf, 0.0, MOM, 0.0, False, 1.0, None, 1, "constant", [], [], [],
                                          None)
                    if ema:
                        want = (p0.double() + (e0.double() - p0.double()) * 0.5 ** (i + 1)).float()
                        assert torch.equal(e, want), (op, n, with_pbf, i, (e - want).abs().max().item())
                run[ema] = (p, m, v, pbf)
            assert torch.equal(run[True][0], p0)
            for a, b in zip(run[True], run[False]):
                assert (a is None and b is None) or torch.equal(a, b), (op, n, with_pbf)
            assert run[True][1].abs().max() > 0  # the slots did move


def test_ema_flat_exact_case(cuda):
    ops = torch.ops.tfd
    for n in LENGTHS:
        p, e0, _ = _exact_inputs(cuda, n, 7 + n % 1000)
        for off in (0, 1):  # 16-B aligned, and not (the scalar form)
            pp, e = p[off:], e0[off:].clone()
            if pp.numel() == 0:
                continue
            for i in range(6):
                ops.ema_flat(e, pp, 0.5)
                want = (pp.double() + (e0[off:].double() - pp.double()) * 0.5 ** (i + 1)).float()
                assert torch.equal(e, want), (n, off, i)
    with pytest.raises(RuntimeError, match="ema_decay"):
        ops.ema_flat(torch.zeros(4, device=cuda), torch.zeros(4, device=cuda), 1.0)
    with pytest.raises(RuntimeError, match="ema_decay"):
        ops.ema_flat(torch.zeros(4, device=cuda), torch.zeros(4, device=cuda), 0.0)
    with pytest.raises(RuntimeError, match="size"):
        ops.ema_flat(torch.zeros(5, device=cuda), torch.zeros(4, device=cuda), 0.5)


# ---------------------------------------------------------------- 2. d_t on the device
def test_decay_follows_the_device_step(cuda):
    """One update from e = 1, p = 0 leaves e = 1 - (1 - d_t). The bound is the one derived beside the
    helper (csrc/ema.h): the division rounds d_t by at most 2^-25 d_t, 1 - d_t rounds by at most 2^-25,
    and 1 - omd is exact or rounds by 2^-25 again: 3 * 2^-25 < 2 * 2^-24."""
    ops = torch.ops.tfd
    n, bound, worst = 6, 2 * U, 0.0
    for s in range(12):
        step = torch.tensor([s], device=cuda)
        t = s + 1
        want = min(0.5, (1.0 + t) / (10.0 + t))
        assert want == O.ema_decay_at(0.5, t, True)
        got = {}
        z = lambda: torch.zeros(n, device=cuda)  # noqa: E731
        e = torch.ones(n, device=cuda)
        ops.adam_flat(z(), z(), z(), z(), None, 0.0, 0.9, 0.999, 1e-8, step, 1.0, 1, "constant", [], [], [], None, e, 0.5,
                      True)
        got["adam"] = e
        e = torch.ones(n, device=cuda)
        ops.momentum_ema_flat(z(), z(), z(), None, 0.0, MOM, 0.0, False, 1.0, step, 1, "constant", [], [], [], None,
                              ema=e, ema_decay=0.5, ema_num_updates=True)
        got["momentum"] = e
        e = torch.ones(n, device=cuda)
        ops.ema_flat(e, z(), 0.5, True, step, 1)
        got["ema_flat"] = e
        for k, e in got.items():
            err = (e.double() - want).abs().max().item()
            worst = max(worst, err)
            assert err <= bound, (k, s, err)
            assert torch.equal(e, got["ema_flat"]), (k, s)  # one helper: the same bits everywhere
        if t >= 8:
            assert torch.equal(got["adam"], torch.full((n,), 0.5, device=cuda))  # min() has switched to decay
    print(f"ema d_t worst abs err {worst:.3e} (bound {bound:.3e})")
    with pytest.raises(RuntimeError, match="step"):
        ops.momentum_ema_flat(torch.zeros(4, device=cuda), None, torch.zeros(4, device=cuda), None, 0.0, 0.0, 0.0, False,
                              1.0, None, 1, "constant", [], [], [], None, ema=torch.zeros(4, device=cuda), ema_decay=0.5,
                              ema_num_updates=True)


# ---------------------------------------------------------------- 3. EMA changes nothing else
@pytest.mark.parametrize("opt", ["adam", "momentum", "adam_piecewise"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ema_changes_nothing_else(cuda, dtype, opt):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        off = _engine(cuda, ds, dtype, opt)
        on = _engine(cuda, ds, dtype, opt, ema=DECAY)
        e0 = on.ema_params().clone()
        assert torch.equal(e0, on.params())  # starts as a copy of the parameters
        for _ in range(8):
            off.train_step()
            on.train_step()
    torch.cuda.synchronize()
    assert int(on.step_tensor().item()) == 8 and on.ema_decay() == DECAY and off.ema_decay() == 0
    _same(_state(on), _state(off))
    assert not torch.equal(on.ema_params(), e0) and not torch.equal(on.ema_params(), on.params())
    with pytest.raises(RuntimeError, match="set_ema first"):
        off.ema_params()
    with pytest.raises(RuntimeError, match="set_ema"):
        off.set_ema(1.0, True)


# ---------------------------------------------------------------- 4 + 5. fused equals stand-alone; the fp64 definition
# Per-element bound of the shadow against the fp64 recurrence fed the device's own fp32 parameters. One
# update computes fl(e + omd_f * fl(p' - e)): the subtraction rounds by u |p' - e| (u = 2^-24), omd_f is
# within u of 1 - d_t (the division's u d_t and the subtraction's u (1 - d_t), csrc/ema.h) so it adds
# u |p' - e|, and the fused multiply-add rounds by u |e'|. With X = max(|e|, |p'|) over the update's
# operands and result, |p' - e| <= 2 X and |e'| <= X: at most (2 + 2 + 1) u X = 5 u X per update, c = 5.
# The error carried in from earlier updates is multiplied by d_t <= 1, so errors add and never grow:
# after n updates |e_n - ref_n| <= n * 5 * 2^-24 * X, X the largest |e| or |p'| the element took so far.
EMA_C = 5.0

TRAJECTORIES = {"fused_bf16": ("bf16", 1, False), "fused_fp32": ("fp32", 1, False), "unfused_bf16": ("bf16", 0, False),
                "unfused_fp32": ("fp32", 0, False), "clip_bf16": ("bf16", 1, True), "clip_fp32": ("fp32", 1, True)}
_WORST = {}


def _check_fp64(got, ref64, mag, n, what):
    bound = n * EMA_C * U * mag
    err = (got.double() - ref64).abs()
    ok = bool((err <= bound).all().item())
    ratio = float((err / bound.clamp_min(1e-300)).max().item())
    return ok, ratio


@pytest.mark.parametrize("which", list(TRAJECTORIES))
def test_fused_equals_standalone_and_tracks_fp64(cuda, which):
    """After each of 8 eager steps the engine's shadow equals, bit for bit, ema_flat applied to a copy of
    it kept here, from the engine's own params(); and it stays within n * 5 * 2^-24 * X of the fp64
    recurrence (EMA_C above). Measured worst ratio to the bound on an MI355X: see profiles/ema_err.txt."""
    ops = torch.ops.tfd
    dtype, fused, clipped = TRAJECTORIES[which]
    clip = 0.05 * _norm0(cuda, dtype) if clipped else None
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), dtype, "adam", ema=DECAY, clip=clip)
        e.set_fused_tail(fused)
        ref = e.ema_params().clone()
        ref64 = ref.double()
        mag = ref64.abs()
        worst = 0.0
        for n in range(1, 9):
            e.train_step()
            ops.ema_flat(ref, e.params(), DECAY, True, e.step_tensor(), 0)  # t = global_step after the update
            got = e.ema_params()
            assert torch.equal(got, ref), (which, n, (got - ref).abs().max().item())
            ref64 = O.ema_update(ref64, e.params(), DECAY, n, True)
            mag = torch.maximum(mag, torch.maximum(ref64.abs(), e.params().double().abs()))
            ok, ratio = _check_fp64(got, ref64, mag, n, which)
            worst = max(worst, ratio)
            assert ok, (which, n, ratio)
        if clipped:
            assert float(e.grad_norm()[1].item()) < 1  # still clipping
        # a 1.02x mutation of one 64-element slice must fail the check
        bad = e.ema_params().clone()
        sl = slice(M.BUCKET_SPLIT + 4096, M.BUCKET_SPLIT + 4096 + 64)
        assert (bad[sl] != 0).all()
        bad[sl] *= 1.02
        ok, _ = _check_fp64(bad, ref64, mag, 8, which)
        assert not ok
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 8
    _WORST[which] = worst
    print(f"ema fp64 worst err / bound, {which}: {worst:.4f}")
    assert worst > 0  # the check is not vacuous: fp32 did round


# ---------------------------------------------------------------- 6. graphs
def _three_ways(make):
    eager, one, four = make(), make(), make()
    for _ in range(8):
        eager.train_step()
    one.train_step()
    one.capture_train_step("g1")
    one.replay("g1", 7)
    four.capture_train_steps("g4", 4)
    four.replay("g4", 2)
    torch.cuda.synchronize()
    for e in (one, four):
        assert int(e.step_tensor().item()) == int(eager.step_tensor().item()) == 8
        _same(_state(e, True), _state(eager, True))
    return eager, one, four


@pytest.mark.parametrize("opt", ["adam", "adam_piecewise"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ema_graphs_equal_eager(cuda, dtype, opt):
    """num_updates on: d_t moves inside the graph, read from the device step counter."""
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        eager, _, _ = _three_ways(lambda: _engine(cuda, ds, dtype, opt, ema=DECAY, nu=True))
        const = _engine(cuda, ds, dtype, opt, ema=DECAY, nu=False)
        for _ in range(8):
            const.train_step()
    torch.cuda.synchronize()
    assert torch.equal(const.params(), eager.params())
    assert not torch.equal(const.ema_params(), eager.ema_params())  # num_updates is felt


# ---------------------------------------------------------------- 7. fusion is real; the default is untouched
# capture_topology(1) of the default one-GPU bf16 Adam step at B = 32 (the list pinned by
# tests/test_clip_norm_gpu.py): six kernel nodes in a chain
PARENT_TOPOLOGY = ['node 0 0', 'node 1 0', 'node 2 0', 'node 3 0', 'node 4 0', 'node 5 0',
                   'edge 0 1', 'edge 1 2', 'edge 2 3', 'edge 3 4', 'edge 4 5',
                   'tag conv_fwd@0 0', 'tag fc_fwd@0 1 2', 'tag fc_bwd@0 3', 'tag conv_bwd@0 4', 'tag opt@0 5']


def test_ema_step_keeps_its_six_nodes_and_the_default_is_what_it_was(cuda):
    ds = _dataset(cuda, rows=256)
    with torch.cuda.stream(torch.cuda.Stream()):
        on = _engine(cuda, ds, ema=DECAY, batch=32)
        never = _engine(cuda, ds, batch=32)
        off = _engine(cuda, ds, batch=32)
        off.set_ema(0, True)
        topo = {}
        for name, e in (("on", on), ("never", never), ("off", off)):
            e.capture_train_steps("g", 4)
            e.replay("g", 1)
            topo[name] = list(e.capture_topology(1))
    torch.cuda.synchronize()
    print("ema topology:", topo["on"])
    assert topo["on"] == PARENT_TOPOLOGY  # the shadow's update is inside the optimizer's node
    assert topo["never"] == PARENT_TOPOLOGY and topo["off"] == PARENT_TOPOLOGY
    assert int(never.step_tensor().item()) == 4 and off.ema_decay() == 0
    _same(_state(never), _state(off))
    _same(_state(never), _state(on))


# ---------------------------------------------------------------- 8. forced DP at world 1
@pytest.mark.parametrize("mode,wire,dtype,sfb", [
    ("rccl", "bf16", "bf16", False), ("rccl", "fp32", "bf16", False), ("ipc", "bf16", "bf16", False),
    ("ipc", "fp32", "bf16", False), ("rccl", "fp32", "fp32", False), ("ipc", "fp32", "fp32", False),
    ("rccl", "bf16", "bf16", True), ("ipc", "bf16", "bf16", True)])
def test_forced_dp_world1_ema(cuda, mode, wire, dtype, sfb):
    """The all-reduce schedule (its fc-region optimizer deferred on a stream of its own) and the SFB
    serial schedule over a world-1 communicator."""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    ops = torch.ops.tfd
    ds = _dataset(cuda)
    trs = []

    def make():
        e = _engine(cuda, ds, dtype, "adam", ema=DECAY)
        trs.append(attach_engine(e, 0, 1, cuda, mode=mode, force_dp=True, bf16=wire == "bf16", sfb=sfb))
        assert e.dp() and e.fc_sfb() == sfb
        return e

    with torch.cuda.stream(torch.cuda.Stream()):
        eager, graph = make(), make()
        ref = eager.ema_params().clone()
        for _ in range(8):
            eager.train_step()
            ops.ema_flat(ref, eager.params(), DECAY, True, eager.step_tensor(), 0)
            assert torch.equal(eager.ema_params(), ref)
        graph.capture_train_steps("g", 4)
        graph.replay("g", 2)
        # the deferred fc-region optimizer has finished before the shadow is read
        right_after = graph.ema_params().clone()
        torch.cuda.synchronize()
        assert torch.equal(right_after, graph.ema_params())
        _same(_state(graph, True), _state(eager, True))
    assert int(graph.step_tensor().item()) == 8
    for tr in trs:
        tr.check()
        tr.close()


# ---------------------------------------------------------------- 9. ZeRO-1 raises before launching
@pytest.mark.parametrize("sfb", [False, True], ids=["zero", "sfb+zero"])
def test_ema_with_zero_raises_before_launching(cuda, sfb):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), "bf16", "adam", ema=DECAY)
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, sfb=sfb, zero=True)
        e.set_zero(True)
        before = _state(e, True)
        with pytest.raises(RuntimeError, match="set_ema conflicts with ZeRO-1"):
            e.train_step()
        torch.cuda.synchronize()
        _same(_state(e, True), before)
        assert int(e.step_tensor().item()) == 0
        e.set_ema(0, True)  # off again: the sharded schedule steps
        e.train_step()
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 1
    tr.check()
    tr.close()


# ---------------------------------------------------------------- 10. two ranks sharing the GPU over IPC
def _ipc_worker(rank, world, steps):
    from tensorflow_distributed_amd.parallel.ipc import make_ipc_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = make_ipc_comm(rank, world, 0, M.TOTAL)
    eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 5, rank)
    eng.set_adam(LR, 0.9, 0.999, 1e-8)
    eng.set_ipc(comm, 1 << 30, True)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(steps, world * B, 784, generator=g)
    y = torch.randint(0, 10, (steps, world * B), generator=g, dtype=torch.int32)
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.params().copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()}).to(dev))
        eng.sync_shadow()
        eng.set_ema(DECAY, True)
        for i in range(steps):
            eng.feed_x().copy_(x[i, rank * B:(rank + 1) * B].to(dev))
            eng.feed_y().copy_(y[i, rank * B:(rank + 1) * B].to(dev))
            if i == 0:
                eng.train_step()
                eng.capture_train_step("t")
            else:
                eng.replay("t", 1)
            torch.cuda.current_stream().synchronize()
    torch.cuda.synchronize()
    out = eng.params().cpu(), eng.ema_params().cpu(), int(eng.step_tensor().item()), comm.error(), eng.world()
    comm.close()
    return out


@pytest.mark.timeout(300)
def test_two_ranks_over_ipc_average_identically(cuda):
    """run_ranks waits for each child under a timeout, raises at the first failure and ends the others."""
    res = run_ranks(_ipc_worker, 2, 4, timeout=120)
    for p, e, st, err, w in res:
        assert err == 0 and w == 2 and st == 4
        assert torch.isfinite(p).all() and torch.isfinite(e).all()
        assert torch.equal(p, res[0][0]), "replicas diverged"
        assert torch.equal(e, res[0][1]), "averages diverged"
    assert not torch.equal(res[0][0], res[0][1])


# ---------------------------------------------------------------- 11. evaluation from the averages
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_evaluate_reads_the_averages(cuda, dtype):
    ds = _dataset(cuda)
    g = torch.Generator(device=cuda).manual_seed(11)
    x = torch.rand(7, 784, device=cuda, generator=g)  # 7 rows: a full batch of 5 and a tail of 2
    y = torch.randint(0, 10, (7,), dtype=torch.int32, device=cuda, generator=g)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, ds, dtype, ema=DECAY)
        for _ in range(8):
            e.train_step()
        got = e.evaluate(x, y, True).clone()
        own = e.evaluate(x, y, False).clone()
        assert torch.equal(e.evaluate(x, y), own)  # the default reads the parameters
        assert torch.equal(e.evaluate(x, y, True), got)  # the bf16 image is reused, not stale
        other = _engine(cuda, ds, dtype)
        other.params().copy_(e.ema_params())
        other.sync_shadow()
        want = other.evaluate(x, y, False).clone()
        e.train_step()  # the shadow moves: its image is cast again
        moved = e.evaluate(x, y, True).clone()
        with pytest.raises(RuntimeError, match="set_ema first"):
            other.evaluate(x, y, True)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), (got, want)
    assert got[0].item() != own[0].item()
    assert moved[0].item() != got[0].item()


# ---------------------------------------------------------------- 12. runner round trip
def test_runner_checkpoint_round_trip(cuda):
    from tensorflow_distributed_amd.models.mnist_runner import EMA_SUFFIX, NativeMnistRunner

    g = torch.Generator().manual_seed(5)
    xs = torch.rand(5, B, 784, generator=g)
    ys = torch.randint(0, 10, (5, B), generator=g, dtype=torch.int32)
    opt = O.AdamOptimizer(LR, ema_decay=0.9, ema_num_updates=True)

    def runner():
        r = NativeMnistRunner(B, opt, keep_prob=0.75, seed=3, device=cuda)
        r.load_flat(M.flat_from_dict(M.init_params(13)) * 0.05, {}, 0)
        return r

    a = runner()
    assert torch.equal(a.ema_params(), a.params())
    for i in range(3):
        a.train_step(xs[i], ys[i])
    sd = a.state_dict_tf()
    assert sum(k.endswith(EMA_SUFFIX) for k in sd) == len(M.PARAM_SPECS)
    b = runner()
    b.load_state_dict_tf(sd)
    assert torch.equal(b.ema_params(), a.ema_params()) and not torch.equal(b.ema_params(), b.params())
    for i in range(3, 5):
        a.train_step(xs[i], ys[i])
        b.train_step(xs[i], ys[i])
    assert a.global_step() == b.global_step() == 5
    assert torch.equal(a.params(), b.params())
    assert torch.equal(a.ema_params(), b.ema_params())
    ev = a.evaluate(xs[0], ys[0], use_ema=True)
    assert ev == b.evaluate(xs[0], ys[0], use_ema=True) and ev != a.evaluate(xs[0], ys[0])
    # a checkpoint without the averages: the shadow starts again from the restored values
    c = runner()
    c.load_state_dict_tf({k: v for k, v in sd.items() if not k.endswith(EMA_SUFFIX)})
    assert torch.equal(c.ema_params(), c.params())
