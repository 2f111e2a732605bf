"""Learning-rate schedules evaluated on the device from global_step (csrc/lr_schedule.h): the device
function itself, the flat optimizer ops, the MNIST engine's captured graphs (one GPU and the forced
data-parallel schedules), the unchanged default and the GPU parameter-server shard.

The engine tests compare a multi-step hipGraph whose schedule boundaries fall INSIDE the graph with
eager steps whose constant rate the host sets before every step: the two agree bit for bit only if
the kernels read global_step-before-the-update (Adam's t - 1) and follow TF's inclusive boundaries.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import lr_at, schedule_args

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- 1. the device function
BOUNDS, VALUES = [20, 50], [1e-2, 1e-3, 1e-4]
DECAY, WARM = 100, 4
GRID = sorted({0, 1, 10 ** 6, WARM - 1, WARM} | {b + d for b in BOUNDS for d in (-1, 0, 1)} |
              {DECAY - 1, DECAY, DECAY + 1})
SMOOTH = {
    "exponential": O.ExponentialDecay(0.1, DECAY, 0.96),
    "polynomial": O.PolynomialDecay(0.1, DECAY, end_learning_rate=0.001, power=2.0),
    "cosine": O.CosineDecay(0.1, DECAY, alpha=0.01),
    "warmup_constant": O.ConstantWarmup(0.3, WARM),
    "warmup_exponential": O.ExponentialDecay(0.1, DECAY, 0.96, warmup_steps=WARM),
    "staircase": O.ExponentialDecay(0.1, DECAY, 0.96, staircase=True),
}
# Worst relative error of the device fp32 lr_at() against the fp64 lr_at() over GRID x SMOOTH measured on
# an MI355X: 1.130e-07 (profiles/lr_schedule_eval_err.txt). The bound is 4x that.
MEASURED_REL = 1.130e-07
REL_BOUND = 4 * MEASURED_REL
FLT_MIN = float(np.finfo(np.float32).tiny)


def _eval(cuda, sched, steps):
    st = torch.tensor(list(steps), dtype=torch.int64, device=cuda)
    out = torch.ops.tfd.lr_schedule_eval(st, *schedule_args(sched))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rel(dev, ref):
    """Relative error; below the smallest normal float32 the format carries no relative precision (the
    exponential at step 10^6 is 1e-179 in fp64 and 0 in fp32), so the denominator is floored there."""
    return abs(float(dev) - ref) / max(abs(ref), FLT_MIN)


def test_eval_constant_and_piecewise_are_exact(cuda):
    got = _eval(cuda, 0.0123, GRID)
    assert got.dtype == np.float32 and (got == np.float32(0.0123)).all()
    sc = O.PiecewiseConstant(BOUNDS, VALUES)
    got = _eval(cuda, sc, GRID)
    want = np.array([VALUES[0] if s <= BOUNDS[0] else VALUES[1] if s <= BOUNDS[1] else VALUES[2] for s in GRID],
                    dtype=np.float32)
    assert (got == want).all(), (GRID, got, want)
    assert (want == np.array([lr_at(sc, s) for s in GRID], dtype=np.float32)).all()
    four = O.PiecewiseConstant([1, 2, 3, 4], [5.0, 4.0, 3.0, 2.0, 1.0])
    assert _eval(cuda, four, range(7)).tolist() == [5.0, 5.0, 4.0, 3.0, 2.0, 1.0, 1.0]
    assert _eval(cuda, O.PiecewiseConstant([], [0.5]), GRID).tolist() == [0.5] * len(GRID)


def test_eval_staircase_is_constant_within_a_stair(cuda):
    sc = O.ExponentialDecay(0.1, DECAY, 0.96, staircase=True)
    got = _eval(cuda, sc, range(0, 3 * DECAY))
    for k in range(3):
        stair = got[k * DECAY:(k + 1) * DECAY]
        assert (stair == stair[0]).all()
    assert got[0] > got[DECAY] > got[2 * DECAY]


def test_eval_smooth_kinds_track_fp64(cuda):
    assert REL_BOUND < 1e-4
    worst = {}
    for name, sc in SMOOTH.items():
        dev = _eval(cuda, sc, GRID)
        errs = [_rel(d, lr_at(sc, s)) for d, s in zip(dev, GRID)]
        worst[name] = max(errs)
        print(f"lr_schedule_eval {name}: worst rel err {max(errs):.3e} at step {GRID[int(np.argmax(errs))]}")
    print(f"lr_schedule_eval worst rel err over the grid: {max(worst.values()):.3e} (bound {REL_BOUND:.3e})")
    assert max(worst.values()) <= REL_BOUND, worst
    # mutation check: an off-by-one in s moves the exponential by |ln 0.96| / 100 = 4e-4 relative, which
    # the bound must tell apart wherever the value is a normal float
    sc = SMOOTH["exponential"]
    dev = _eval(cuda, sc, GRID)
    for d, s in zip(dev, GRID):
        if lr_at(sc, s + 1) > FLT_MIN:
            assert _rel(d, lr_at(sc, s + 1)) > REL_BOUND, s
            assert _rel(d, lr_at(sc, max(s - 1, 0))) > REL_BOUND or s == 0, s


def test_eval_rejects_bad_schedules(cuda):
    st = torch.zeros(1, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError):
        torch.ops.tfd.lr_schedule_eval(st, "piecewise", [0.1], [5, 2], [1.0, 0.1, 0.01])
    with pytest.raises(RuntimeError):
        torch.ops.tfd.lr_schedule_eval(st, "piecewise", [0.1], [1, 2, 3, 4, 5], [1.0] * 6)
    with pytest.raises(RuntimeError):
        torch.ops.tfd.lr_schedule_eval(st, "exponential", [0.1, 0.0, 0.96])
    with pytest.raises(RuntimeError):
        torch.ops.tfd.lr_schedule_eval(st, "nope", [0.1])
    for bad in (100.5, float("nan"), float("inf"), 1e30):  # decay_steps / warmup_steps: integral, in range
        with pytest.raises(RuntimeError):
            torch.ops.tfd.lr_schedule_eval(st, "exponential", [0.1, bad, 0.96])
        with pytest.raises(RuntimeError):
            torch.ops.tfd.lr_schedule_eval(st, "exponential", [0.1, 100.0, 0.96, 0.0, 1.0, 0.0, bad])


# ---------------------------------------------------------------- 2. the flat ops
N_FLAT = 1027  # one block of float4 lanes plus the 3-element scalar tail
FLAT_SCHED = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])


def _flat_state(cuda):
    """An Adam state as Adam leaves one: v >= m^2, so |m| / sqrt(v) <= 1 before the step and the update
    stays O(lr). (With v drawn independently of m some elements have v << m^2 and an update of O(1),
    where ANY fp32 evaluation differs from fp64 by more than the absolute tolerance.)"""
    g = torch.Generator().manual_seed(7)
    p = torch.randn(N_FLAT, generator=g)
    m = torch.randn(N_FLAT, generator=g) * 1e-2
    v = m * m + torch.rand(N_FLAT, generator=g) * 1e-4
    gr = torch.randn(N_FLAT, generator=g) * 1e-1
    return [t.to(cuda) for t in (p, m, v, gr)]


@pytest.mark.parametrize("s", [2, 3, 5, 6])
def test_flat_ops_follow_the_device_step(cuda, s):
    ops = torch.ops.tfd
    step = torch.tensor([s], dtype=torch.int64, device=cuda)
    lr_dev = float(_eval(cuda, FLAT_SCHED, [s])[0])
    assert lr_dev == float(np.float32(lr_at(FLAT_SCHED, s)))
    kind, params, bounds, values = schedule_args(FLAT_SCHED)
    # Adam: t = step + 1, the schedule reads s = step
    p, m, v, g = _flat_state(cuda)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    ops.adam_flat(p, m, v, g, None, params[0], 0.9, 0.999, 1e-8, step, 1.0, 1, kind, params, bounds, values)
    ops.adam_flat(p2, m2, v2, g, None, lr_dev, 0.9, 0.999, 1e-8, step)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)
    # momentum
    p, m, _, g = _flat_state(cuda)
    p2, m2 = p.clone(), m.clone()
    ops.momentum_flat(p, m, g, None, params[0], 0.9, 1e-4, False, 1.0, step, 1, kind, params, bounds, values)
    ops.momentum_flat(p2, m2, g, None, lr_dev, 0.9, 1e-4, False, 1.0)
    assert torch.equal(p, p2) and torch.equal(m, m2)
    with pytest.raises(RuntimeError):  # the positional lr must agree with the schedule's base rate
        ops.adam_flat(p, m, v, g, None, 123.0, 0.9, 0.999, 1e-8, step, 1.0, 1, kind, params, bounds, values)
    with pytest.raises(RuntimeError):  # a schedule without the step tensor is an error, not a constant
        ops.momentum_flat(p, m, g, None, params[0], 0.9, 1e-4, False, 1.0, None, 1, kind, params, bounds, values)


def test_flat_adam_exponential_step_matches_fp64(cuda):
    sc = O.ExponentialDecay(0.1, 100, 0.96)
    s = 250
    step = torch.tensor([s], dtype=torch.int64, device=cuda)
    p, m, v, g = _flat_state(cuda)
    pd, md, vd, gd = (t.double().cpu() for t in (p, m, v, g))
    torch.ops.tfd.adam_flat(p, m, v, g, None, 0.1, 0.9, 0.999, 1e-8, step, 1.0, 1, *schedule_args(sc))
    t = s + 1
    lr_t = 0.1 * 0.96 ** 2.5 * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
    md = md + (gd - md) * (1 - 0.9)
    vd = vd + (gd * gd - vd) * (1 - 0.999)
    pd = pd - lr_t * md / (vd.sqrt() + 1e-8)
    torch.testing.assert_close(p.cpu().double(), pd, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- 3. the engine, one GPU
ENG_B, ENG_ROWS = 32, 64
ENG_SCHED = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])


def _host_lr(s, bounds=(2, 5), values=(1e-2, 1e-3, 1e-4)):
    """TF's inclusive convention, spelled out: the rate of the update that starts at global_step s."""
    return values[0] if s <= bounds[0] else values[1] if s <= bounds[1] else values[2]


def _dataset(cuda, rows, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(rows, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=cuda, generator=g)
    perm = torch.randperm(rows, device=cuda, generator=g).to(torch.int32)
    return data, labels, perm


def _set_opt(e, opt, lr):
    if opt == "momentum":
        e.set_momentum(lr, 0.9, False)
    else:
        e.set_adam(lr, 0.9, 0.999, 1e-8)


def _engine(cuda, ds, dtype, opt, B=ENG_B, keep=0.75):
    e = torch.classes.tfd.MnistEngine(B, 0, keep, 1234, 0)
    e.set_dtype(dtype)
    _set_opt(e, opt, 1e-2)
    if opt == "adam_unfused":
        e.set_fused_tail(False)
    e.params().copy_(M.flat_from_dict(M.init_params(13)).to(cuda) * 0.05)
    e.sync_shadow()
    e.set_dataset(*ds)
    e.set_input_mode(1)
    return e


def _state(e):
    return [e.params().clone(), e.adam_m().clone(), e.adam_v().clone(), e.params_bf16().clone()]


@pytest.mark.parametrize("opt", ["adam", "adam_unfused", "momentum"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_graph_follows_schedule_across_boundaries(cuda, dtype, opt):
    stream = torch.cuda.Stream()
    ds = _dataset(cuda, ENG_ROWS)
    with torch.cuda.stream(stream):
        eager = _engine(cuda, ds, dtype, opt)
        for s in range(8):  # the oracle: the host sets the constant rate of every step
            _set_opt(eager, opt, _host_lr(s))
            eager.train_step()
        graph = _engine(cuda, ds, dtype, opt)
        graph.set_lr_schedule(*schedule_args(ENG_SCHED))
        graph.capture_train_steps("g", 4)  # steps 0..3 and 4..7: both boundaries fall inside a graph
        graph.replay("g", 2)
        moved = _engine(cuda, ds, dtype, opt)
        moved.set_lr_schedule(*schedule_args(O.PiecewiseConstant([1, 4], ENG_SCHED.values)))
        moved.capture_train_steps("g", 4)
        moved.replay("g", 2)
    torch.cuda.synchronize()
    assert int(graph.step_tensor().item()) == int(eager.step_tensor().item()) == 8
    for name, a, b in zip(("params", "adam_m", "adam_v", "params_bf16"), _state(graph), _state(eager)):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
    assert [graph.lr_at_step(s) for s in range(8)] == [float(np.float32(_host_lr(s))) for s in range(8)]
    # mutation check: boundaries one step earlier (what reading t for t - 1 amounts to) must show
    assert not torch.equal(moved.params(), eager.params())


# ---------------------------------------------------------------- 4. forced DP at world 1
@pytest.mark.parametrize("name,sfb,zero,mr", [("allreduce", False, False, False), ("sfb", True, False, False),
                                             ("sfb+zero+mr", True, True, True)])
def test_dp_graph_follows_schedule_across_boundaries(cuda, name, sfb, zero, mr):
    """The DP schedules over the real communicator (the deferred fc optimizer reading the head's t,
    the ZeRO ranges launch, the merged tail): two eager steps, then a 3-step graph replayed twice, so
    the boundaries at 2 and 5 are crossed inside the graph."""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    stream = torch.cuda.Stream()
    ds = _dataset(cuda, 1024)
    trs = []
    with torch.cuda.stream(stream):
        engs = []
        for _ in range(2):
            e = _engine(cuda, ds, "bf16", "adam", B=128)
            trs.append(attach_engine(e, 0, 1, cuda, mode="rccl", force_dp=True, sfb=sfb))
            if zero:
                e.set_zero(True)
            e.set_sfb_merge_reduce(mr)
            engs.append(e)
        graph, eager = engs
        for s in range(8):
            _set_opt(eager, "adam", _host_lr(s))
            eager.train_step()
        graph.set_lr_schedule(*schedule_args(ENG_SCHED))
        graph.train_step()
        graph.train_step()
        graph.capture_train_steps("t", 3)
        graph.replay("t", 2)
        for e in engs:
            e.sync_params()
    torch.cuda.synchronize()
    for tr in trs:
        tr.check()
    assert graph.dp() and eager.dp()
    assert int(graph.step_tensor().item()) == int(eager.step_tensor().item()) == 8
    assert torch.equal(graph.params(), eager.params())
    assert torch.equal(graph.adam_v(), eager.adam_v())
    assert torch.equal(graph.params_bf16(), eager.params_bf16())
    for tr in trs:
        tr.close()


# ---------------------------------------------------------------- 5. the default is unchanged
def test_constant_schedule_is_the_default(cuda):
    stream = torch.cuda.Stream()
    ds = _dataset(cuda, ENG_ROWS)
    with torch.cuda.stream(stream):
        plain = _engine(cuda, ds, "bf16", "adam")
        const = _engine(cuda, ds, "bf16", "adam")
        const.set_lr_schedule("constant", [1e-2], [], [])
        for e in (plain, const):
            e.train_step()
            e.capture_train_steps("g", 4)
            e.replay("g", 1)
    torch.cuda.synchronize()
    assert int(plain.step_tensor().item()) == int(const.step_tensor().item()) == 5
    for a, b in zip(_state(plain), _state(const)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- 6. the GPU parameter server
@pytest.mark.parametrize("kind", ["adam", "momentum"])
def test_gpu_ps_shard_follows_schedule(cuda, kind):
    """One shard of 64 parameters, 4 updates across the boundaries: the host FlatApplier within the
    tolerance of tests/test_gpu_ps_gpu.py (rtol 1e-5, atol 1e-6)."""
    n = 64
    sc = O.PiecewiseConstant([0, 2], [1e-1, 1e-2, 1e-3])
    opt = O.AdamOptimizer(sc) if kind == "adam" else O.MomentumOptimizer(sc, 0.9)
    shard = torch.classes.tfd.GpuPsShard(0, torch.tensor([[0, n]], dtype=torch.int64), n, 1,
                                         0 if kind == "adam" else 2, 1e-1, 0.9, 0.999, 1e-8, 0.9, False)
    shard.set_lr_schedule(*schedule_args(sc))
    g = torch.Generator().manual_seed(2)
    ref = torch.randn(n, generator=g) * 0.05
    shard.load_state(ref.to(cuda), None, None, 0)
    ap = O.FlatApplier(opt, n)
    const = O.FlatApplier(O.AdamOptimizer(1e-1) if kind == "adam" else O.MomentumOptimizer(1e-1, 0.9), n)
    ref_const = ref.clone()
    for s in range(4):
        gr = torch.randn(n, generator=g) * 1e-2
        assert shard.current_lr() == float(np.float32(lr_at(sc, s)))
        shard.test_mailbox_slot(0).copy_(gr.to(cuda))
        torch.cuda.synchronize()
        shard.apply(0, 1.0)
        ap.apply(ref, gr)
        const.apply(ref_const, gr)
    assert shard.updates() == 4
    got = shard.params().cpu()
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
    assert not torch.allclose(got, ref_const, rtol=1e-5, atol=1e-6)  # the constant base rate lands elsewhere
