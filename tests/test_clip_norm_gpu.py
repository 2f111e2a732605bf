"""Global-norm gradient clipping on the device (csrc/kernels/grad_norm.hip, optim_clip.hip,
MnistEngine.set_clip_norm): the reduction itself, its accuracy on real gradients, the inactive and the
active clip, captured graphs against eager steps, the forced data-parallel schedule at world 1, two
ranks over IPC, and the default step, which must be what it was.

Engines run at batch 32 on a synthetic 256-row dataset; bit-for-bit comparisons throughout, since the
norm kernels use no atomics and every order of summation is fixed.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import schedule_args

from dist_util import run_ranks

pytestmark = pytest.mark.gpu

B, ROWS = 32, 256
LR, MOM = 1e-2, 0.9
SCHED = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])  # both boundaries inside a 4-step graph
# Worst relative error of the device norm against the fp64 norm of the same gradient buffer over the
# cases of this file (one GPU bf16 / fp32 dtype; forced DP with bf16 / fp32 wire and fp32 dtype, RCCL and IPC),
# measured on an MI355X: 2.780e-08 (profiles/clip_norm_err.txt; the fp32 rounding of the result alone is up to
# 6e-8). The bound is 4x that.
MEASURED_REL = 2.780e-08
REL_BOUND = 4 * MEASURED_REL


# ---------------------------------------------------------------- helpers
def _dataset(cuda, rows=ROWS, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(rows, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=cuda, generator=g)
    perm = torch.randperm(rows, device=cuda, generator=g).to(torch.int32)
    return data, labels, perm


def _engine(cuda, ds, dtype="bf16", opt="adam", clip=None, keep=0.75):
    e = torch.classes.tfd.MnistEngine(B, 0, keep, 1234, 0)
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
    return e


def _state(e):
    return {"params": e.params().clone(), "adam_m": e.adam_m().clone(), "adam_v": e.adam_v().clone(),
            "params_bf16": e.params_bf16().clone(), "step": e.step_tensor().clone()}


def _same(a, b):
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())


def _pair(e):
    torch.cuda.synchronize()
    return e.grad_norm().cpu().numpy().copy()


def _rel_err(e, buf, what):
    """Device norm of the last step against the fp64 norm of the gradient buffer the optimizer read."""
    ref = float(buf.double().norm().item())
    got = float(_pair(e)[0])
    rel = abs(got - ref) / ref
    print(f"clip_norm rel err {what}: device {got!r} fp64 {ref!r} rel {rel:.3e} (bound {REL_BOUND:.3e})")
    return rel


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


# ---------------------------------------------------------------- 1. the reduction covers every element, exactly
# 3,274,634 is the model's parameter count (n % 4 == 2: a scalar tail); the engine's flat buffers are padded
# to M.TOTAL = 3,274,688
N_PARAMS = 3274634
LENGTHS = [1, 3, 4, 5, 255, 1025, 262147, N_PARAMS, M.TOTAL]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_norm_of_ones_is_exact(cuda, dt):
    assert N_PARAMS % 4 == 2 and N_PARAMS <= M.TOTAL
    for n in LENGTHS:
        out = torch.ops.tfd.grad_global_norm(torch.ones(n, dtype=dt, device=cuda), 1e30)
        assert out.dtype == torch.float32 and out.shape == (2,)
        norm, scale = out.cpu().numpy()
        # every partial sum is an integer below 2^24: exact in fp32, so the only rounding is the last
        assert norm == np.float32(np.sqrt(np.float64(n))), (n, norm)
        assert scale == np.float32(1.0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_norm_sees_a_single_element_anywhere(cuda, dt):
    for n in (5, 1025, 262147, N_PARAMS):
        for pos in (0, n - 1, (n - 1) // 4 * 4):  # first, last (the scalar tail), the last multiple of 4
            g = torch.zeros(n, dtype=dt, device=cuda)
            g[pos] = 3.0
            norm, scale = torch.ops.tfd.grad_global_norm(g, 1.5).cpu().numpy()
            assert norm == np.float32(3.0), (n, pos, norm)
            assert scale == np.float32(0.5), (n, pos, scale)


def test_norm_is_bit_identical_run_to_run_and_handles_any_alignment(cuda):
    g = torch.randn(N_PARAMS + 1, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    for buf in (g[:N_PARAMS], g[1:], g[:N_PARAMS].to(torch.bfloat16), g.to(torch.bfloat16)[1:]):
        a = torch.ops.tfd.grad_global_norm(buf, 1.0)
        b = torch.ops.tfd.grad_global_norm(buf, 1.0)
        assert torch.equal(a, b)
        ref = float(buf.double().norm().item())
        assert abs(float(a[0].item()) - ref) / ref < 1e-6
    assert REL_BOUND < 1e-5


def test_norm_scale_argument_and_non_finite_norms(cuda):
    ops = torch.ops.tfd
    g = torch.full((64,), 0.5, device=cuda)  # sum of squares 16, norm 4
    assert ops.grad_global_norm(g, 1.0).tolist() == [4.0, 0.25]
    assert ops.grad_global_norm(g, 1.0, 0.25).tolist() == [1.0, 1.0]  # the averaged gradient's norm
    assert ops.grad_global_norm(g, 0.5, 0.25).tolist() == [1.0, 0.5]
    assert ops.grad_global_norm(g, 4.0).tolist() == [4.0, 1.0]
    g[3] = float("inf")
    assert ops.grad_global_norm(g, 1.0).tolist() == [float("inf"), 0.0]
    g[3] = float("nan")
    norm, scale = ops.grad_global_norm(g, 1.0).tolist()
    assert norm != norm and scale == 1.0  # no special handling: the NaN gradient propagates by itself
    with pytest.raises(RuntimeError):
        ops.grad_global_norm(torch.zeros(0, device=cuda), 1.0)
    with pytest.raises(RuntimeError):
        ops.grad_global_norm(torch.zeros(4, device=cuda, dtype=torch.float64), 1.0)


# ---------------------------------------------------------------- 2. accuracy on real gradients
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_engine_norm_tracks_fp64(cuda, dtype):
    """The bound is 4x the worst error measured on the MI355X; fixed-order fp32 lanes of a few tens of
    adds, a tree and an fp64 finish must stay below 1e-5 whatever was measured."""
    assert REL_BOUND < 1e-5
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), dtype, clip=1e30)
        e.train_step()
    torch.cuda.synchronize()
    assert e.clip_norm() == 1e30
    assert _rel_err(e, e.grads(), f"one GPU {dtype}") <= REL_BOUND


# ---------------------------------------------------------------- 3. an inactive clip changes no bit
@pytest.mark.parametrize("opt", ["adam", "momentum"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_inactive_clip_changes_no_bit(cuda, dtype, opt):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        plain = _engine(cuda, ds, dtype, opt)
        plain.set_fused_tail(0)
        clipped = _engine(cuda, ds, dtype, opt, clip=1e30)
        for _ in range(6):
            plain.train_step()
            clipped.train_step()
    torch.cuda.synchronize()
    assert int(clipped.step_tensor().item()) == 6
    _same(_state(clipped), _state(plain))
    assert _pair(clipped)[1] == np.float32(1.0)
    assert _pair(plain).tolist() == [0.0, 1.0]  # never written without clipping


# ---------------------------------------------------------------- 4. an active clip is what it says
@pytest.mark.parametrize("opt", ["adam", "momentum"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_active_clip_scales_the_gradient_by_clip_over_norm(cuda, dtype, opt):
    ops = torch.ops.tfd
    clip = 0.5 * _norm0(cuda, dtype)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), dtype, opt, clip=clip)
        before = _state(e)
        e.train_step()
    torch.cuda.synchronize()
    norm, scale = _pair(e)
    assert scale < 1
    assert scale == np.float32(clip) / norm  # fp32 division, bit for bit
    assert abs(float(norm) - 2 * clip) / (2 * clip) <= REL_BOUND
    after = _state(e)
    assert int(after["step"].item()) == 1

    def flat(grad_scale, gscale):
        p, m, v, pbf = (before[k].clone() for k in ("params", "adam_m", "adam_v", "params_bf16"))
        if opt == "adam":  # t = the engine's bumped step: t_offset 0
            ops.adam_flat(p, m, v, e.grads(), pbf, LR, 0.9, 0.999, 1e-8, e.step_tensor(), grad_scale, 0, "constant",
                          [], [], [], gscale)
        else:
            ops.momentum_flat(p, m, e.grads(), pbf, LR, MOM, 0.0, False, grad_scale, None, 0, "constant", [], [], [],
                              gscale)
        torch.cuda.synchronize()
        return {"params": p, "adam_m": m, "adam_v": v, "params_bf16": pbf, "step": after["step"]}

    _same(flat(float(scale), None), after)              # the host-read factor as grad_scale
    _same(flat(1.0, e.grad_norm()[1:2]), after)         # the same factor read by the kernel from the device
    unclipped = flat(1.0, None)
    assert not torch.equal(unclipped["params"], after["params"])
    with pytest.raises(RuntimeError):
        flat(1.0, e.grad_norm())  # two elements: not a clip factor


# ---------------------------------------------------------------- 5. graph equals eager
def _graph_vs_eager(make):
    eager, graph = make(), make()
    for _ in range(8):
        eager.train_step()
    graph.capture_train_steps("g", 4)
    graph.replay("g", 2)
    torch.cuda.synchronize()
    assert int(graph.step_tensor().item()) == int(eager.step_tensor().item()) == 8
    _same(_state(graph), _state(eager))
    pe, pg = _pair(eager), _pair(graph)
    assert pe.tobytes() == pg.tobytes(), (pe, pg)
    assert pe[1] < 1, pe  # still clipping at step 8
    return eager, graph


@pytest.mark.parametrize("opt", ["adam", "momentum", "adam_piecewise"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_clipped_graph_equals_eager(cuda, dtype, opt):
    ds = _dataset(cuda)
    clip = 0.05 * _norm0(cuda, dtype)
    with torch.cuda.stream(torch.cuda.Stream()):
        eager, graph = _graph_vs_eager(lambda: _engine(cuda, ds, dtype, opt, clip=clip))
        # the clip is felt: the same eight steps unclipped land elsewhere
        plain = _engine(cuda, ds, dtype, opt)
        for _ in range(8):
            plain.train_step()
    torch.cuda.synchronize()
    assert not torch.equal(plain.params(), eager.params())


# ---------------------------------------------------------------- 6. forced DP at world 1
@pytest.mark.parametrize("mode,wire,dtype", [("rccl", "bf16", "bf16"), ("rccl", "fp32", "bf16"), ("ipc", "bf16", "bf16"),
                                             ("ipc", "fp32", "bf16"), ("rccl", "fp32", "fp32"), ("ipc", "fp32", "fp32")])
def test_forced_dp_world1_clipped_graph_equals_eager(cuda, mode, wire, dtype):
    """The all-reduce schedule over a world-1 communicator, bf16 and fp32 wire (and the fp32 dtype, whose
    wire is fp32 and whose gradient is one bucket)."""
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    ds = _dataset(cuda)
    clip = 0.05 * _norm0(cuda, dtype)
    trs = []

    def make():
        e = _engine(cuda, ds, dtype, "adam", clip=clip)
        trs.append(attach_engine(e, 0, 1, cuda, mode=mode, force_dp=True, bf16=wire == "bf16"))
        assert e.dp()
        return e

    with torch.cuda.stream(torch.cuda.Stream()):
        eager, graph = _graph_vs_eager(make)
    for tr in trs:
        tr.check()
    # the norm is that of the buffer the optimizer read: the bf16 wire buffer, or the fp32 gradients
    buf = eager.grads_bf16() if wire == "bf16" else eager.grads()
    assert _rel_err(eager, buf, f"forced DP {mode} {dtype} dtype {wire} wire") <= REL_BOUND
    if wire == "bf16":  # ... and not of the other one (the fp32 buffer holds no reduced gradient here)
        other = float(eager.grads().double().norm().item())
        assert abs(float(_pair(eager)[0]) - other) / max(other, 1e-30) > REL_BOUND
    for tr in trs:
        tr.close()


@pytest.mark.parametrize("which", ["sfb", "zero"])
def test_clip_with_a_sharded_schedule_raises_before_launching(cuda, which):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), "bf16", "adam", clip=1.0)
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, sfb=which == "sfb", zero=which == "zero")
        if which == "zero":
            e.set_zero(True)
        else:
            assert e.fc_sfb()
        before = _state(e)
        with pytest.raises(RuntimeError, match="set_clip_norm conflicts with"):
            e.train_step()
        torch.cuda.synchronize()
        _same(_state(e), before)
        assert int(e.step_tensor().item()) == 0
        e.set_clip_norm(0)  # off again: the sharded schedule steps
        e.train_step()
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 1
    tr.check()
    tr.close()


# ---------------------------------------------------------------- 7. two ranks sharing the GPU over IPC
def _ipc_worker(rank, world, steps, clip):
    from tensorflow_distributed_amd.parallel.ipc import make_ipc_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = make_ipc_comm(rank, world, 0, M.TOTAL)
    eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 5, rank)
    eng.set_adam(LR, 0.9, 0.999, 1e-8)
    eng.set_ipc(comm, 1 << 30, True)
    eng.set_clip_norm(clip)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(steps, world * B, 784, generator=g)
    y = torch.randint(0, 10, (steps, world * B), generator=g, dtype=torch.int32)
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.params().copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()}).to(dev))
        eng.sync_shadow()
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
    out = eng.params().cpu(), eng.grad_norm().cpu(), int(eng.step_tensor().item()), comm.error(), eng.world()
    comm.close()
    return out


@pytest.mark.timeout(300)
def test_two_ranks_over_ipc_clip_identically(cuda):
    """Both ranks take the norm of the same all-reduced gradient: identical factors, identical replicas.
    run_ranks waits for each child under a timeout, raises at the first failure and ends the others."""
    res = run_ranks(_ipc_worker, 2, 4, 0.5, timeout=120)
    for p, pair, st, err, w in res:
        assert err == 0 and w == 2 and st == 4
        assert torch.isfinite(p).all()
        assert torch.equal(p, res[0][0]), "replicas diverged"
        assert pair.numpy().tobytes() == res[0][1].numpy().tobytes()
    norm, scale = res[0][1].tolist()
    assert norm > 0.5 and scale == float(np.float32(0.5) / np.float32(norm))


# ---------------------------------------------------------------- 8. the default is untouched
# capture_topology(1) of the default one-GPU bf16 Adam step at B = 32, recorded on the parent commit
PARENT_TOPOLOGY = ['node 0 0', 'node 1 0', 'node 2 0', 'node 3 0', 'node 4 0', 'node 5 0',
                   'edge 0 1', 'edge 1 2', 'edge 2 3', 'edge 3 4', 'edge 4 5',
                   'tag conv_fwd@0 0', 'tag fc_fwd@0 1 2', 'tag fc_bwd@0 3', 'tag conv_bwd@0 4', 'tag opt@0 5']


def test_default_step_is_what_it_was(cuda):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        never = _engine(cuda, ds)
        off = _engine(cuda, ds)
        off.set_clip_norm(0)
        topo = []
        for e in (never, off):
            assert e.clip_norm() == 0
            e.capture_train_steps("g", 4)
            e.replay("g", 1)
            topo.append(list(e.capture_topology(1)))
    torch.cuda.synchronize()
    assert int(never.step_tensor().item()) == 4
    _same(_state(never), _state(off))
    assert _pair(never).tolist() == _pair(off).tolist() == [0.0, 1.0]
    print("default topology:", topo[0])
    assert topo[0] == topo[1]
    assert topo[0] == PARENT_TOPOLOGY
