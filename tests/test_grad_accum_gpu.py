"""Gradient accumulation on the device (csrc/kernels/grad_accum.hip, MnistEngine.set_grad_accum): the
streaming kernel exactly, the accumulated gradient as the sequential fp32 sum of the micro-batch
gradients, the update as the flat optimizer on that sum at scale 1/K, captured graphs against eager
steps, composition with clipping / EMA / LAMB / LARS, the forced data-parallel schedule at world 1, the
sharded schedules' refusal, two ranks over IPC, one big batch to rounding, and the default step, which
must be what it was.

Engines run at batch 32 on a synthetic 256-row dataset (the conventions of tests/test_clip_norm_gpu.py);
bit-for-bit comparisons throughout: the kernel uses no atomics and adds in micro-batch order.
"""
import numpy as np
import pytest
import torch

from tensorflow_distributed_amd.models import mnist_cnn as M
from tensorflow_distributed_amd.training import optimizers as O
from tensorflow_distributed_amd.training.optimizers import schedule_args

import grad_accum_util as U
from dist_util import run_ranks

pytestmark = pytest.mark.gpu

B, ROWS = 32, 256
LR, MOM = 1e-2, 0.9
SCHED = O.PiecewiseConstant([2, 5], [1e-2, 1e-3, 1e-4])  # boundaries at 2 and 5 optimizer steps
# tests/test_clip_norm_gpu.py: worst relative error of the device norm against the fp64 norm of the same
# buffer, measured on an MI355X: 2.780e-08 (profiles/clip_norm_err.txt); the bound is 4x that. The norm
# kernel and the length (M.TOTAL) are unchanged here, so the bound is too.
REL_BOUND = 4 * 2.780e-08
# Worst e_acc / e_one over the eight parameter tensors and both dtypes, measured on an MI355X by
# tools/grad_accum_rel.py: profiles/grad_accum_err.txt. The bound is 3x that (the project's convention).
MEASURED_RATIO = 1.0003
R = 3 * MEASURED_RATIO
LW = dict(lr=2.0 ** -7, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, mu=0.9, eeta=1e-3)


# ---------------------------------------------------------------- helpers
def _dataset(cuda, rows=ROWS, seed=3):
    g = torch.Generator(device=cuda).manual_seed(seed)
    data = torch.rand(rows, 784, device=cuda, generator=g)
    labels = torch.randint(0, 10, (rows,), dtype=torch.int32, device=cuda, generator=g)
    perm = torch.randperm(rows, device=cuda, generator=g).to(torch.int32)
    return data, labels, perm


def _engine(cuda, ds, dtype="bf16", opt="adam", K=None, clip=None, ema=None, keep=0.75):
    e = torch.classes.tfd.MnistEngine(B, 0, keep, 1234, 0)
    e.set_dtype(dtype)
    if opt == "momentum":
        e.set_momentum(LR, MOM, False)
    elif opt == "lamb":
        e.set_lamb(LW["lr"], LW["b1"], LW["b2"], LW["eps"], LW["wd"], True)
    elif opt == "lars":
        e.set_lars(LW["lr"], LW["mu"], LW["wd"], LW["eeta"], 0.0, True)
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
        e.set_ema(ema, True)
    if K is not None:
        e.set_grad_accum(K)
    return e


def _state(e, ema=False):
    s = {"params": e.params().clone(), "adam_m": e.adam_m().clone(), "adam_v": e.adam_v().clone(),
         "params_bf16": e.params_bf16().clone(), "step": e.step_tensor().clone()}
    if ema:
        s["ema"] = e.ema_params().clone()
    return s


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())


_MICRO = {}


def _micro(cuda, dtype, steps):
    """Gradients of a plain engine (K = 1, same seed, rank and dataset) with its step set to each of
    `steps` in turn, by forward / backward_a / backward_b: computed once per (dtype, step), shared."""
    need = [s for s in steps if (dtype, s) not in _MICRO]
    if need:
        with torch.cuda.stream(torch.cuda.Stream()):
            e = _engine(cuda, _dataset(cuda), dtype)
            for s in need:
                e.step_tensor().fill_(s)
                e.forward(True)
                e.backward_a()
                e.backward_b()
                _MICRO[(dtype, s)] = e.grads().clone()
        torch.cuda.synchronize()
    return [_MICRO[(dtype, s)] for s in steps]


def _seq_sum(gs):
    acc = gs[0]
    for g in gs[1:]:
        acc = acc + g  # torch fp32, in micro-batch order
    return acc


# ---------------------------------------------------------------- 1. the kernel, exactly
N_PARAMS = 3274634
LENGTHS = [1, 3, 4, 5, 255, 1025, 262147, N_PARAMS, M.TOTAL]
NAN = float("nan")


def _buf(cuda, n, phase, dt, fill):
    """(whole, view): n elements starting at element `phase` >= 1 of an allocation, one sentinel element
    before (whole[phase - 1]) and one after (whole[-1])."""
    whole = torch.full((phase + n + 1,), fill, dtype=dt, device=cuda)
    return whole, whole[phase:phase + n]


@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_three_modes_every_alignment(cuda, n):
    ops = torch.ops.tfd
    gen = torch.Generator(device=cuda).manual_seed(n % 1000)
    # element phases of (acc, g, out) inside their allocations: all aligned; each alone off by one element
    # (no common phase: everything goes one by one); all off by one and by two (a scalar head, then the
    # 16-byte body)
    phases = [(4, 0, 4), (1, 0, 4), (4, 1, 4), (4, 0, 1), (1, 1, 1), (2, 2, 2)]
    if n > 300000:  # the large lengths: the aligned body, the shifted body and the all-scalar path once each
        phases = [(4, 0, 4), (1, 1, 1), (4, 1, 4)]
    for gdt in (torch.float32, torch.bfloat16):
        gsrc = torch.randn(n + 4, device=cuda, generator=gen).to(gdt)
        asrc = torch.randn(n, device=cuda, generator=gen)
        for pa, pg, po in phases:
            g = gsrc[pg:pg + n]
            # store over NaNs: no zero-fill is relied on
            aw, acc = _buf(cuda, n, pa, torch.float32, NAN)
            aw[pa - 1] = aw[-1] = 7.0

            def acc_sentinels():
                return aw[pa - 1] == 7.0 and aw[-1] == 7.0

            ops.grad_accum_flat(acc, g, None, True)
            assert torch.equal(acc, g.float()), (n, gdt, "store", (pa, pg, po))
            assert not torch.isnan(acc).any() and acc_sentinels()
            # add
            acc.copy_(asrc)
            want = asrc + g.float()
            ops.grad_accum_flat(acc, g)
            assert torch.equal(acc, want), (n, gdt, "add", (pa, pg, po))
            assert acc_sentinels()
            # emit, fp32 and bf16 out; acc untouched; two runs bit-identical
            acc.copy_(asrc)
            for odt in (torch.float32, torch.bfloat16):
                ow, out = _buf(cuda, n, po, odt, 5.0)
                ops.grad_accum_flat(acc, g, out)
                assert torch.equal(out, want.to(odt)), (n, gdt, odt, "emit", (pa, pg, po))
                assert ow[po - 1] == 5.0 and ow[-1] == 5.0, (n, "emit sentinel")
                assert torch.equal(acc, asrc) and acc_sentinels(), "emit wrote acc"
                _, again = _buf(cuda, n, po, odt, 5.0)
                ops.grad_accum_flat(acc, g, again)
                assert torch.equal(out, again)


def test_kernel_aligned_allocations_in_place_and_misuse(cuda):
    ops = torch.ops.tfd
    n = M.TOTAL
    gen = torch.Generator(device=cuda).manual_seed(5)
    g0, g1, g2 = (torch.randn(n, device=cuda, generator=gen) for _ in range(3))
    acc = torch.full((n,), NAN, device=cuda)
    ops.grad_accum_flat(acc, g0, None, True)
    ops.grad_accum_flat(acc, g1)
    want = (g0 + g1) + g2
    out = g2.clone()
    ops.grad_accum_flat(acc, out, out)  # the engine's emit: out is g itself
    assert torch.equal(out, want)
    obf = torch.empty(n, dtype=torch.bfloat16, device=cuda)
    ops.grad_accum_flat(acc, g2, obf)
    assert torch.equal(obf, want.to(torch.bfloat16))
    for blocks, loads in ((1, 1), (7, 4), (2048, 2), (4096, 1)):  # the probe's knobs change no bit
        o2 = torch.empty_like(out)
        ops.grad_accum_tuned(acc, g2, o2, False, blocks, loads)
        assert torch.equal(o2, want), (blocks, loads)
    a4, g4 = torch.zeros(4, device=cuda), torch.zeros(4, device=cuda)
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(a4, torch.zeros(5, device=cuda))  # lengths
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(a4, g4, torch.zeros(3, device=cuda))
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(a4, g4, torch.zeros(4, device=cuda), True)  # first together with out
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(a4.to(torch.bfloat16), g4)  # acc is fp32
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(a4, g4.double())
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(a4, g4, torch.zeros(4, device=cuda, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        ops.grad_accum_flat(torch.zeros(0, device=cuda), torch.zeros(0, device=cuda))  # empty


# ---------------------------------------------------------------- 2. the accumulated gradient is the sequential fp32 sum
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_accumulated_gradient_is_the_sequential_fp32_sum(cuda, dtype):
    """Pins the data rows and the dropout mask of every micro-batch too: micro-batch m of the accumulating
    engine is step m of a plain one. From global_step 1 the six micro-batches so far (192 rows) and the
    next three wrap the 256-row permutation."""
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, ds, dtype, K=3)
        assert e.grad_accum() == 3
        e.train_step()
        g_a = e.grads().clone()
        e.train_step()
        g_b = e.grads().clone()
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 2 and int(e.micro_step_tensor().item()) == 6
    # the second step's micro-batches see the parameters the first step updated: compare it from a
    # fresh engine placed at global_step 1 instead
    assert torch.equal(g_a, _seq_sum(_micro(cuda, dtype, [0, 1, 2])))
    with torch.cuda.stream(torch.cuda.Stream()):
        f = _engine(cuda, ds, dtype, K=3)
        f.step_tensor().fill_(1)
        f.sync_micro_step()
        f.train_step()
    torch.cuda.synchronize()
    assert int(f.step_tensor().item()) == 2 and int(f.micro_step_tensor().item()) == 6
    want = _seq_sum(_micro(cuda, dtype, [3, 4, 5]))
    assert torch.equal(f.grads(), want)
    assert not torch.equal(f.grads(), g_a) and not torch.equal(g_b, g_a)
    assert 3 * B * 2 + 3 * B > ROWS  # the wrap


# ---------------------------------------------------------------- 3. the update is the flat optimizer on that sum at 1/K
def _flat(e, opt, before, grads, grad_scale, sched=None):
    ops = torch.ops.tfd
    p, m, v, pbf = (before[k].clone() for k in ("params", "adam_m", "adam_v", "params_bf16"))
    kind, params, bnd, vals = schedule_args(sched) if sched is not None else ("constant", [], [], [])
    if opt == "adam":  # t = the engine's bumped step: t_offset 0
        ops.adam_flat(p, m, v, grads, pbf, LR, 0.9, 0.999, 1e-8, e.step_tensor(), grad_scale, 0, kind, params, bnd, vals)
    else:
        ops.momentum_flat(p, m, grads, pbf, LR, MOM, 0.0, False, grad_scale, None, 0, kind, params, bnd, vals)
    torch.cuda.synchronize()
    return {"params": p, "adam_m": m, "adam_v": v, "params_bf16": pbf, "step": e.step_tensor().clone()}


@pytest.mark.parametrize("opt", ["adam", "momentum"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_update_is_the_flat_optimizer_on_the_sum_at_one_over_k(cuda, dtype, opt):
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), dtype, opt, K=3)
        before = _state(e)
        e.train_step()
    torch.cuda.synchronize()
    after = _state(e)
    assert int(e.step_tensor().item()) == 1 and int(e.micro_step_tensor().item()) == 3
    _same(_flat(e, opt, before, e.grads(), 1.0 / 3), after)
    unscaled = _flat(e, opt, before, e.grads(), 1.0)
    assert not torch.equal(unscaled["params"], after["params"])


# ---------------------------------------------------------------- 4. graph equals eager
def _graph_vs_eager(make, ema=False):
    eager, graph = make(), make()
    for _ in range(4):
        eager.train_step()
    graph.capture_train_steps("g", 2)
    graph.replay("g", 2)
    torch.cuda.synchronize()
    assert int(graph.step_tensor().item()) == int(eager.step_tensor().item()) == 4
    assert int(graph.micro_step_tensor().item()) == int(eager.micro_step_tensor().item()) == 4 * eager.grad_accum()
    _same(_state(graph, ema), _state(eager, ema))
    assert torch.equal(graph.grads(), eager.grads())
    return eager, graph


@pytest.mark.parametrize("opt", ["adam", "momentum", "adam_piecewise"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graph_equals_eager(cuda, dtype, opt):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        eager, _ = _graph_vs_eager(lambda: _engine(cuda, ds, dtype, opt, K=3))
    assert int(eager.micro_step_tensor().item()) == 12
    if opt != "adam_piecewise":
        return
    # the boundaries are crossed by global_step, not by the micro counter: the update from global_step 3
    # (micro-batches 9..11) takes the rate of step 3, the second value -- the micro counter would be past
    # the boundary at 5 and take the third
    plain = _engine(cuda, ds, dtype, opt)
    assert plain.lr_at_step(3) == eager.lr_at_step(3) == pytest.approx(1e-3)
    assert plain.lr_at_step(9) == pytest.approx(1e-4)
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, ds, dtype, opt, K=3)
        for _ in range(3):
            e.train_step()
        before = _state(e)
        e.train_step()
    torch.cuda.synchronize()
    after = _state(e)
    _same({"params": after["params"]}, {"params": eager.params()})
    got = _flat(e, "adam", before, e.grads(), 1.0 / 3, SCHED)
    assert torch.equal(got["params"], after["params"]) and torch.equal(got["adam_m"], after["adam_m"])
    # ... which a constant rate (the first value) does not reproduce
    assert not torch.equal(_flat(e, "adam", before, e.grads(), 1.0 / 3)["params"], after["params"])


# ---------------------------------------------------------------- 5. composition
_NORM0 = {}


def _norm0(cuda, dtype, K=3):
    """fp64 norm of the step-0 summed gradient at scale 1/K (from the shared micro-batch gradients)."""
    if dtype not in _NORM0:
        g = _seq_sum(_micro(cuda, dtype, list(range(K))))
        _NORM0[dtype] = float((g.double() / K).norm().item())
    return _NORM0[dtype]


@pytest.mark.parametrize("what", ["clip", "ema", "lamb", "lars"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_composition_graph_equals_eager(cuda, dtype, what):
    ops = torch.ops.tfd
    ds = _dataset(cuda)
    K = 3
    kw = {"clip": dict(clip=0.05 * _norm0(cuda, dtype)), "ema": dict(ema=0.99), "lamb": dict(opt="lamb"),
          "lars": dict(opt="lars")}[what]
    with torch.cuda.stream(torch.cuda.Stream()):
        eager, graph = _graph_vs_eager(lambda: _engine(cuda, ds, dtype, K=K, **kw), ema=what == "ema")
        one = _engine(cuda, ds, dtype, K=K, **kw)
        before = _state(one)
        one.train_step()
    torch.cuda.synchronize()
    if what == "clip":
        assert eager.grad_norm().cpu().numpy().tobytes() == graph.grad_norm().cpu().numpy().tobytes()
        norm, scale = one.grad_norm().cpu().numpy()
        ref = float((one.grads().double() / K).norm().item())
        rel = abs(float(norm) - ref) / ref
        print(f"grad_accum clip {dtype}: device norm {norm!r} fp64 {ref!r} rel {rel:.3e} (bound {REL_BOUND:.3e})")
        assert rel <= REL_BOUND
        assert scale < 1 and scale == np.float32(kw["clip"]) / norm  # fp32 division, bit for bit
        assert float(eager.grad_norm()[1].item()) < 1  # still clipping at step 4
    elif what == "ema":
        plain = _engine(cuda, ds, dtype, K=K)
        with torch.cuda.stream(torch.cuda.Stream()):
            for _ in range(4):
                plain.train_step()
        torch.cuda.synchronize()
        assert torch.equal(plain.params(), eager.params())  # the update is the same with the shadow on
        assert not torch.equal(eager.ema_params(), eager.params())
        # d_t follows global_step: four updates, not twelve
        e = one.ema_params().double()
        want = before["params"].double() - (1 - one.ema_decay_at_step(1)) * (before["params"].double() - one.params().double())
        assert float((e - want).abs().max()) <= 1e-6 * float(want.abs().max())
    else:
        # the norms and ratios are those of the summed gradient: the flat layer-wise op on the state before
        # the step with grads() at scale 1/K reproduces the table and the parameters
        segs = torch.tensor(M.segments(True), dtype=torch.int64).reshape(-1, 3)
        p, m, v, pbf = (before[k].clone() for k in ("params", "adam_m", "adam_v", "params_bf16"))
        if what == "lamb":
            tab = ops.lamb_flat(p, m, v, one.grads(), pbf, segs, LW["lr"], LW["b1"], LW["b2"], LW["eps"], LW["wd"],
                                one.step_tensor(), 0, 1.0 / K)
        else:
            tab = ops.lars_flat(p, m, one.grads(), pbf, segs, LW["lr"], LW["mu"], LW["wd"], LW["eeta"], 0.0,
                                one.step_tensor(), 0, 1.0 / K)
        torch.cuda.synchronize()
        assert torch.equal(tab.reshape(-1), one.layer_norms().reshape(-1))
        assert torch.equal(p, one.params()) and torch.equal(m, one.adam_m())
        if what == "lars":  # column 1 is |g| of the gradient the optimizer consumed: the sum at 1/K
            gn = ops.layer_norms(one.grads() * np.float32(1.0 / K), segs)
            got = one.layer_norms()[:, 1]
            assert float(((got - gn).abs() / gn).max()) <= 1e-6, (got, gn)


# ---------------------------------------------------------------- 6. forced DP at world 1
@pytest.mark.parametrize("mode,wire,dtype", [("rccl", "bf16", "bf16"), ("rccl", "fp32", "bf16"), ("ipc", "bf16", "bf16"),
                                             ("ipc", "fp32", "bf16"), ("rccl", "fp32", "fp32"), ("ipc", "fp32", "fp32")])
def test_forced_dp_world1(cuda, mode, wire, dtype):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    ds = _dataset(cuda)
    K = 2
    trs = []

    def make():
        e = _engine(cuda, ds, dtype, "adam", K=K)
        trs.append(attach_engine(e, 0, 1, cuda, mode=mode, force_dp=True, bf16=wire == "bf16"))
        assert e.dp()
        return e

    with torch.cuda.stream(torch.cuda.Stream()):
        _graph_vs_eager(make)
        one = make()
        before = _state(one)
        one.train_step()
        topo = list(one.capture_topology(1))
    torch.cuda.synchronize()
    for tr in trs:
        tr.check()
    tags = [ln.split()[1].split("@")[0] for ln in topo if ln.startswith("tag ")]
    colls = [i for i, t in enumerate(tags) if t.startswith("ar")]
    accs = [i for i, t in enumerate(tags) if t == "accum"]
    assert len(accs) == K, tags
    assert sorted(tags[i] for i in colls) == (["ar"] if dtype == "fp32" else ["ar_conv", "ar_fc"]), tags
    assert min(colls) > max(accs), tags  # micro-batches launch no collective
    want = _seq_sum(_micro(cuda, dtype, [0, 1]))
    after = _state(one)
    if wire == "bf16":
        # the emit rounded the fp32 sum to bf16 once; at world 1 the reduced buffer equals it, and the
        # optimizer read that buffer and not grads() (which holds the last micro-batch's gradient)
        assert torch.equal(one.grads_bf16(), want.to(torch.bfloat16))
        _same(_flat(one, "adam", before, one.grads_bf16(), 1.0 / K), after)
        assert not torch.equal(_flat(one, "adam", before, one.grads(), 1.0 / K)["params"], after["params"])
    else:
        assert torch.equal(one.grads(), want)
        _same(_flat(one, "adam", before, one.grads(), 1.0 / K), after)
    for tr in trs:
        tr.close()


# ---------------------------------------------------------------- 7. sharded schedules raise before launching
@pytest.mark.parametrize("which", ["sfb", "zero"])
def test_sharded_schedule_raises_before_launching(cuda, which):
    from tensorflow_distributed_amd.parallel.transport import attach_engine

    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), "bf16", "adam", K=2)
        tr = attach_engine(e, 0, 1, cuda, mode="ipc", force_dp=True, sfb=which == "sfb", zero=which == "zero")
        if which == "zero":
            e.set_zero(True)
        else:
            assert e.fc_sfb()
        before = _state(e)
        with pytest.raises(RuntimeError, match="set_grad_accum conflicts with"):
            e.train_step()
        torch.cuda.synchronize()
        _same(_state(e), before)
        assert int(e.step_tensor().item()) == 0 and int(e.micro_step_tensor().item()) == 0
        e.set_grad_accum(1)  # off again: the sharded schedule steps
        e.train_step()
    torch.cuda.synchronize()
    assert int(e.step_tensor().item()) == 1
    tr.check()
    tr.close()


def test_capture_grads_raises_while_accumulating(cuda):
    with torch.cuda.stream(torch.cuda.Stream()):
        e = _engine(cuda, _dataset(cuda), "bf16", "adam", K=2)
        with pytest.raises(RuntimeError, match="set_grad_accum"):
            e.capture_grads("grads")
        with pytest.raises(RuntimeError):
            e.set_grad_accum(0)
        e.set_grad_accum(1)
        e.forward(True)
        e.backward_a()
        e.backward_b()
        e.capture_grads("grads")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 8. two ranks sharing the GPU over IPC
def _ipc_worker(rank, world, steps, K):
    from tensorflow_distributed_amd.parallel.ipc import make_ipc_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    comm = make_ipc_comm(rank, world, 0, M.TOTAL)
    eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 5, rank)
    eng.set_adam(LR, 0.9, 0.999, 1e-8)
    eng.set_ipc(comm, 1 << 30, True)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(steps, world, 2 * B, 784, generator=g)  # the same draws whatever K is
    y = torch.randint(0, 10, (steps, world, 2 * B), generator=g, dtype=torch.int32)
    with torch.cuda.stream(torch.cuda.Stream()):
        eng.set_grad_accum(K)
        eng.params().copy_(M.flat_from_dict({k: v * 0.05 for k, v in M.init_params(3).items()}).to(dev))
        eng.sync_shadow()
        assert tuple(eng.feed_x().shape) == (K * B, 784)
        for i in range(steps):
            eng.feed_x().copy_(x[i, rank, :K * B].to(dev))
            eng.feed_y().copy_(y[i, rank, :K * B].to(dev))
            if i == 0:
                eng.train_step()
                eng.capture_train_step("t")
            else:
                eng.replay("t", 1)
            torch.cuda.current_stream().synchronize()
    torch.cuda.synchronize()
    out = (eng.params().cpu(), int(eng.step_tensor().item()), int(eng.micro_step_tensor().item()), comm.error(),
           eng.world())
    comm.close()
    return out


@pytest.mark.timeout(300)
def test_two_ranks_over_ipc_accumulate_identically(cuda):
    """Fed batches of K * B rows per rank, one all-reduce per step: identical replicas. run_ranks waits
    for each child under a timeout, raises at the first failure and ends the others."""
    res = run_ranks(_ipc_worker, 2, 4, 2, timeout=120)
    for p, st, mi, err, w in res:
        assert err == 0 and w == 2 and st == 4 and mi == 8
        assert torch.isfinite(p).all()
        assert torch.equal(p, res[0][0]), "replicas diverged"
    one = run_ranks(_ipc_worker, 2, 4, 1, timeout=120)
    assert one[0][1] == 4 and one[0][3] == 0
    assert not torch.equal(one[0][0], res[0][0])  # the second B rows of every step were felt


# ---------------------------------------------------------------- 9. equal to one big batch, to rounding
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_equal_to_one_big_batch_to_rounding(cuda, dtype):
    """K = 4 micro-batches of 32 against a plain engine at batch 128 on the same 128 rows, keep_prob 1.0:
    per parameter tensor the rel-L2 error of grads() / 4 against the fp64 oracle at batch 128 is at most
    R times the plain engine's own (the parent's path, measured here). With K a power of two the two
    differ only in the grouping of fp32 sums."""
    e_acc, e_one, summed = U.accum_vs_one(cuda, dtype)
    for k in e_acc:
        print(f"grad_accum vs one batch {dtype} {k}: e_acc {e_acc[k]:.3e} e_one {e_one[k]:.3e} "
              f"ratio {e_acc[k] / e_one[k]:.3f} (bound {R:.3f})")
    for k in e_acc:
        assert e_acc[k] <= R * e_one[k], (k, e_acc[k], e_one[k])
    # the sum is the micro-batch gradients' own
    micro = U.micro_grads(cuda, dtype)
    assert torch.equal(summed, _seq_sum(micro))
    # mutation: one micro-batch's contribution scaled by 1.05 must fail the bound
    bad = _seq_sum([micro[0], micro[1] * 1.05, micro[2], micro[3]])
    e_bad = U.rel_l2(bad / U.K, U.oracle_grads(dtype))
    assert any(e_bad[k] > R * e_one[k] for k in e_bad), (e_bad, e_one)


# ---------------------------------------------------------------- 10. the default is untouched
# capture_topology(1) of the default one-GPU bf16 Adam step at B = 32, recorded on the parent commit
# (the list of tests/test_clip_norm_gpu.py)
PARENT_TOPOLOGY = ['node 0 0', 'node 1 0', 'node 2 0', 'node 3 0', 'node 4 0', 'node 5 0',
                   'edge 0 1', 'edge 1 2', 'edge 2 3', 'edge 3 4', 'edge 4 5',
                   'tag conv_fwd@0 0', 'tag fc_fwd@0 1 2', 'tag fc_bwd@0 3', 'tag conv_bwd@0 4', 'tag opt@0 5']


def test_default_step_is_what_it_was(cuda):
    ds = _dataset(cuda)
    with torch.cuda.stream(torch.cuda.Stream()):
        never = _engine(cuda, ds)
        off = _engine(cuda, ds, K=1)
        topo = []
        for e in (never, off):
            assert e.grad_accum() == 1
            assert tuple(e.feed_x().shape) == (B, 784) and tuple(e.feed_y().shape) == (B,)
            e.capture_train_steps("g", 4)
            e.replay("g", 1)
            topo.append(list(e.capture_topology(1)))
    torch.cuda.synchronize()
    assert int(never.step_tensor().item()) == 4 and int(off.micro_step_tensor().item()) == 4
    _same(_state(never), _state(off))
    assert topo[0] == topo[1]
    assert topo[0] == PARENT_TOPOLOGY
