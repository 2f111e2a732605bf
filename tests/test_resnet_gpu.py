"""ResNet on the native kernel library: forward/backward against a pure-PyTorch fp32 reference
with the same weights (bf16-rounded), and a few SGD steps reduce the loss."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


class _RB(torch.autograd.Function):
    """Round to bf16 in forward AND backward: where the native kernels store bf16 tensors."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


@pytest.fixture
def row_mode():
    """BN statistics in row mode (fixed-order partial rows + bn_final): every sum of the step in a
    fixed order, so the bit-exact comparisons below can see a race or a misplaced gradient."""
    old = torch.ops.tfd.set_bn_part_slots(0)
    yield
    torch.ops.tfd.set_bn_part_slots(old)


def _same_run(loss0, loss1, g0, g1):
    """Two forward + backward passes that must agree: bit for bit in row mode (every sum in a fixed
    order; only split-K weight-gradient atomics may reorder fp32 adds, hence the tiny tolerance); in
    slot mode (bn_part_slots() > 0) the BN statistics are atomic fp32 sums too, and a changed last bit
    of a mean can flip bf16 roundings downstream -- a relative-norm bound instead."""
    if torch.ops.tfd.bn_part_slots() == 0:
        assert loss0 == loss1
        torch.testing.assert_close(g1, g0, rtol=1e-5, atol=1e-6)
    else:
        assert abs(loss0 - loss1) <= 1e-5 * abs(loss0)
        assert ((g1 - g0).norm() / g0.norm()).item() < 1e-2


def _ref_forward(model, x, labels):
    """Pure PyTorch fp32 ResNet with the model's weights (NCHW), training-mode BN."""
    fp = model.fp
    P = {}

    def W(name):  # HWIO bf16 -> OIHW fp32 leaf
        if name not in P:
            P[name] = fp.w(name).float().cpu().permute(3, 2, 0, 1).contiguous().requires_grad_(True)
        return P[name]

    def V(name):
        if name not in P:
            P[name] = fp.p(name).float().cpu().clone().requires_grad_(True)
        return P[name]

    def conv(x, L):
        return _RB.apply(F.conv2d(x, W(L.name), stride=L.stride, padding=L.pad))

    def bn(y, L, relu=True, res=None):
        z = F.batch_norm(y, None, None, V(L.name + "/gamma"), V(L.name + "/beta"), training=True, eps=1e-5)
        if res is not None:
            z = z + res
        return _RB.apply(torch.relu(z) if relu else z)

    h = F.pad(x.permute(0, 3, 1, 2), (0, 0, 0, 0, 0, 5))  # 3 -> 8 channels
    h = bn(conv(h, model.stem), model.stem_bn)
    h = F.max_pool2d(h, 3, 2, 1)
    for blk in model.blocks:
        sc = h
        if "cd" in blk:
            sc = bn(conv(h, blk["cd"]), blk["bd"], relu=False)
        if model.kind == "basic":
            t = bn(conv(h, blk["c1"]), blk["b1"])
            h = bn(conv(t, blk["c2"]), blk["b2"], True, sc)
        else:
            t = bn(conv(h, blk["c1"]), blk["b1"])
            t = bn(conv(t, blk["c2"]), blk["b2"])
            h = bn(conv(t, blk["c3"]), blk["b3"], True, sc)
    h = _RB.apply(h.mean((2, 3)))
    wfc = fp.w("fc").float().cpu().requires_grad_(True)
    P["fc"] = wfc
    logits = h @ wfc + V("fc/bias")
    return F.cross_entropy(logits, labels.long()), P


# End to end the bf16 roundings of every layer compound through train-mode BN: row-mode relative L2 of
# the fc gradients (profiles/resnet_oracle_rel_r5.txt) at depth 18 (4 x 64^2 images): weight 0.83 %,
# bias 0.23 %; at depth 50 (8 x 128^2): weight 3.6 %, bias 0.39 % (4 x 64^2 images: 9.7 %, bias 1.7 %,
# hence the larger input). Bounds per depth: (input batch, image, weight bound, bias bound).
E2E_CASE = {18: (4, 64, 2e-2, 1e-2), 50: (8, 128, 6e-2, 1.5e-2)}


@pytest.mark.parametrize("depth", [18, 50])
def test_resnet_end_to_end_loss_and_head(cuda, row_mode, depth):
    """Whole network: loss and the fc gradient agree with the fp32 reference. (Deep gradients are
    checked block by block below: end to end, train-mode BN over tiny M amplifies bf16 rounding --
    a one-ulp change of a batch statistic moves this loss by up to ~2 %
    (tools/debug/bn_slot_race.py), so the statistics are summed in row mode's fixed order here;
    slot mode's atomic order is covered by test_bn_slot_mode_matches_row_mode.)"""
    from tensorflow_distributed_amd.models.resnet import ResNet

    nb, hw, wb, bb = E2E_CASE[depth]
    torch.manual_seed(0)
    m = ResNet(depth, num_classes=16, device=cuda, seed=1, width=16, zero_init_residual=False)
    x = torch.randn(nb, hw, hw, 3)
    lab = torch.randint(0, 16, (nb,), dtype=torch.int32)
    loss, _ = m.loss(x.to(cuda), lab.to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    lref, P = _ref_forward(m, x.to(torch.bfloat16).float(), lab)
    lref.backward()
    assert abs(loss.item() - lref.item()) / lref.item() < 3e-2, (loss.item(), lref.item())
    gfc, rfc = m.fp.g("fc").float().cpu(), P["fc"].grad
    gb, rb = m.fp.g("fc/bias").float().cpu(), P["fc/bias"].grad
    cos = torch.nn.functional.cosine_similarity(gfc.flatten(), rfc.flatten(), dim=0).item()
    assert cos > 0.99, cos
    # magnitude too: relative L2 of the fc weight and bias gradients (row mode); where the bound is
    # below 3 %, a 5 % scale error must fail it (the deep weight gradient's bound leaves no room: the
    # per-block test pins every weight gradient's scale tightly)
    for a, b, bound in ((gfc, rfc, wb), (gb, rb, bb)):
        assert rel_l2(a, b) <= bound, (rel_l2(a, b), bound)
        if bound < 3e-2:
            assert rel_l2(1.05 * a, b) > bound


def rel_l2(a, b) -> float:
    """||a - b|| / ||b|| in fp64 (magnitude-sensitive: a wrong scale shows, unlike a cosine)."""
    a, b = a.flatten().double(), b.flatten().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def block_case(cuda, depth, bi, hw):
    """One residual block from identical inputs through the native kernels and through the fp32
    PyTorch reference: {name: (native, reference)} for the output, dX and every weight / BN gradient
    (CPU fp32, NCHW / HWIO matched)."""
    from tensorflow_distributed_amd.models.resnet import ResNet

    torch.manual_seed(bi)
    m = ResNet(depth, num_classes=16, device=cuda, seed=1, width=16, zero_init_residual=False)
    blk = m.blocks[bi]
    cin = m.fp.by_name[blk["c1"].name].shape[2]
    x = torch.randn(4, hw, hw, cin).to(torch.bfloat16).float()
    xn = x.to(cuda, torch.bfloat16).requires_grad_(True)
    m.fp.grad.zero_()
    out = m.block_forward(blk, xn)
    g = torch.randn(out.shape).to(torch.bfloat16).float()
    out.backward(g.to(cuda, torch.bfloat16))
    torch.cuda.synchronize()
    Ws = {k: m.fp.w(L.name).float().cpu().permute(3, 2, 0, 1).clone().requires_grad_(True)
          for k, L in blk.items() if k.startswith("c")}
    Gs = {k: [m.fp.p(L.name + s).cpu().clone().requires_grad_(True) for s in ("/gamma", "/beta")]
          for k, L in blk.items() if k.startswith("b")}

    def conv(h, k):
        return _RB.apply(F.conv2d(h, Ws[k], stride=blk[k].stride, padding=blk[k].pad))

    def bn(y, k, relu=True, res=None):
        z = F.batch_norm(y, None, None, Gs[k][0], Gs[k][1], training=True, eps=1e-5)
        z = z + res if res is not None else z
        return _RB.apply(torch.relu(z) if relu else z)

    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    scr = bn(conv(xr, "cd"), "bd", relu=False) if "cd" in blk else xr
    if m.kind == "basic":
        outr = bn(conv(bn(conv(xr, "c1"), "b1"), "c2"), "b2", True, scr)
    else:
        outr = bn(conv(bn(conv(bn(conv(xr, "c1"), "b1"), "c2"), "b2"), "c3"), "b3", True, scr)
    outr.backward(g.permute(0, 3, 1, 2))
    pairs = {"out": (out.detach().float().cpu().permute(0, 3, 1, 2), outr.detach()),
             "dx": (xn.grad.float().cpu().permute(0, 3, 1, 2), xr.grad)}
    for k, L in blk.items():
        if k.startswith("c"):
            pairs[k] = (m.fp.g(L.name).float().cpu(), Ws[k].grad.permute(2, 3, 1, 0))
        else:
            pairs[k + "/gamma"] = (m.fp.g(L.name + "/gamma").float().cpu(), Gs[k][0].grad)
            pairs[k + "/beta"] = (m.fp.g(L.name + "/beta").float().cpu(), Gs[k][1].grad)
    return pairs


# Relative-L2 bounds per tensor kind, row mode (fixed-order BN sums); calibrated on the box over every
# case below (tools/debug/resnet_oracle_rel.py, profiles/resnet_oracle_rel_r5.txt; row-mode maxima:
# out 3e-5, dx 2.2e-3, conv dW 5.7e-4, dgamma 5.2e-4, dbeta 5.8e-4), ~5-10x headroom and far below
# the 5 % a wrong scale of any one tensor gives.
REL_BOUND = {"out": 1e-3, "dx": 1e-2, "conv": 5e-3, "gamma": 5e-3, "beta": 5e-3}


def _kind(name):
    if name in ("out", "dx"):
        return name
    return "gamma" if name.endswith("/gamma") else "beta" if name.endswith("/beta") else "conv"


@pytest.mark.parametrize("depth,bi,hw", [(50, 0, 16), (50, 1, 16), (50, 3, 16), (50, 13, 4), (18, 0, 16), (18, 2, 16)])
def test_resnet_block_forward_backward(cuda, row_mode, depth, bi, hw):
    """One residual block from identical inputs: output, dX and every weight/BN gradient within a
    per-tensor relative-L2 bound of the fp32 reference (magnitude-sensitive), cosine > 0.999 as an
    extra direction check, and the mutation check: any one tensor scaled by 1.05 must break its bound
    (a missing 1/M in dgamma or a doubled residual gradient cannot pass)."""
    pairs = block_case(cuda, depth, bi, hw)
    rels = {k: rel_l2(a, b) for k, (a, b) in pairs.items()}
    bad = {k: r for k, r in rels.items() if not r <= REL_BOUND[_kind(k)]}
    assert not bad, (bad, rels)
    coss = {k: F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item() for k, (a, b) in pairs.items()}
    assert all(c > 0.999 for c in coss.values()), coss
    for k, (a, b) in pairs.items():
        assert rel_l2(1.05 * a, b) > REL_BOUND[_kind(k)], (k, "a 5 % scale error would pass")


@pytest.mark.parametrize("depth", [18, 50])
def test_residual_join_fusion_matches_autograd_adds(cuda, row_mode, depth):
    """fuse_joins (the residual-join gradient sum formed in the dgrad epilogue, GradJoin) against
    autograd's separate adds: same loss, and every parameter gradient equal up to the one extra
    bf16 rounding the unfused sum takes."""
    from tensorflow_distributed_amd.models.resnet import ResNet

    torch.manual_seed(4)
    x = torch.randn(4, 64, 64, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    grads, losses = [], []
    for fuse in (False, True):
        m = ResNet(depth, num_classes=16, device=cuda, seed=1, width=16, zero_init_residual=False, fuse_joins=fuse)
        m.fp.grad.zero_()
        loss, _ = m.loss(x, lab)
        loss.backward()
        torch.cuda.synchronize()
        losses.append(loss.item())
        grads.append(m.fp.grad.cpu().clone())
    assert losses[0] == losses[1]
    cos = torch.nn.functional.cosine_similarity(grads[0], grads[1], dim=0).item()
    rel = ((grads[0] - grads[1]).norm() / grads[0].norm()).item()
    assert cos > 0.999 and rel < 3e-2, (cos, rel)


def test_resnet_training_reduces_loss(cuda):
    from tensorflow_distributed_amd.models.resnet import ResNet

    torch.manual_seed(0)
    m = ResNet(18, num_classes=16, device=cuda, seed=2, width=16)
    x = torch.randn(16, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (16,), dtype=torch.int32, device=cuda)
    losses = [m.train_step(x, lab, lr=0.05).item() for _ in range(15)]
    assert losses[-1] < 0.5 * losses[0], losses


def test_resnet_graph_capture(cuda):
    from tensorflow_distributed_amd.models.resnet import ResNet

    m = ResNet(18, num_classes=16, device=cuda, seed=3, width=16)
    x = torch.randn(8, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (8,), dtype=torch.int32, device=cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m.train_step(x, lab, lr=0.01)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.train_step(x, lab, lr=0.01)
    vals = []
    for _ in range(3):
        g.replay()
        vals.append(out.item())
    assert all(v == v for v in vals) and vals[-1] < vals[0] + 1.0


def _rccl_bucketed_worker(rank, world, bf16, small_ipc=False):
    import torch

    from tensorflow_distributed_amd import _native
    from tensorflow_distributed_amd.models.resnet import ResNet

    _native.require()
    cuda = torch.device("cuda", 0)
    torch.manual_seed(11)
    uid = torch.classes.tfd.RcclComm.unique_id()
    comm = torch.classes.tfd.RcclComm(uid, 1, 0, cuda.index)
    x = torch.randn(8, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (8,), dtype=torch.int32, device=cuda)
    small = None
    if small_ipc:  # buckets <= 24 KB over the IPC one-shot all-reduce, the rest over RCCL
        from tensorflow_distributed_amd.parallel.transport import small_bucket_ipc

        small = small_bucket_ipc(0, 1, cuda, comm, 24 << 10, force=True)
        assert small is not None
    ms = []
    for dp in (False, True):
        m = ResNet(18, num_classes=16, device=cuda, seed=5, width=16)
        if dp:
            m.set_comm(comm, bucket_mb=0.05, bf16_grads=bf16, force_dp=True, small=small, small_mb=24 / 1024)
            assert m.reducer.stream is not None and len(m.reducer.buckets) > 3
            if small_ipc:
                assert 0 < m.reducer.small_buckets < len(m.reducer.buckets), (m.reducer.small_buckets,
                                                                               len(m.reducer.buckets))
        elif bf16:  # the reference step reads its gradients rounded to bf16, as the wire delivers them
            fp = m.fp
            m.reducer.reduced_grads = lambda fp=fp: fp.grad.to(torch.bfloat16)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                m.train_step(x, lab, lr=0.01)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m.train_step(x, lab, lr=0.01)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        if dp:
            assert m.reducer.launched == len(m.reducer.buckets)
        ms.append(m)
    p0, p1 = ms[0].fp.master, ms[1].fp.master
    bad = (p0 != p1).nonzero().flatten()
    names = sorted({s.name for s in ms[0].fp.specs for i in bad[:64].tolist() if s.offset <= i < s.offset + s.numel})
    return int(bad.numel()), names[:8], bool(torch.isfinite(p1).all().item())


@pytest.mark.parametrize("bf16,small_ipc", [(False, False), (True, False), (True, True)])
def test_resnet_rccl_bucketed_world1_equals_no_comm(cuda, row_mode, bf16, small_ipc):
    """The ResNet DP path (BucketReducer: comm stream, per-bucket collectives launched from inside
    the backward, 1/N in the fused SGD) forced at world 1 over a REAL RcclComm, eager and captured
    in a CUDA graph: the world-1 sum is the identity, so the parameters equal the no-communicator
    step bit for bit -- with the bf16 wire, the one whose optimizer reads bf16-rounded gradients (a
    bucket cast before its last gradient landed would show up here).

    Runs in the suite's process again (round 3 moved it to a fresh one after an in-suite segfault in
    CUDAGraph.replay): RcclComm's destructor no longer destroys a communicator that an earlier
    test's still-alive captured graph used (see test_rccl_comm_outlives_its_python_object).
    small_ipc: the small buckets ride the IPC one-shot all-reduce beside RCCL (a world-1 IpcComm)."""
    import gc

    n_bad, names, finite = _rccl_bucketed_worker(0, 1, bf16, small_ipc)
    # the models' layers point back at them (reference cycles): collect them and their communicator
    # here, where nothing is capturing, not whenever the collector next runs (a communicator
    # destroyed inside a later capture invalidates that capture)
    gc.collect()
    assert finite
    assert n_bad == 0, f"{n_bad} parameters differ (first in {names})"


def test_rccl_comm_outlives_its_python_object(cuda):
    """A graph that captured collectives keeps its communicator alive after the Python RcclComm (and
    the model holding it) is gone -- every capture hands the graph a reference (a HIP user object) --
    and the communicator is destroyed once the graph goes too: in the suite's own process, graphs
    destroyed freely (the round-4 process-lifetime graph retention is gone, see
    test_capture_destroy_cycles_keep_the_heap_intact)."""
    import gc
    import time

    from tensorflow_distributed_amd.models.resnet import ResNet

    RC = torch.classes.tfd.RcclComm
    RC.reap()
    comm = RC(RC.unique_id(), 1, 0, cuda.index)
    assert comm.graph_refs() == 0
    m = ResNet(18, num_classes=16, device=cuda, seed=5, width=16)
    m.set_comm(comm, bucket_mb=0.05, bf16_grads=True, force_dp=True)
    x = torch.randn(4, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.train_step(x, lab, lr=0.01)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.train_step(x, lab, lr=0.01)
    assert comm.graph_refs() >= 1, "the captured graph holds no reference to its communicator"
    master = m.fp.master
    del m, comm
    gc.collect()  # the model's layers point back at it (reference cycles)
    assert RC.retired_count() == 0  # still alive: the graph holds it
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(master).all()
    del g, out
    torch.cuda.synchronize()
    freed, t0 = 0, time.time()
    while freed == 0 and time.time() - t0 < 10:  # the graph's user objects are released by HIP
        freed += RC.reap()
        time.sleep(0.05)
    assert freed == 1 and RC.retired_count() == 0


@pytest.mark.parametrize("mode,cycles", [("ipc1", 100), ("rccl1", 40)])
def test_capture_destroy_cycles_keep_the_heap_intact(cuda, mode, cycles):
    """bench_resnet's probe cycle -- rebuild the bucket reducer, two eager steps, capture the DP step,
    replay, DESTROY the graph -- repeated in a fresh process under glibc's heap checks
    (MALLOC_CHECK_=3). Issuing the comm-stream hand-offs from inside the autograd engine's backward
    thread broke the heap within 1-30 such cycles (round 4 kept every graph alive instead); they are
    issued from the caller's thread now (BucketReducer.mark_ready / finish)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MALLOC_CHECK_="3", MALLOC_PERTURB_="165")
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "debug", "rn_configure_loop.py"), mode,
                        str(cycles)], capture_output=True, text=True, timeout=280, cwd=root, env=env)
    assert p.returncode == 0 and "done" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


@pytest.mark.parametrize("depth", [18, 50])
def test_bn_bwd_stats_in_dgrad_epilogue(cuda, row_mode, depth, monkeypatch):
    """BN-backward statistics summed in the epilogue of the dgrad that produces the BN's dout
    (conv2d_dgrad_bn: relu mask from y for residual-free BNs, relu bits for the residual BN behind a
    residual-join conv) give the same gradients as bn_bwd's separate partial pass: only the fp32
    summation order of the per-channel sums differs. Both mask kinds must actually take the fused
    path."""
    from tensorflow_distributed_amd.models import resnet as R

    kinds = []
    orig = R._dgrad_bn

    def spy(dy, L, xs, acc, bn, fid, acc_bits=None, acc_sub2=False):
        kinds.append(("bits" if bn.fwd_state[3] is not None else "from_y", acc is not None))
        return orig(dy, L, xs, acc, bn, fid, acc_bits, acc_sub2)

    monkeypatch.setattr(R, "_dgrad_bn", spy)
    torch.manual_seed(depth)
    x = torch.randn(4, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    out = []
    for on in (False, True):
        m = R.ResNet(depth, num_classes=16, device=cuda, seed=3, width=16, zero_init_residual=False, bn_bwd_stats=on)
        m.fp.grad.zero_()
        loss, _ = m.loss(x, lab)
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.item(), m.fp.grad.clone()))
    assert abs(out[0][0] - out[1][0]) <= 1e-5 * abs(out[0][0])  # same forward (slot-mode sums: order may differ)
    g0, g1 = out[0][1], out[1][1]
    assert torch.isfinite(g1).all()
    rel = ((g1 - g0).norm() / g0.norm()).item()
    # the fused path also sums each residual join in another order (GradJoin defers the conv that
    # carries the statistics), so bf16 roundings differ; train-mode BN over these tiny batches
    # amplifies that to 0.8-1.6 % relative at depth 18 / 50 -- as much as the order change alone gives
    # at 8 x 64^2 images without any deferral (tools/debug/bn_bwd_stats_rel.py)
    assert rel < 3e-2, rel
    assert ("from_y", False) in kinds and ("bits", True) in kinds, kinds


@pytest.mark.parametrize("depth", [18, 50])
def test_folded_bn_matches_unfused(cuda, row_mode, depth):
    """The forward BN fold (single-consumer relu BNs applied inside the consuming conv's operand
    loader, _BNReluConv) against the separate bn_apply pass (fold_bn=False, the oracle): the same loss,
    running statistics and parameter gradients -- bit for bit (same constants, same rounding; only
    split-K weight-gradient atomics could reorder fp32 adds)."""
    from tensorflow_distributed_amd.models import resnet as R

    calls = []
    orig = R._BNReluConv.forward

    def spy(ctx, *a):
        calls.append(1)
        return orig(ctx, *a)

    torch.manual_seed(depth + 1)
    x = torch.randn(4, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    out = []
    for fold in (False, True):
        m = R.ResNet(depth, num_classes=16, device=cuda, seed=3, width=16, zero_init_residual=False, fold_bn=fold)
        R._BNReluConv.forward = staticmethod(spy) if fold else staticmethod(orig)
        try:
            m.fp.grad.zero_()
            loss, _ = m.loss(x, lab)
            loss.backward()
        finally:
            R._BNReluConv.forward = staticmethod(orig)
        torch.cuda.synchronize()
        out.append((loss.item(), m.fp.grad.clone(), torch.cat([torch.cat([b.rmean, b.rvar]) for b in m.bns])))
    nfold = len(m.blocks) * (1 if depth == 18 else 2)
    assert len(calls) == nfold, (len(calls), nfold)
    _same_run(out[0][0], out[1][0], out[0][1], out[1][1])
    if torch.ops.tfd.bn_part_slots() == 0:
        assert torch.equal(out[0][2], out[1][2])
    else:
        torch.testing.assert_close(out[0][2], out[1][2], rtol=1e-5, atol=1e-6)


def test_second_forward_before_backward_keeps_bn_state_per_forward(cuda):
    """Two train-mode forwards, then the FIRST one's backward: the BN-backward statistics the dgrad
    epilogues would take from the layers' saved forward state belong to the second forward, so the
    tagged state must be refused (the BN backward runs its own partial pass) -- the gradients equal
    a clean forward + backward of the first batch."""
    from tensorflow_distributed_amd.models.resnet import ResNet

    torch.manual_seed(21)
    x1 = torch.randn(4, 32, 32, 3, device=cuda)
    x2 = torch.randn(4, 32, 32, 3, device=cuda) * 3 + 1
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    grads = []
    for second in (False, True):
        m = ResNet(50, num_classes=16, device=cuda, seed=3, width=16, zero_init_residual=False)
        m.fp.grad.zero_()
        l1, _ = m.loss(x1, lab)
        if second:
            m.loss(x2, lab)  # its graph is dropped; its BN states overwrite the layers' ones
        l1.backward()
        torch.cuda.synchronize()
        grads.append(m.fp.grad.clone())
    rel = ((grads[1] - grads[0]).norm() / grads[0].norm()).item()
    # the refused states also turn off GradJoin's deferral, so the joins sum in another order: the
    # tiny-batch amplification of bf16 rounding (see test_bn_bwd_stats_in_dgrad_epilogue) bounds this
    # at a few %; a wrong forward's statistics would be off by far more (x2 is scaled and shifted)
    assert rel < 3e-2, rel


@pytest.mark.parametrize("depth", [18, 50])
def test_masked_join_matches_materialised_dres(cuda, row_mode, depth):
    """Identity-shortcut gradients handed to the joining conv's dgrad epilogue as (dout, relu bits)
    (masked_join, the residual BN backward writes no dres) against the materialised dres tensor
    (the oracle): the masked dout is exactly the bf16 dres, so loss and every gradient are bit-equal.
    The masked operand must actually reach a dgrad epilogue."""
    from tensorflow_distributed_amd.models import resnet as R

    seen = []
    orig = R.GradJoin.arrive

    def spy(self, g=None, conv=None, masked=None):
        if masked is not None:
            seen.append(1)
        return orig(self, g, conv, masked)

    torch.manual_seed(depth + 7)
    x = torch.randn(4, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    out = []
    for on in (False, True):
        m = R.ResNet(depth, num_classes=16, device=cuda, seed=5, width=16, zero_init_residual=False)
        m.masked_join = on
        R.GradJoin.arrive = spy
        try:
            m.fp.grad.zero_()
            loss, _ = m.loss(x, lab)
            loss.backward()
        finally:
            R.GradJoin.arrive = orig
        torch.cuda.synchronize()
        out.append((loss.item(), m.fp.grad.clone()))
    assert seen, "no identity-shortcut gradient took the masked path"
    assert torch.isfinite(out[1][1]).all()
    _same_run(out[0][0], out[1][0], out[0][1], out[1][1])


@pytest.mark.parametrize("depth", [18, 50])
def test_bn_slot_mode_matches_row_mode(cuda, depth):
    """BN statistics as fp32 atomics into zeroed slots with the finalize inside the apply passes (the
    default; no bn_final launches) against row mode (per-block partial rows reduced by bn_final in a
    fixed order): the same loss, running statistics and gradients up to fp32 summation order (and the
    bf16 roundings a changed last bit can flip)."""
    from tensorflow_distributed_amd.models.resnet import ResNet

    torch.manual_seed(depth + 11)
    x = torch.randn(4, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    out = []
    old = torch.ops.tfd.bn_part_slots()
    try:
        for slots in (0, 4):
            torch.ops.tfd.set_bn_part_slots(slots)
            m = ResNet(depth, num_classes=16, device=cuda, seed=9, width=16, zero_init_residual=False)
            assert (m.stats.buf is None) == (slots == 0)
            m.fp.grad.zero_()
            loss, _ = m.loss(x, lab)
            loss.backward()
            torch.cuda.synchronize()
            out.append((loss.item(), m.fp.grad.clone(), torch.cat([torch.cat([b.rmean, b.rvar]) for b in m.bns])))
    finally:
        torch.ops.tfd.set_bn_part_slots(old)
    assert abs(out[0][0] - out[1][0]) <= 1e-5 * abs(out[0][0])
    torch.testing.assert_close(out[1][2], out[0][2], rtol=1e-5, atol=1e-6)
    g0, g1 = out[0][1], out[1][1]
    assert torch.isfinite(g1).all()
    assert ((g1 - g0).norm() / g0.norm()).item() < 1e-2


@pytest.mark.parametrize("depth", [18, 50])
def test_stride2_shortcut_gradient_on_its_own_grid(cuda, row_mode, depth, monkeypatch):
    """A downsample block's 1x1 stride-2 shortcut dgrad computed on its own (stride-2) grid and added
    at the even pixels inside the joining conv's dgrad epilogue (acc_sub2) against the full-grid
    dgrad with its zero phases written (TFD_JOIN_SUB2=0): the same loss, and gradients equal up to the
    fp32 order of the shortcut GEMM (bf16 roundings amplified through train-mode BN); the stride-2 form
    must actually be used."""
    from tensorflow_distributed_amd.models import resnet as R

    used = []
    orig = R._dgrad_bn

    def spy(dy, L, xs, acc, bn, fid, acc_bits=None, acc_sub2=False):
        used.append(acc_sub2)
        return orig(dy, L, xs, acc, bn, fid, acc_bits, acc_sub2)

    monkeypatch.setattr(R, "_dgrad_bn", spy)
    torch.manual_seed(depth + 3)
    x = torch.randn(4, 64, 64, 3, device=cuda)
    lab = torch.randint(0, 16, (4,), dtype=torch.int32, device=cuda)
    out = []
    for sub in (False, True):
        monkeypatch.setattr(R, "_JOIN_SUB2", sub)
        m = R.ResNet(depth, num_classes=16, device=cuda, seed=4, width=16, zero_init_residual=False)
        m.fp.grad.zero_()
        loss, _ = m.loss(x, lab)
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.item(), m.fp.grad.clone()))
    assert any(used), "no join took the stride-2 shortcut operand"
    assert out[0][0] == out[1][0]
    g0, g1 = out[0][1], out[1][1]
    assert torch.isfinite(g1).all()
    assert ((g1 - g0).norm() / g0.norm()).item() < 3e-2


def test_captured_graph_keeps_its_bn_mode(cuda):
    """The BN-statistics mode is a launch argument of every producer kernel (BnPart / BnFin), not a
    device global read at replay: a step graph captured in slot mode and replayed after
    set_bn_part_slots(0) still adds into the slots it was built for -- its losses track a twin model
    that never switched (only the fp32 atomic order differs), and nothing writes row-mode rows into
    the [S][2][C] slot buffers."""
    from tensorflow_distributed_amd.models.resnet import ResNet

    old = torch.ops.tfd.bn_part_slots()
    torch.manual_seed(31)
    x = torch.randn(8, 32, 32, 3, device=cuda)
    lab = torch.randint(0, 16, (8,), dtype=torch.int32, device=cuda)
    runs = []
    try:
        for switch in (False, True):
            torch.ops.tfd.set_bn_part_slots(4)
            m = ResNet(18, num_classes=16, device=cuda, seed=3, width=16)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    m.train_step(x, lab, lr=0.01)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = m.train_step(x, lab, lr=0.01)
            losses = []
            for i in range(4):
                if switch and i == 2:
                    torch.ops.tfd.set_bn_part_slots(0)
                g.replay()
                torch.cuda.synchronize()
                losses.append(float(out.item()))
            runs.append(losses)
    finally:
        torch.ops.tfd.set_bn_part_slots(old)
    a, b = runs
    assert all(v == v for v in a + b), runs
    for u, v in zip(a, b):
        assert abs(u - v) <= 1e-3 * abs(u), runs
