"""The conv/BN oracle and its checker (tests/conv_oracle.py), without a GPU: the references agree with
torch's fp64 ops and autograd, the checker catches each way a tiled kernel goes subtly wrong and names
the slice, and every exact case of the GPU test's tables is exact (so a failing GPU test cannot be an
input problem)."""
import pytest
import torch
import torch.nn.functional as F

import conv_oracle as O

F64 = torch.float64


def close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---------------------------------------------------------------- references against torch fp64
def test_bf16_rne_equals_the_cast_ties_included():
    g = torch.Generator().manual_seed(0)
    t = torch.cat([torch.randn(200000, generator=g) * 300, torch.arange(-2050.0, 2050.0),
                   torch.tensor([257.0, 259.0, 261.0, -257.0, 1.00390625, 0.0, -0.0, 3e38, 1e-40])])
    assert torch.equal(O.bf16_rne(t), t.to(torch.bfloat16).double())
    assert O.bf16_rne(torch.tensor([257.0, 259.0])).tolist() == [256.0, 260.0]  # ties go to the even neighbour
    assert O.bf16_trunc(torch.tensor([259.0, -259.0])).tolist() == [258.0, -258.0]
    assert O.tie_count(torch.tensor([257.0, 258.0, 255.0, 515.0, 514.0, 520.0])) == 2  # 257, and 514 (spacing 4 above 512)


@pytest.mark.parametrize("shape", O.T64 + O.STRIDED + [O.HALO[0]])
def test_conv_references_agree_with_torch_autograd(shape):
    N, H, W, C, K, R, st, pad = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(R, R, C, K, generator=g, dtype=F64).requires_grad_(True)
    y = nhwc(F.conv2d(nchw(x), w.permute(3, 2, 0, 1), stride=st, padding=pad))
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    dx, dw = torch.autograd.grad(y, [x, w], dy)
    close(O.conv_fwd(x.detach(), w.detach(), st, pad), y.detach())
    close(O.conv_dgrad(dy, w.detach(), (N, H, W, C), st, pad), dx)
    close(O.conv_wgrad(x.detach(), dy, R, R, st, pad), dw)
    add = torch.randn(N, H, W, C, generator=g, dtype=F64)
    close(O.conv_dgrad(dy, w.detach(), (N, H, W, C), st, pad, add), dx + add)
    bits = O.pack_bits(torch.rand(N * H * W, C, generator=g) < 0.5)
    keep = O.unpack_bits(bits, C).reshape(N, H, W, C)
    close(O.conv_dgrad(dy, w.detach(), (N, H, W, C), st, pad, add, bits), dx + add * keep)
    sub = torch.randn(N, (H + 1) // 2, (W + 1) // 2, C, generator=g, dtype=F64)
    full = torch.zeros(N, H, W, C, dtype=F64)
    full[:, ::2, ::2] = sub
    close(O.conv_dgrad(dy, w.detach(), (N, H, W, C), st, pad, sub, None, True), dx + full)


def test_relu_bit_layout():
    m = torch.zeros(2, 16, dtype=torch.bool)
    m[0, 0], m[0, 9], m[1, 15] = True, True, True
    b = O.pack_bits(m)
    assert b.tolist() == [[1, 2], [0, 128]]  # bit j of byte c/8 = channel 8 (c/8) + j
    assert torch.equal(O.unpack_bits(b, 16), m)


def test_linear_and_stem_references():
    from tensorflow_distributed_amd.models.resnet import pair_stem_weight, unpair_stem_grad
    g = torch.Generator().manual_seed(2)
    x, w, dy = (torch.randn(s, generator=g, dtype=F64) for s in ((5, 16), (16, 24), (5, 24)))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    gx, gw = torch.autograd.grad(xr @ wr, [xr, wr], dy)
    close(O.linear_dgrad(dy, w), gx)
    close(O.linear_wgrad(x, dy), gw)
    # the width-paired stem computes the 7x7 stride-2 conv of the channel-padded input
    c = O.exact_stem_case(2, 10, 12, 16)
    xpad = torch.zeros(2, 10, 12, 8, dtype=F64)
    xpad[..., :3] = c["x"]
    xp = torch.zeros(2, 10, 6, 8, dtype=F64)
    xp[..., :6] = c["x"].reshape(2, 10, 6, 6)
    wp = pair_stem_weight(c["w"])
    # paired conv: height stride 2 / pad 3, width stride 1 / left pad 2 over the paired pixels
    xpp = F.pad(nchw(xp), (2, 1, 3, 3))
    yp = nhwc(F.conv2d(xpp, wp.permute(3, 2, 0, 1), stride=(2, 1)))[:, :, :c["y"].shape[2]]
    close(yp, c["y"])
    dw = torch.full((7, 7, 8, 16), float("nan"), dtype=F64)
    wpr = wp.clone().requires_grad_(True)
    ypr = nhwc(F.conv2d(xpp, wpr.permute(3, 2, 0, 1), stride=(2, 1)))[:, :, :c["y"].shape[2]]
    unpair_stem_grad(torch.autograd.grad(ypr, [wpr], c["dy"])[0], dw)
    close(dw, c["dw"])


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_batchnorm_references_agree_with_torch_autograd(relu, res):
    g = torch.Generator().manual_seed(3)
    M, C = 37, 24
    y = (torch.randn(M, C, generator=g, dtype=F64) * 3 + 1).requires_grad_(True)
    gamma, beta = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    r = torch.randn(M, C, generator=g, dtype=F64) if res else None
    gam = gamma.clone().requires_grad_(True)
    bet = beta.clone().requires_grad_(True)
    z = F.batch_norm(y, None, None, gam, bet, training=True, eps=1e-5)
    z = z + r if res else z
    z = torch.relu(z) if relu else z
    dout = torch.randn(M, C, generator=g, dtype=F64)
    gy, gg, gb = torch.autograd.grad(z, [y, gam, bet], dout)
    out, mean, invstd, var = O.bn_fwd(y.detach(), gamma, beta, r, relu, 1e-5)
    close(out, z.detach())
    close(mean, y.detach().mean(0))
    close(var, y.detach().var(0, unbiased=False))
    dy, dz, dg, db = O.bn_bwd(dout, y.detach(), gamma, mean, invstd, (out > 0) if relu else None)
    close(dy, gy)
    close(dg, gg)
    close(db, gb)
    rm, rv = O.bn_running(torch.zeros(C), torch.ones(C), mean, var, M, 0.9)
    close(rv, 0.9 + 0.1 * y.detach().var(0, unbiased=True))
    close(rm, 0.1 * mean)
    rmean, rvar = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    inf = F.batch_norm(y.detach(), rmean, rvar, gamma, beta, training=False, eps=1e-5)
    close(O.bn_infer(y.detach(), gamma, beta, rmean, rvar, 1e-5, True), torch.relu(inf))
    # the statistics partials by definition
    mask = O.bn_mask(2, y.detach(), mean, invstd, gamma, beta, None)
    assert torch.equal(mask, O.bn_fwd(y.detach(), gamma, beta, None, False, 1e-5)[0] > 0)
    bits = O.pack_bits(mask)
    assert torch.equal(O.bn_mask(3, y.detach(), mean, invstd, gamma, beta, bits), mask)
    assert O.bn_mask(0, y.detach(), mean, invstd, gamma, beta, None).all()


@pytest.mark.parametrize("k,st,pad,H,W", [(3, 2, 1, 11, 9), (2, 2, 0, 9, 11), (3, 3, 1, 10, 10), (3, 1, 1, 8, 8), (3, 2, 1, 2, 2)])
def test_pool_references_agree_with_torch(k, st, pad, H, W):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, H, W, 8, generator=g, dtype=F64).requires_grad_(True)  # no ties: torch's choice is unique
    yr = nhwc(F.max_pool2d(nchw(x), k, st, pad))
    y, am = O.maxpool_fwd(x.detach(), k, st, pad)
    close(y, yr.detach())
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    close(O.maxpool_bwd(dy, am, (2, H, W, 8), k, st, pad), torch.autograd.grad(yr, [x], dy)[0])
    close(O.avgpool_fwd(x.detach()), x.detach().mean((1, 2)))
    d2 = torch.randn(2, 8, generator=g, dtype=F64)
    close(O.avgpool_bwd(d2, (2, H, W, 8)), torch.autograd.grad(x.mean((1, 2)), [x], d2)[0])


def test_maxpool_argmax_is_the_first_maximum_in_rs_order():
    x = torch.zeros(1, 3, 3, 8, dtype=F64)  # every window element ties
    y, am = O.maxpool_fwd(x, 3, 1, 1)
    # centre window: first element (r, s) = (0, 0); corner (0, 0): the first in-image tap is (1, 1) -> 4
    assert int(am[0, 1, 1, 0]) == 0 and int(am[0, 0, 0, 0]) == 4 and int(am[0, 2, 2, 0]) == 0 and int(am[0, 0, 2, 0]) == 3
    _, last = O.maxpool_fwd(x, 3, 1, 1, last=True)
    assert int(last[0, 1, 1, 0]) == 8


def test_softmax_xent_reference_agrees_with_torch():
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(5, 1001, generator=g, dtype=F64) * 3).requires_grad_(True)
    lab = torch.randint(0, 1001, (5,), generator=g)
    lr = F.cross_entropy(z, lab, reduction="none")
    loss, corr, dl = O.softmax_xent(z.detach(), lab)
    close(loss, lr.detach())
    close(dl, torch.autograd.grad(lr.mean(), [z])[0])
    assert torch.equal(corr, (z.detach().argmax(1) == lab).double())
    eq = torch.full((3, 10), 1.25, dtype=F64)
    _, c2, _ = O.softmax_xent(eq, torch.tensor([0, 1, 9]))
    assert c2.tolist() == [1.0, 0.0, 0.0]  # equal logits: the prediction is index 0
    big = torch.tensor([[80.0, -80.0, 80.0]], dtype=F64)
    l3, _, d3 = O.softmax_xent(big, torch.tensor([1]))
    assert torch.isfinite(l3).all() and torch.isfinite(d3).all() and abs(float(l3) - (160 + 0.6931471805599453)) < 1e-9


# ---------------------------------------------------------------- the checker names the slice
SHAPE = (2, 9, 10, 16, 24, 3, 1, 1)  # M = 180: two full 64-row tiles and 52 ragged rows


def _fwd():
    c = O.exact_fwd_case(SHAPE)
    return c, O.bf16_rne(c["y"]), lambda: O.layout_nhwc(*c["y"].shape)


def fails(got, ref, bound, layout):
    with pytest.raises(O.Mismatch) as e:
        O.check(got, ref, bound, layout, "mutated")
    return e.value


def test_checker_passes_a_correct_output():
    c, ref, lay = _fwd()
    O.check(ref.to(torch.bfloat16), ref, 0.0, lay)
    rc = O.random_conv_case(O.T64[0])
    N, H, W, C, K, R, st, pad = O.T64[0]
    O.check(O.bf16_rne(rc["y"]), rc["y"], O.bound_bf16(rc["y"], R * R * C, rc["yA"]), None)  # fp64 result rounded once
    O.check(rc["dw"].float(), rc["dw"], O.bound_f32(conv_l := O.conv_L(O.T64[0], "wgrad"), rc["dwA"]), None)
    assert conv_l == 2 * 9 * 7


def test_mutation_one_tap_scaled():
    """1.05 x on tap (2, 1): caught in the output, and in the filter gradient the tap is named."""
    c, ref, lay = _fwd()
    got = O.bf16_rne(O.conv_fwd(c["x"], c["w"], 1, 1, tap_scale={(2, 1): 1.05}))
    m = fails(got, ref, 0.0, lay)
    assert O.blame_tap(got, c["x"], c["w"], 1, 1, c["y"])[0] == (2, 1)
    assert m.names("out-channel 8-chunk")
    rc = O.random_conv_case(SHAPE)
    got = O.conv_fwd(rc["x"], rc["w"], 1, 1, tap_scale={(2, 1): 1.05})
    fails(O.bf16_rne(got), rc["y"], O.bound_bf16(rc["y"], 9 * 16, rc["yA"]), lay)  # random family too
    w = O.exact_wgrad_case(SHAPE)
    dw = w["dw"].clone()
    dw[2, 1] *= 1.05
    m = fails(dw, w["dw"], 0.0, lambda: O.layout_hwio(3, 3, 16, 24))
    assert m.only("tap") == "tap (r, s) = (2, 1)"
    rw = O.random_conv_case(SHAPE)
    dw = rw["dw"].clone()
    dw[2, 1] *= 1.05
    m = fails(dw, rw["dw"], O.bound_f32(O.conv_L(SHAPE, "wgrad"), rw["dwA"]), lambda: O.layout_hwio(3, 3, 16, 24))
    assert m.only("tap") == "tap (r, s) = (2, 1)"


def test_mutation_one_output_channel_chunk_scaled():
    c, ref, lay = _fwd()
    y = c["y"].clone()
    y[..., 8:16] *= 1.02
    m = fails(O.bf16_rne(y), ref, 0.0, lay)
    assert m.only("out-channel 8-chunk") == "channels 8..15"
    rc = O.random_conv_case(SHAPE)
    y = rc["y"].clone()
    y[..., 8:16] *= 1.02
    m = fails(O.bf16_rne(y), rc["y"], O.bound_bf16(rc["y"], 9 * 16, rc["yA"]), lay)
    assert m.only("out-channel 8-chunk") == "channels 8..15"


def test_mutation_padding_shifted_on_one_edge():
    """The left column computed as if the padding were one pixel narrower (reads the wrapped pixel)."""
    c, ref, lay = _fwd()
    N, H, W, C, K, R, st, pad = SHAPE
    xs = torch.roll(c["x"], 1, dims=2)  # column -1 becomes the last column instead of zero
    wrong = O.conv_fwd(torch.cat([xs[:, :, :1], c["x"]], 2), c["w"], 1, 1)[:, :, 1:]
    y = c["y"].clone()
    y[:, :, 0] = wrong[:, :, 0]
    m = fails(O.bf16_rne(y), ref, 0.0, lay)
    assert all("left column" in n for n in m.names("border")) and m.names("border")
    assert "interior" not in m.names("border")


def test_mutation_ragged_last_rows_zero():
    c, ref, lay = _fwd()
    y = c["y"].clone().reshape(-1, 24)
    M = y.shape[0]
    assert M % 64 == 52
    y[M - M % 64:] = 0
    m = fails(O.bf16_rne(y).reshape(ref.shape), ref, 0.0, lay)
    assert m.only("m_tile64") == f"rows 128..{M - 1}"


def test_mutation_one_stride2_phase_dropped():
    shape = O.STRIDED[0]
    N, H, W, C, K, R, st, pad = shape
    c = O.exact_dgrad_case(shape)
    got = O.conv_dgrad(c["dy"], c["w"], (N, H, W, C), st, pad, drop_phase=(1, 0))
    m = fails(O.bf16_rne(got), O.bf16_rne(c["dx"]), 0.0, lambda: O.layout_nhwc(N, H, W, C, stride=st, name="in-channel"))
    assert m.only("phase") == "phase (h%2, w%2) = (1, 0)"


def test_mutation_bf16_truncation():
    c, ref, lay = _fwd()
    assert O.tie_count(c["y"]) > 0 and float(c["y"].abs().max()) > 256
    fails(O.bf16_trunc(c["y"]), ref, 0.0, lay)
    # on ties alone: truncation and round-half-up both differ from nearest-even somewhere
    t = torch.tensor([257.0, 259.0, -257.0, -259.0])
    assert not torch.equal(O.bf16_trunc(t), O.bf16_rne(t))


def test_mutation_relu_bit_order_reversed():
    shape = O.T64[0]
    N, H, W, C, K, R, st, pad = shape
    c = O.exact_dgrad_case(shape, add="bits")
    keep = O.unpack_bits(c["bits"], C, reverse=True).reshape(N, H, W, C)
    got = O.conv_dgrad(c["dy"], c["w"], (N, H, W, C), st, pad) + c["add"] * keep
    m = fails(O.bf16_rne(got), O.bf16_rne(c["dx"]), 0.0, lambda: O.layout_nhwc(N, H, W, C, name="in-channel"))
    assert len(m.names("in-channel 8-chunk")) == C // 8  # every byte is affected, no spatial pattern
    # and as the BN-backward mask (mode 3): the partials differ
    cb = O.exact_dgrad_case(shape, bn_mode=3)
    wrong = O.dgrad_bn_stats(cb["dx"], cb["y"], cb["mean"], cb["invstd"], O.unpack_bits(cb["mask_bits"], C, reverse=True))
    fails(wrong, cb["stats"], 0.0, lambda: O.layout_stats(C))


def test_mutation_stats_include_rows_past_m():
    """A partial that also sums what a kernel leaves in the tile rows past M (here: a copy of row 0)."""
    c = O.exact_fwd_case(SHAPE, stats=True)
    yb = O.bf16_rne(c["y"]).reshape(-1, 24)
    ghost = torch.cat([yb, yb[:1].expand(64 - yb.shape[0] % 64, 24)])
    wrong = torch.stack([ghost.sum(0), (ghost * ghost).sum(0)])
    m = fails(wrong, c["stats"], 0.0, lambda: O.layout_stats(24))
    assert "sum b" in m.names("statistic")


def test_mutation_argmax_takes_the_last_maximum():
    x = O.tie_pool_input(2, 9, 11, 16)
    y, am = O.maxpool_fwd(x, 3, 2, 1)
    y2, am2 = O.maxpool_fwd(x, 3, 2, 1, last=True)
    assert torch.equal(y, y2)
    lay = lambda: O.layout_nhwc(*y.shape, name="channel")  # noqa: E731
    fails(am2.double(), am.double(), 0.0, lay)
    dy = torch.ones(y.shape, dtype=F64)
    fails(O.maxpool_bwd(dy, am2, tuple(x.shape), 3, 2, 1), O.maxpool_bwd(dy, am, tuple(x.shape), 3, 2, 1), 0.0,
          lambda: O.layout_nhwc(*x.shape, name="channel"))


def test_checker_reports_halo_tile_and_image():
    c, ref, lay = _fwd()
    y = ref.clone()
    y[1, 8:, :, :] += 2  # image 1, rows 8.. : halo tile row 1
    m = fails(y, ref, 0.0, lay)
    assert m.only("image") == "image 1" and m.only("halo tile") == "tile (h/8, w/16) = (1, 0)"
    y = ref.clone()
    y[0, 0, 0, 0] = float("nan")
    assert fails(y, ref, 1e30, lay).only("image") == "image 0"  # a non-finite value is beyond every bound


# ---------------------------------------------------------------- every exact case is exact
def test_every_exact_case_of_the_gpu_tables_is_exact():
    """The generators assert sum |a||b| < 2^24 (and the statistics' sums) themselves; run them all. The
    big maps are generated at their real size: this is what the GPU test feeds the kernels."""
    ties = 0
    for s in O.FWD_SHAPES:
        c = O.exact_fwd_case(s)
        ties += O.tie_count(c["y"])
        cs = O.exact_fwd_case(s, stats=True)
        assert float(cs["stats"][1].max()) < O.EXACT_LIMIT
    assert ties > 1000  # exact values beyond 256 on bf16 ties
    for s in O.DGRAD_SHAPES:
        for a in O.dgrad_adds(s):
            O.exact_dgrad_case(s, add=a)
    for s in O.DGRAD_BN_SHAPES:
        for mode in (0, 2, 3):
            c = O.exact_dgrad_case(s, add="plain", bn_mode=mode)
            assert float(c["stats"].abs().max()) < O.EXACT_LIMIT
            x = (c["y"].reshape(-1, s[3]) - c["mean"]) * c["invstd"]
            assert torch.equal(x, torch.round(x))  # xhat is an integer
            if mode != 0:
                assert 0.05 < c["mask"].double().mean() < 0.95  # the mask acts
    for s in O.WGRAD:
        assert float(O.exact_wgrad_case(s)["dw"].abs().max()) > 256
    for s in O.FOLD:
        c = O.exact_fwd_case(s, stats=True, fold=True)
        assert (c["xin"] == 0).any() and (c["xin"] > 0).any()  # the relu acts
        sh = c["beta"] - c["mean"] * c["invstd"] * c["gamma"]
        assert (sh > 0).any()  # a padded tap put through the affine would not stay zero
        O.exact_wgrad_case(s, fold=True)
    for s in O.STEM:
        O.exact_stem_case(*s)
    for M, Kin, N in O.LINEAR:
        O.exact_gemm_case(M, Kin, N)
    for M, N, K in O.GEMM_NT:
        O.exact_gemm_case(M, K, N)
    for s, op in O.RANDOM_CASES:
        assert O.conv_L(s, op) <= O.MAX_L
