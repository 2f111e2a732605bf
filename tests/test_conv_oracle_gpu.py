"""The generic NHWC kernel library (csrc/kernels/conv_nhwc.hip, csrc/conv_halo.h, csrc/gemm256.h,
csrc/kernels/norm.hip) against the fp64 oracles of tests/conv_oracle.py, element by element.

Exact family: integer-valued operands whose every product sum stays below 2^24, so each fp32 output
has one right value and each bf16 output is its round-to-nearest-even -- the tests demand bit
equality on every tile path (64x64, 128x64, 128x128, the 256-row core's three widths, halo tiles,
strided-dgrad phases, split-K, slot-mode atomics), with ragged M / N tails. Random family: bf16 normal
operands at reduction lengths <= 1152 against the derived per-element bound (conv_oracle's module
docstring; the batch-norm and cross-entropy bounds are derived next to their run_* helpers). A
failure names the slices (tap, channel chunk, M tile, border, phase, halo tile) that hold the bad
elements. The shape tables live in conv_oracle so that tests/test_conv_oracle_checker_cpu.py can show
every exact case exact without a GPU."""
import pytest
import torch

import conv_oracle as O

pytestmark = pytest.mark.gpu
ops = None


@pytest.fixture(autouse=True, params=[(0, 0), (2, 0), (1, 2)], ids=["core128", "core256", "halo"])
def _ops(cuda, request):
    """Every test on every GEMM path, as in test_conv_ops_gpu.py: the 128-row core, the 256-row core
    wherever it applies, and the LDS halo-tile kernel for every eligible 3x3 stride-1 conv."""
    global ops
    ops = torch.ops.tfd
    core, halo = request.param
    old = ops.conv_gemm_core(core), ops.conv_halo_mode(halo)
    yield
    ops.conv_gemm_core(old[0])
    ops.conv_halo_mode(old[1])


@pytest.fixture(params=[0, 4], ids=["rowmode", "slots4"])
def bn_mode(request):
    """Statistics partials in row mode (one row per producer block) and in slot mode (fp32 atomics
    into 4 zeroed slots)."""
    old = torch.ops.tfd.set_bn_part_slots(request.param)
    yield request.param
    torch.ops.tfd.set_bn_part_slots(old)


def check_all(checks):
    for what, got, ref, bound, layout in checks:
        O.check(got, ref, bound, layout, what)


def ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


# ---------------------------------------------------------------- exact family
@pytest.mark.parametrize("shape", O.FWD_SHAPES, ids=ids(O.FWD_SHAPES))
def test_exact_conv_fwd(cuda, shape):
    check_all(O.run_fwd_exact(ops, cuda, shape))


@pytest.mark.parametrize("shape", O.FWD_SHAPES, ids=ids(O.FWD_SHAPES))
def test_exact_conv_fwd_stats(cuda, bn_mode, shape):
    """y equal to conv2d_fwd's and to the oracle; the summed partials equal to the column sums and sums
    of squares of the stored bf16 output (rows past M must add nothing)."""
    check_all(O.run_fwd_stats_exact(ops, cuda, shape))


DGRAD = [(s, a) for s in O.DGRAD_SHAPES for a in O.dgrad_adds(s)]


@pytest.mark.parametrize("shape,add", DGRAD, ids=[f"{i}-{a}" for (s, a), i in zip(DGRAD, ids([s for s, _ in DGRAD]))])
def test_exact_conv_dgrad(cuda, shape, add):
    """Plain, + add, + relu-bit-masked add (stride 1), + the stride-2 operand at the even pixels. Input
    rows and columns that no tap reaches are 0 (or the add)."""
    check_all(O.run_dgrad_exact(ops, cuda, shape, add))


DGRAD_BN = [(s, m, a) for s in O.DGRAD_BN_SHAPES for m in (0, 2, 3) for a in (None, "plain", "bits", "sub2")
            if a in O.dgrad_adds(s) and (a in (None, "plain") or s[0] * s[1] * s[2] < 4096)]


@pytest.mark.parametrize("shape,mode,add", DGRAD_BN,
                         ids=[f"{i}-mode{m}-{a}" for (s, m, a), i in zip(DGRAD_BN, ids([s for s, _, _ in DGRAD_BN]))])
def test_exact_conv_dgrad_bn(cuda, bn_mode, shape, mode, add):
    """dx, the summed BN-backward partials (mask modes 0, 2, 3) and the dgamma / dbeta that
    bn_bwd(partials=...) makes of them, against the oracle."""
    check_all(O.run_dgrad_bn_exact(ops, cuda, shape, mode, add))


@pytest.mark.parametrize("zeroed", [False, True], ids=["clears", "zeroed"])
@pytest.mark.parametrize("shape", O.WGRAD, ids=ids(O.WGRAD))
def test_exact_conv_wgrad(cuda, shape, zeroed):
    check_all(O.run_wgrad_exact(ops, cuda, shape, zeroed))


@pytest.mark.parametrize("shape", O.FOLD, ids=ids(O.FOLD))
def test_exact_folded_bn_input(cuda, bn_mode, shape):
    """mean ... beta given to conv2d_fwd / conv2d_fwd_stats / conv2d_wgrad, against the oracle itself
    (relu(bn(x)) then zero padding: padded taps stay zero after the affine and the relu)."""
    check_all(O.run_fold_exact(ops, cuda, shape))


@pytest.mark.parametrize("shape", O.STEM, ids=ids(O.STEM))
def test_exact_width_paired_stem(cuda, bn_mode, shape):
    check_all(O.run_stem_exact(ops, cuda, shape))


@pytest.mark.parametrize("shape", O.LINEAR, ids=ids(O.LINEAR))
def test_exact_linear(cuda, shape):
    check_all(O.run_linear_exact(ops, cuda, shape))


@pytest.mark.parametrize("shape", O.GEMM_NT, ids=ids(O.GEMM_NT))
def test_exact_gemm_nt(cuda, shape):
    check_all(O.run_gemm_nt_exact(ops, cuda, shape))


@pytest.mark.parametrize("shape", O.POOLS, ids=ids(O.POOLS))
def test_exact_maxpool(cuda, shape):
    """Integer inputs dense with ties: output, argmax (the first maximum in (r, s) order) and the
    backward's scatter, H or W below k included."""
    check_all(O.run_maxpool_exact(ops, cuda, shape))


@pytest.mark.parametrize("N,H,W,C", [(2, 16, 16, 64), (3, 15, 13, 32)])
def test_bn_relu_maxpool_on_ties(cuda, bn_mode, N, H, W, C):
    """bn_relu_maxpool on a tie-heavy integer conv output: output and argmax equal bn_fwd + maxpool2d_fwd,
    and that argmax is the oracle's first maximum of bn_fwd's stored output."""
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-1, 2, (N, H, W, 8), generator=g).to(cuda, torch.bfloat16)
    w = (torch.randint(-1, 2, (3, 3, 8, C), generator=g) * (torch.rand(3, 3, 8, C, generator=g) < 0.25)).to(cuda, torch.bfloat16)
    y, part = ops.conv2d_fwd_stats(x, w, 1, 1)  # a handful of small integers: few distinct values
    gm, b = (torch.rand(C, generator=g) + 0.5).to(cuda), torch.randn(C, generator=g).to(cuda)
    rm0, rv0 = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    rm1, rv1 = rm0.clone(), rv0.clone()
    bo, m0, i0 = ops.bn_fwd(y, gm, b, None, True, rm0, rv0, 0.9, 1e-5, part)
    p0, a0 = ops.maxpool2d_fwd(bo, 3, 2, 1)
    p1, a1, m1, i1 = ops.bn_relu_maxpool(y, gm, b, rm1, rv1, 0.9, 1e-5, part, 3, 2, 1)
    ry, ram = O.maxpool_fwd(bo.cpu().double(), 3, 2, 1)
    win = O._windows(bo.cpu().double(), 3, 2, 1, float("-inf"))
    assert ((win == ry[..., None]).sum(-1) > 1).float().mean() > 0.1  # an input property: many windows tie
    lay = lambda: O.layout_nhwc(*ry.shape, name="channel")  # noqa: E731
    O.check(p1, ry, 0.0, lay, "bn_relu_maxpool out")
    O.check(a1, ram.double(), 0.0, lay, "bn_relu_maxpool argmax")
    O.check(p0, ry, 0.0, lay, "maxpool2d_fwd out")
    O.check(a0, ram.double(), 0.0, lay, "maxpool2d_fwd argmax")
    for u, v in ((m1, m0), (i1, i0), (rm1, rm0), (rv1, rv0)):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N,H,W,C", [(3, 7, 7, 64), (2, 4, 4, 16), (3, 7, 7, 12), (1, 1, 1, 8)])
def test_exact_avgpool_bwd_and_derived_fwd(cuda, N, H, W, C):
    """avgpool_bwd = bf16_rne(fp32(dy) / fp32(HW)), the IEEE fp32 quotient (chunk and scalar kernels);
    avgpool_fwd within the derived bound of an fp32 sum of HW terms, one division and one bf16 rounding."""
    g = torch.Generator().manual_seed(N + H + C)
    dy = O.randn_bf16(g, (N, C))
    da = ops.avgpool_bwd(dy.to(cuda, torch.bfloat16), [N, H, W, C])
    want = O.bf16_rne(dy.float() / float(H * W))[:, None, None, :].expand(N, H, W, C)
    O.check(da, want, 0.0, lambda: O.layout_nhwc(N, H, W, C, name="channel"), "avgpool_bwd")
    x = O.randn_bf16(g, (N, H, W, C))
    a = ops.avgpool_fwd(x.to(cuda, torch.bfloat16))
    ref, A = O.avgpool_fwd(x), O.avgpool_fwd(x.abs())
    O.check(a, ref, O.bound_bf16(ref, H * W + 1, A), lambda: O.layout_rows(N, C), "avgpool_fwd")


@pytest.mark.parametrize("P,cin,cout", [(1, 3, 8), (37, 3, 8), (300, 5, 16), (65, 8, 8)])
def test_exact_pad_channels_and_stem_pack(cuda, P, cin, cout):
    """fp32 -> bf16 round-to-nearest-even (ties in the data), zero fill of the padded channels."""
    g = torch.Generator().manual_seed(P)
    x = torch.randn(P, cin, generator=g) * 300
    x[::3] = torch.round(x[::3])  # integers beyond 256: bf16 ties among them
    x[0, 0] = 257.0
    p = ops.pad_channels(x.to(cuda), cout)
    want = torch.zeros(P, cout, dtype=torch.float64)
    want[:, :cin] = O.bf16_rne(x)
    O.check(p, want, 0.0, lambda: O.layout_rows(P, cout), "pad_channels")
    x3 = torch.round(torch.randn(2, 5, 2 * P, 3, generator=g) * 300)
    xp = ops.stem_pack(x3.to(cuda))
    w3 = torch.zeros(2, 5, P, 8, dtype=torch.float64)
    w3[..., :6] = O.bf16_rne(x3).reshape(2, 5, P, 6)
    O.check(xp, w3, 0.0, lambda: O.layout_nhwc(2, 5, P, 8, name="channel"), "stem_pack")


# ---------------------------------------------------------------- random family
@pytest.mark.parametrize("shape,op", O.RANDOM_CASES, ids=[f"{i}-{op}" for (s, op), i in
                                                           zip(O.RANDOM_CASES, ids([s for s, _ in O.RANDOM_CASES]))])
def test_random_conv_within_derived_bound(cuda, shape, op):
    check_all(O.run_conv_random(ops, cuda, shape, op))


@pytest.mark.parametrize("relu,res,src", O.bn_combos(), ids=[f"relu{int(r)}-res{int(q)}-{s}" for r, q, s in O.bn_combos()])
@pytest.mark.parametrize("M,C", O.BN_SHAPES)
def test_random_batchnorm_within_derived_bound(cuda, M, C, relu, res, src):
    """bn_fwd (statistics, running statistics, output, relu bits) and bn_bwd (dy, dres, dgamma, dbeta) at
    the thread layouts of row_split: C = 8 (one thread per row), 24 (three), 2048 (one row group),
    M = 1 and M below the row groups."""
    check_all(O.run_bn_random(ops, cuda, M, C, relu, res, src))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", O.BN_SHAPES)
def test_random_bn_infer_within_derived_bound(cuda, M, C, relu):
    check_all(O.run_bn_infer_random(ops, cuda, M, C, relu))


@pytest.mark.parametrize("name", list(O.xent_cases()))
def test_softmax_xent(cuda, name):
    """Loss, prediction (the first maximal logit) and dlogits against fp64: normal rows, rows of equal
    logits, logits of +-80 (finite loss), a label on a tied maximum that is not the first."""
    checks = O.run_xent(ops, cuda, name)
    assert torch.isfinite(checks[0][1]).all() and torch.isfinite(checks[2][1].float()).all()
    if name.startswith("equal"):
        z, lab = O.xent_cases()[name]
        assert torch.equal(checks[1][2], (lab == 0).double())
    if name.startswith("tied") and O.xent_cases()[name][0].shape[1] > 2:
        assert not checks[1][2].any()  # the prediction is index 1, the label is the last maximum
    check_all(checks)


# ---------------------------------------------------------------- host checks
def test_shapes_the_kernels_cannot_run_raise(cuda):
    bf = dict(device=cuda, dtype=torch.bfloat16)
    f = dict(device=cuda)

    def vec(c):
        return torch.ones(c, **f)

    y = torch.zeros(4, 16, **bf)
    ok = (y, y, y, vec(16), vec(16), vec(16), False, False, vec(16), vec(16))
    ops.bn_bwd(*ok)  # the well-formed call runs
    bad_bwd = [
        (torch.zeros(4, 12, **bf),) * 3 + (vec(12), vec(12), vec(12), False, False, vec(12), vec(12)),       # C % 8
        (torch.zeros(2, 2056, **bf),) * 3 + (vec(2056), vec(2056), vec(2056), False, False, vec(2056), vec(2056)),  # C > 2048
        (y, y, y, vec(8), vec(16), vec(16), False, False, vec(16), vec(16)),                                # gamma size
        (y, y, y, vec(16), vec(16), vec(16).double(), False, False, vec(16), vec(16)),                      # invstd dtype
        (y, y, y, vec(16), vec(32)[::2], vec(16), False, False, vec(16), vec(16)),                          # mean strided
        (y, y, y, vec(16), vec(16), vec(16), False, False, vec(8), vec(16)),                                # dgamma size
        (y[:2], y, y, vec(16), vec(16), vec(16), False, False, vec(16), vec(16)),                           # dout shape
    ]
    for a in bad_bwd:
        with pytest.raises(RuntimeError):
            ops.bn_bwd(*a)
    ops.bn_infer(y, vec(16), vec(16), vec(16), vec(16), 1e-5, True)
    bad_inf = [
        (torch.zeros(4, 12, **bf), vec(12), vec(12), vec(12), vec(12)),
        (torch.zeros(2, 2056, **bf), vec(2056), vec(2056), vec(2056), vec(2056)),
        (y, vec(8), vec(16), vec(16), vec(16)),
        (y, vec(16), vec(16), vec(16).double(), vec(16)),
        (y, vec(16), vec(16), vec(16), vec(32)[::2]),
        (y, vec(16), vec(16).cpu(), vec(16), vec(16)),
    ]
    for a in bad_inf:
        with pytest.raises(RuntimeError):
            ops.bn_infer(*a, 1e-5, False)
    dy = torch.zeros(1, 2, 2, 8, **bf)
    am = torch.zeros(1, 2, 2, 8, device=cuda, dtype=torch.uint8)
    ops.maxpool2d_bwd(dy, am, [1, 4, 4, 8], 2, 2, 0)
    for a in [(dy, am.int(), [1, 4, 4, 8], 2, 2, 0), (dy, am[:, :1], [1, 4, 4, 8], 2, 2, 0), (dy, am, [1, 6, 4, 8], 2, 2, 0),
              (dy, am, [1, 4, 4, 16], 2, 2, 0), (torch.zeros(1, 2, 2, 12, **bf), torch.zeros(1, 2, 2, 12, device=cuda, dtype=torch.uint8),
                                                   [1, 4, 4, 12], 2, 2, 0), (dy, am.cpu(), [1, 4, 4, 8], 2, 2, 0)]:
        with pytest.raises(RuntimeError):
            ops.maxpool2d_bwd(*a)
    for a in [(torch.zeros(2, 8, **bf), [3, 2, 2, 8]), (torch.zeros(2, 8, **bf), [2, 2, 2, 16]), (torch.zeros(2, 8, **bf), [2, 2, 8]),
              (torch.zeros(2, 8, **bf), [2, 0, 2, 8])]:
        with pytest.raises(RuntimeError):
            ops.avgpool_bwd(*a)
    for x in (torch.zeros(2, 0, 3, 8, **bf), torch.zeros(2, 3, 8, **bf)):
        with pytest.raises(RuntimeError):
            ops.avgpool_fwd(x)
