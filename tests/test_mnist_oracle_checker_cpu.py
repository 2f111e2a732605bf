"""The localised oracle checker (tests/mnist_oracle.py) on the host: its own output passes, every
localised mutation is named.

The six mutations of the first test are the ones that pass the whole-tensor bounds of
test_step_grads_match_oracle (seed 0, B = 128, scale 0.05); the rest cover the activations, the pool
argmax, the loss rows and the prediction flags. bf16 bounds are exercised on an oracle output carrying
noise of the kind the bf16 step has; fp32 bounds on the unperturbed output.
"""
import pytest
import torch

import mnist_oracle as O

B = 128
KEYS = ("pool1", "pool2", "hidden", "loss_rows", "correct_rows", "idx1", "idx2", "dlogits", "dh")


def _bf16_noise(ref):
    """What separates a correct bf16 step from the oracle: a stored bf16 activation now and then rounds to
    the neighbouring bf16 number (the kernel sums in fp32, the oracle in fp64), at about the measured
    rates; the gradients, fp32 sums over bf16 operands, inherit half a bf16 rounding error (2^-10) per
    entry. Loss rows and out_b never pass through bf16: they carry fp32 rounding only."""
    g = torch.Generator().manual_seed(1)

    def flip(t, rate):
        ulp = torch.where(t != 0, 2.0 ** (torch.floor(torch.log2(t.abs().clamp_min(1e-300))) - 7), torch.zeros_like(t))
        hit = torch.rand(t.shape, generator=g, dtype=torch.float64) < rate
        sign = torch.where(torch.rand(t.shape, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
        return torch.where(hit, t + sign * ulp, t)

    got = {k: ref[k].clone() for k in KEYS}
    got["pool1"] = flip(ref["pool1"], 1e-4)
    got["pool2"] = flip(ref["pool2"], 1e-3)
    got["hidden"] = flip(ref["hidden"], 1e-3)
    got["dh"] = flip(ref["dh"], 1e-3)
    got["loss_rows"] = ref["loss_rows"].float().double()
    got["dlogits"] = ref["dlogits"].float().double()
    got["grads"] = {}
    for k, v in ref["grads"].items():
        u = torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1
        got["grads"][k] = v.float().double() if k == "out_b" else v * (1 + 2.0 ** -10 * u)
    return got


@pytest.fixture(scope="module", params=["bf16", "fp32"])
def case(request):
    dtype = request.param
    params, x, y = O.random_case(B, 0.05, 0)
    ref = O.oracle_step(params, x, y, dtype)
    if dtype == "bf16":
        base = _bf16_noise(ref)
    else:
        base = {k: ref[k].clone() for k in KEYS}
        base["grads"] = {k: v.clone() for k, v in ref["grads"].items()}
    return dtype, ref, base


def _mutated(base, tensor, fn):
    got = dict(base)
    if tensor in O.GRADS:
        got["grads"] = dict(base["grads"])
        got["grads"][tensor] = base["grads"][tensor].clone()
        fn(got["grads"][tensor])
    else:
        got[tensor] = base[tensor].clone()
        fn(got[tensor])
    return got


def _named(case, tensor, fn):
    dtype, ref, base = case
    bad = O.check(_mutated(base, tensor, fn), ref, dtype)
    assert any(k[0] == tensor for k in bad), f"{dtype}: the mutation of {tensor} passes; flagged: {sorted(bad)}"
    assert all(k[0] == tensor for k in bad), f"{dtype}: other tensors flagged too: {bad}"


def test_own_output_passes(case):
    dtype, ref, base = case
    assert O.check(base, ref, dtype) == {}
    worst = O.measure(base, ref)
    if dtype == "bf16":  # the noise is not vacuous: it uses a good part of several bounds
        assert max(e / O.bound_for(k, ref, dtype) for k, (e, _) in worst.items()) > 0.3


def _scale(index, f):
    def fn(t):
        t[index] *= f
    return fn


def _nearest_rms(t):
    rms = t.pow(2).mean().sqrt()
    return int((t.abs() - rms).abs().argmin())


@pytest.mark.parametrize("name", ["wc2_tap", "wc2_cout", "wc1_cout", "bc2_elem", "wd1_pixel", "wd1_zero"])
def test_mutations_that_pass_the_whole_tensor_bounds(case, name):
    if name == "wc2_tap":
        _named(case, "wc2", _scale((4, 4), 1.04))
    elif name == "wc2_cout":
        _named(case, "wc2", _scale((Ellipsis, 63), 1.05))
    elif name == "wc1_cout":
        _named(case, "wc1", _scale((Ellipsis, 31), 1.05))
    elif name == "bc2_elem":
        _named(case, "bc2", _scale(63, 1.05))
    elif name == "wd1_pixel":  # the 64 fc1 rows of pool pixel (6, 6)
        r0 = (6 * 7 + 6) * 64
        _named(case, "wd1", _scale(slice(r0, r0 + 64), 1.05))
    else:  # one element of ordinary size set to zero

        def zero(t):
            t.view(-1)[_nearest_rms(case[1]["grads"]["wd1"].reshape(-1))] = 0.0

        _named(case, "wd1", zero)


def test_wc1_tap_scaled(case):
    _named(case, "wc1", _scale((2, 2), 0.9))


@pytest.mark.parametrize("tensor", ["pool1", "pool2"])
def test_image_copied_from_its_neighbour(case, tensor):
    def copy(t):
        t[3] = t[4]

    _named(case, tensor, copy)


@pytest.mark.parametrize("tensor,win,pool", [("idx1", "win1", "pool1"), ("idx2", "win2", "pool2")])
def test_pool_argmax_moved(case, tensor, win, pool):
    ref = case[1]
    w = ref[win].reshape(-1, 4)
    moved = (ref[tensor].reshape(-1) + 1) % 4
    regret = w.max(-1).values - w.gather(-1, moved[:, None])[:, 0]
    # a window where the neighbouring position is clearly not the maximum (a tenth of the RMS short)
    i = int((regret > 0.1 * ref[pool].pow(2).mean().sqrt()).nonzero()[0])

    def move(t):
        t.view(-1)[i] = moved[i]

    _named(case, tensor, move)


def test_loss_row_scaled(case):
    i = int(case[1]["loss_rows"].argsort()[B // 2])  # the median row
    _named(case, "loss_rows", _scale(i, 1.003))


def test_correct_flag_flipped(case):
    lg = case[1]["logits"]
    top = lg.topk(2, 1).values
    i = int((top[:, 0] - top[:, 1]).argsort()[B // 2])  # a row with the median top-2 gap

    def flip(t):
        t[i] = 1.0 - t[i]

    _named(case, "correct_rows", flip)


def test_oracle_matches_autograd_in_fp64():
    """The hand-written backward is the gradient of the model: fp32 mode against torch autograd on
    models.mnist_cnn.conv_net in fp64, with a dropout mask."""
    from tensorflow_distributed_amd.models import mnist_cnn as M

    params, x, y = O.random_case(5, 0.05, 2)
    mask = M.native_dropout_mask(5, 0, 0, 1234, 0.75)
    ref = O.oracle_step(params, x, y, "fp32", 0.75, mask)
    p = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    logits = M.conv_net(x.double(), p, 0.75, dropout_mask=mask.double())
    rows = torch.nn.functional.cross_entropy(logits, y.long(), reduction="none")
    rows.mean().backward()
    assert (rows.detach() - ref["loss_rows"]).abs().max() < 1e-12
    for k in p:
        assert (p[k].grad - ref["grads"][k]).norm() <= 1e-12 * p[k].grad.norm(), k


def test_max_batch_is_exported_and_enforced_before_any_device_work():
    """mnist_max_batch() comes from the launches' own constants: dlogits [B][10] + [4][64][10] partials
    in 160 KiB of LDS. The constructor checks it first, so the refusal needs no GPU."""
    from tensorflow_distributed_amd import _native

    _native.require()
    mx = int(torch.ops.tfd.mnist_max_batch())
    assert mx == (160 * 1024 // 4 - 4 * 64 * 10) // 10 == 3840
    with pytest.raises(RuntimeError, match="3840"):
        torch.classes.tfd.MnistEngine(mx + 1, 0, 1.0, 1234, 0)


def test_integer_case_is_exact_and_has_ties():
    """The integer recipe's premises, on the oracle: every forward value integral and <= 256 (exact in
    bf16), both precisions identical, a top-logit tie and positive pool ties at B = 5 and B = 37."""
    for Bi in (5, 37):
        params, x, y = O.integer_case(Bi)
        r = O.oracle_step(params, x, y, "bf16", backward=False)
        r32 = O.oracle_step(params, x, y, "fp32", backward=False)
        for k in ("pool1", "pool2", "hidden", "logits"):
            assert bool((r[k] == r[k].round()).all()) and r[k].abs().max() <= 256 and bool((r[k] == r32[k]).all()), k
        top = r["logits"].topk(2, 1).values
        assert int((top[:, 0] == top[:, 1]).sum()) >= 1
        for w in ("win1", "win2"):
            mx = r[w].max(-1).values
            assert int((((r[w] == mx[..., None]).sum(-1) > 1) & (mx > 0)).sum()) >= 1
