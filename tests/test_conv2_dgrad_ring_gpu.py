"""The conv2 dgrad's W2 ring (csrc/kernels/mnist.hip, conv2_dgrad_body): LDS-DMA'd tap groups that the
compiler's wait insertion does not see. A ring can go wrong in three ways -- a slot read before its DMA
landed, a slot overwritten before its last reader, a group-to-tap mapping off by one -- and each shows in
the conv1 weight-gradient slabs the dgrad blocks write (dX never leaves the block):

* bit identity with the resident-W2 form of the same launch (all 25 taps in LDS before the first MFMA, one
  block per CU, no ring), at B = 1, 2, 3, 5, over seeds, repeated eager launches and graph replays;
* tap-distinct small-integer weights, for which every sum is exact: equality with an fp64 host convolution,
  and on a mismatch the conv2 taps whose removal (or exchange) would explain it;
* no slot carries data from one launch to the next: a second W2 in the same engine gives what a fresh
  process computes for it.
"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
OFF_WC2, N_WC2 = 832, 25 * 32 * 64


def _engine(B):
    from tensorflow_distributed_amd import _native
    _native.require()
    eng = torch.classes.tfd.MnistEngine(B, 0, 1.0, 1, 0)
    eng.set_adam(0.01, 0.9, 0.999, 1e-8)
    return eng


def _inputs(B, seed, integer=False):
    """dz2, W2 (HWIO [5,5,32,64]), x, the conv1 relu outputs and their pool argmax, on the host"""
    g = torch.Generator().manual_seed(seed)
    if integer:
        # |W2| <= 8 and |dz2| <= 4, dz2 sparse so the tail's sums stay far below 2^24 (checked by the test)
        w2 = torch.randint(-8, 9, (5, 5, 32, 64), generator=g).float()
        dz2 = torch.randint(-4, 5, (B, 14, 14, 64), generator=g).float() * (torch.rand(B, 14, 14, 64, generator=g) < 0.1)
        x = torch.randint(0, 3, (B, 784), generator=g).float()
    else:
        w2 = torch.randn(5, 5, 32, 64, generator=g) * 0.05
        dz2 = torch.randn(B, 14, 14, 64, generator=g) * 0.1
        x = torch.rand(B, 784, generator=g)
    p1 = torch.rand(B, 14, 14, 32, generator=g) * (torch.rand(B, 14, 14, 32, generator=g) < 0.6)
    idx1 = torch.randint(0, 4, (B, 14, 14, 32), generator=g, dtype=torch.uint8)
    return dz2.bfloat16(), w2.bfloat16(), x, p1.bfloat16(), idx1


def _load(eng, w2, x, p1, idx1):
    eng.params_bf16()[OFF_WC2:OFF_WC2 + N_WC2].copy_(w2.reshape(-1).cuda())
    eng.feed_x().copy_(x.cuda())
    eng.pool1().view(-1).copy_(p1.reshape(-1).cuda())
    eng.pool1_argmax().view(-1).copy_(idx1.reshape(-1).cuda())


def _run(eng, dz2_dev, resident):
    """one conv2 backward launch on poisoned slabs -> copies of (wg1 slabs, wg2 slabs)"""
    s1, s2 = eng.conv_grad_slabs()
    s1.fill_(float("nan"))
    s2.fill_(float("nan"))
    eng.conv2_bwd_debug(dz2_dev, resident)
    return s1.clone(), s2.clone()


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_ring_is_bit_identical_to_resident_w2(B):
    eng = _engine(B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for seed in range(3):
            dz2, w2, x, p1, idx1 = _inputs(B, 100 * B + seed)
            _load(eng, w2, x, p1, idx1)
            dz2 = dz2.cuda()
            ref1, ref2 = _run(eng, dz2, True)
            assert torch.isfinite(ref1).all().item() and torch.isfinite(ref2).all().item()
            got = [_run(eng, dz2, False) for _ in range(20)]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = _run(eng, dz2, False)
            for _ in range(20):
                graph.replay()
                got.append((out[0].clone(), out[1].clone()))
            s.synchronize()
            for i, (g1, g2) in enumerate(got):
                kind = f"B={B} seed={seed} " + (f"eager launch {i}" if i < 20 else f"graph replay {i - 20}")
                assert torch.equal(g1, ref1), (kind, "conv1 weight-gradient slabs (dgrad blocks)",
                                               (g1 != ref1).any(dim=1).nonzero().flatten().tolist())
                assert torch.equal(g2, ref2), (kind, "conv2 weight-gradient slabs (wgrad blocks)")
            del graph


def _host_wg1(dz2, w2, x, p1, idx1):
    """fp64 host form of what the dgrad blocks write: [2B, 832] (block = image, row half; 25 taps + the
    bias row, 32 channels), and the largest sum of magnitudes behind any entry (the exactness bound)"""
    B = dz2.shape[0]
    d = dz2.double().permute(0, 3, 1, 2)                           # [B,64,14,14]
    wt = w2.double().permute(3, 2, 0, 1).contiguous()              # [co,ci,kh,kw]: conv2's filter
    dx = torch.nn.functional.conv_transpose2d(d, wt, padding=2)    # [B,32,14,14], exact in fp64
    dx = dx.permute(0, 2, 3, 1).float().bfloat16().double()        # the kernel rounds dX to bf16 once
    dx = dx * (p1.double() != 0)
    dz1 = torch.zeros(B, 28, 28, 32, dtype=torch.float64)
    bi, ih, iw, c = torch.meshgrid(torch.arange(B), torch.arange(14), torch.arange(14), torch.arange(32), indexing="ij")
    wi = idx1.long()
    dz1[bi, 2 * ih + (wi >> 1), 2 * iw + (wi & 1), c] = dx
    xp = torch.zeros(B, 32, 32, dtype=torch.float64)
    xp[:, 2:30, 2:30] = x.bfloat16().double().view(B, 28, 28)
    pat = xp.unfold(1, 5, 1).unfold(2, 5, 1)                       # [B,28,28,5,5]
    out = torch.zeros(2 * B, 832, dtype=torch.float64)
    mag = 0.0
    for b in range(B):
        for h in range(2):
            pp, zz = pat[b, 14 * h:14 * h + 14], dz1[b, 14 * h:14 * h + 14]
            out[2 * b + h, :800] = torch.einsum("yxkl,yxc->klc", pp, zz).reshape(-1)
            out[2 * b + h, 800:] = zz.sum(dim=(0, 1))
            mag = max(mag, torch.einsum("yxkl,yxc->klc", pp.abs(), zz.abs()).max().item(), zz.abs().sum(dim=(0, 1)).max().item())
    return out, mag


def test_tap_distinct_integer_weights_match_the_host_convolution():
    B = 2
    dz2, w2, x, p1, idx1 = _inputs(B, 7, integer=True)
    w2 = (w2.float() + (torch.arange(25).view(5, 5, 1, 1) % 3 - 1)).clamp(-8, 8).bfloat16()  # no two taps alike
    assert len({w2[t // 5, t % 5].float().numpy().tobytes() for t in range(25)}) == 25
    want, mag = _host_wg1(dz2, w2, x, p1, idx1)
    assert mag < 2 ** 24 and dz2.float().abs().max() <= 4 and w2.float().abs().max() <= 8, mag  # every fp32 sum exact
    eng = _engine(B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _load(eng, w2, x, p1, idx1)
        got = _run(eng, dz2.cuda(), False)[0]
    s.synchronize()
    got = got.cpu().double()
    if torch.equal(got, want):
        return
    # which conv2 tap explains the difference: its contribution missing, or read from another tap's slot
    blame = []
    for t in range(25):
        for u in [None] + [v for v in range(25) if v != t]:
            w = w2.clone()
            w[t // 5, t % 5] = 0 if u is None else w2[u // 5, u % 5]
            if torch.equal(_host_wg1(dz2, w, x, p1, idx1)[0], got):
                blame.append(f"tap {t} " + ("missing" if u is None else f"read as tap {u}"))
    bad = (got != want).any(dim=1).nonzero().flatten().tolist()
    raise AssertionError(f"conv1 weight-gradient slabs differ in blocks {bad}; explained by: {blame or 'no single tap'}")


_FRESH = """
import sys, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_conv2_dgrad_ring_gpu as T
B = 2
eng = T._engine(B)
dz2, w2, x, p1, idx1 = T._inputs(B, 12)
T._load(eng, w2, x, p1, idx1)
out = T._run(eng, dz2.cuda(), False)
torch.cuda.synchronize()
torch.save([o.cpu() for o in out], sys.argv[1])
"""


def test_second_w2_in_one_stream_equals_a_fresh_process(tmp_path):
    B = 2
    eng = _engine(B)
    dz2a, w2a, xa, p1a, idx1a = _inputs(B, 11)
    dz2b, w2b, xb, p1b, idx1b = _inputs(B, 12)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _load(eng, w2a, xa, p1a, idx1a)
        first = _run(eng, dz2a.cuda(), False)
        _load(eng, w2b, xb, p1b, idx1b)
        second = _run(eng, dz2b.cuda(), False)
    s.synchronize()
    assert not torch.equal(first[0], second[0])
    path = str(tmp_path / "fresh.pt")
    code = _FRESH.format(root=ROOT, tests=os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code, path], check=True, timeout=120)
    fresh = torch.load(path)
    assert torch.equal(second[0].cpu(), fresh[0]) and torch.equal(second[1].cpu(), fresh[1])
