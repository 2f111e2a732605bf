"""The step kernels' first loads wait for no kernel-argument fetch: what the built code says.

Every kernel of the one-GPU MNIST step used to take ``MnistStepArgs`` (about 300 bytes, five 64-byte
lines of the argument segment) by value alone: each wave began with scalar loads of its pointers and
an ``s_waitcnt lgkmcnt(0)`` before its first vector address existed, and some prologues had two or
three of those in a row. Measured on an MI355X, that fetch behind a kernel that streamed 90 MB costs
0.65 us more per kernel than pointers preloaded into SGPRs (profiles/kernarg_probe.log). The kernels now
take the pointers and B of their first load batch as leading parameters, compiled with kernel-argument
preload (docs/DESIGN.md section 8c).

This test compiles the three sources with the build's flags (tools/isa_waits.py mirrors
``_build.py``) and checks, for the five step kernels and the three instantiations of the optimizer
tail:

* the compiler granted a preload (``.amdhsa_user_sgpr_kernarg_preload_length`` > 0);
* the flags used here are the build's;
* in every ROLE of the kernel (tools/isa_waits.py ``path_waits``: the control-flow paths grouped by
  the vector load they reach first -- block roles such as fc1_bwd's dW / dX / output-layer blocks, wave
  roles such as conv12's W2 and x loaders) at most ONE ``s_waitcnt lgkmcnt`` of any kind precedes the end
  of the first vector load batch: what a prologue still reads from the segment is requested together;
* in the kernel's HOT roles NO wait of any kind for a scalar load precedes the first vector load. A hot
  role is named by its loads (HOT below), never by a count of clean roles: for the optimizer tail it is
  the bf16-gradient fc loop, the one the default step runs (p / gbf / m / v per lane, and t beside them).

An "argument wait" is an ``s_waitcnt lgkmcnt`` with a scalar load of the argument segment outstanding.
A wait for a device-indirect scalar (``*step``, the ``rows[B]`` tag, ``t``) is no argument fetch; those
loads stay beside the vector loads of their batch, never in front of its first load: the checks count
waits of every kind, and the tail's hot role must hold t's load INSIDE its first batch.

One kind of role is held to the argument-wait bound alone: a wave of the tail whose first vector load is t
itself (T_ONLY). Those are the gather blocks, an fc thread past the end, and a conv-region wave none of
whose lanes has a slab in range (2B or wg2_splits slabs, fewer than the 16 / 4 slab phases at a small
batch): that wave's first vector load comes behind the block's LDS reduction, and two of its three waits
are for LDS, not for a scalar load.
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no ROCm toolchain")

ALL = "every role"
T_LOAD = r"global_load_dwordx2 v\[\d+:\d+\], v\d+, s\["   # t: a uniform 8-byte load through an SGPR pointer
GBF_LOAD = r"global_load_dwordx2 v\[\d+:\d+\], v\[\d+:\d+\], off"  # the bf16 gradient: 8 bytes per lane


def _first(regex, nth=0):
    """the nth role, in program order, whose first vector load matches"""
    return lambda roles: [[pc for pc, r in roles.items() if re.match(regex, r["load"])][nth]]


def _tail_gbf_loop(roles):
    """the tail's bf16-gradient fc loop: three 16-byte operand loads, the 8-byte gradient and t in one batch"""
    return [pc for pc, r in roles.items()
            if sum(bool(re.match(r"global_load_dwordx4", x)) for x in r["batch_loads"]) == 3
            and any(re.match(GBF_LOAD, x) for x in r["batch_loads"])]


# kernel (substring of the mangled name) -> (source, the hot roles: ALL or selectors by load). Roles that are
# not hot, each with at most one wait in front of the end of its first batch:
#   fc1_bwd           the 17 output-layer blocks, whose first loads are 4- and 2-byte global loads (dlogits /
#                     hd are not among the 14 preloadable dwords: the dX and dW tiles, 996 of the launch's
#                     1013 blocks, take them)
#   conv2_bwd_lds     the wgrad role's second image (its first image's loads have no wait in front)
#   mnist_adam_kernel the conv-region blocks (slab pointers and counts from MnistStepArgs) and the conv-only
#                     launch's step bump
HOT = {
    "conv12_fwd_lds": ("mnist.hip", ALL),    # W2 loader waves, x / W1 loader waves
    "7fc1_fwd": ("mnist.hip", ALL),
    "head_kernel": ("mnist.hip", ALL),
    # dW tiles and dX alone (part 2): buffer loads to registers; dX tiles: the DMA ring
    "7fc1_bwd": ("mnist.hip", [_first(r"buffer_load_dwordx4 v\[", 0), _first(r"buffer_load_dwordx4 v\[", 1),
                               _first(r"buffer_load_dwordx4 v\d+, .* lds$")]),
    # dgrad blocks (LDS DMA), wgrad blocks (their first image)
    "conv2_bwd_lds": ("mnist.hip", [_first(r"global_load_lds_dwordx4"), _first(r"buffer_load_dwordx4", 0)]),
    "mnist_adam_kernelINS_14MnistAdamConst": ("mnist.hip", [_tail_gbf_loop]),   # 1024 of ~1240 blocks
    "mnist_adam_kernelINS_13MnistAdamArgs": ("mnist_tail_sched.hip", [_tail_gbf_loop]),
    "mnist_adam_kernelINS_16MnistAdamEmaArgs": ("mnist_tail_ema.hip", [_tail_gbf_loop]),
}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_waits", os.path.join(ROOT, "tools", "isa_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled():
    """{source: (preload lengths, kernel bodies)}: each source compiled once for the whole module"""
    W = _tool()
    out = {}
    for src in sorted({v[0] for v in HOT.values()}):
        asm = W.compile_asm(os.path.join(ROOT, "csrc", "kernels", src))
        out[src] = (W.preload_lengths(asm), W.kernel_bodies(asm), W)
    return out


def test_tool_mirrors_the_build_flags():
    from tensorflow_distributed_amd import _build

    W = _tool()
    assert list(W.PRELOAD_FLAGS) == list(_build.PRELOAD_FLAGS)
    assert set(W.PRELOAD_SOURCES) == set(_build.PRELOAD_SOURCES)
    assert {v[0] for v in HOT.values()} <= set(_build.PRELOAD_SOURCES)


@pytest.mark.parametrize("kernel", sorted(HOT))
def test_first_load_batch_waits_for_no_argument_fetch(compiled, kernel):
    src, hot = HOT[kernel]
    pre, bodies, W = compiled[src]
    names = [n for n in bodies if kernel in n]
    assert len(names) == 1, (kernel, names)
    name = names[0]
    assert pre.get(name, 0) > 0, f"{name}: no kernel-argument preload granted"
    roles = W.path_waits(bodies[name])
    assert roles, name
    for pc, r in roles.items():
        print(f"{kernel} +{pc}: {r}")
    tail = "mnist_adam_kernel" in kernel
    for pc, r in roles.items():
        assert r["batch_arg"] <= 1, f"{name} +{pc}: {r['batch_arg']} waits for the argument segment in a first batch: {r}"
        t_only = tail and len(r["batch_loads"]) == 1 and re.match(T_LOAD, r["load"])
        if not t_only:
            assert r["batch_all"] <= 1, f"{name} +{pc}: {r['batch_all']} scalar waits inside a first load batch: {r}"
    hot_pcs = sorted(roles) if hot == ALL else [pc for sel in hot for pc in sel(roles)]
    assert hot_pcs and len(set(hot_pcs)) == len(hot_pcs), (name, hot_pcs)
    for pc in hot_pcs:
        r = roles[pc]
        assert r["first_all"] == 0, f"{name} +{pc}: {r['first_all']} scalar waits in front of a hot role's first load: {r}"
    if tail:  # t beside the operand loads: in the hot role's first batch, and not its first load
        (pc,) = hot_pcs
        loads = roles[pc]["batch_loads"]
        assert any(re.match(T_LOAD, x) for x in loads[1:]) and not re.match(T_LOAD, loads[0]), loads


def test_probe_pair_differs_only_in_the_argument_path(compiled):
    """tools/debug/kernarg_probe.py rests on this: the struct form waits once for the argument segment in
    front of its load, the preloaded form not at all."""
    W = compiled["mnist.hip"][2]
    asm = W.compile_asm(os.path.join(ROOT, "csrc", "kernels", "kernarg_probe.hip"))
    pre, bodies = W.preload_lengths(asm), W.kernel_bodies(asm)
    got = {}
    for name, body in bodies.items():
        (r,) = W.path_waits(body).values()
        got["preload" if "preload" in name else "struct"] = (pre.get(name, 0), r["first_arg"], r["first_all"])
    assert got["struct"] == (0, 1, 1), got
    assert got["preload"][0] >= 4 and got["preload"][1:] == (0, 0), got
