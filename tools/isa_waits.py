"""Where do a kernel's prologue loads get waited for? Compiles a HIP source for gfx950 with
--save-temps (into a scratch directory) and prints, per kernel, the instruction stream up to its
first MFMA (or the first N lines) reduced to vector loads (global / buffer / LDS-DMA), s_waitcnt
vmcnt, barriers and branches, so a wait issued in the middle of a load batch -- an exec-masked load
merged by a phi, a hoisted compare, a dependent index chain -- shows up before any timing run.
(The round-6 MNIST finds: docs/DESIGN.md §8.)

    python tools/isa_waits.py csrc/kernels/mnist.hip [--kernel fc1_fwd] [--lines 400]
    python tools/isa_waits.py csrc/kernels/mnist.hip --masked   # per kernel: exec-masked loads that wait
                                                               # inside their branch (each a serial round trip)
    python tools/isa_waits.py csrc/kernels/mnist.hip --scalar   # also the scalar side of the prologue: s_load /
                                                               # s_buffer_load and s_waitcnt lgkmcnt, and per kernel
                                                               # the lgkmcnt waits in front of its first load batch

--scalar is about the kernel-argument chain (docs/DESIGN.md §8c): a wave forms its first vector address
only after the scalar loads of its pointers have come back, and every s_waitcnt lgkmcnt in front of the
first vector load batch is one more serial round trip to the argument segment. The files of
PRELOAD_SOURCES are compiled as the build compiles them, with kernel-argument preload; the fallback
prologue the compiler keeps for firmware without preload (the 256 bytes in front of the real entry) is
not part of the listing.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-fPIC", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-D__HIP_PLATFORM_AMD__=1",
         "-ffp-contract=fast", "-munsafe-fp-atomics", "-Wno-unused-result", "-Xclang", "-target-feature", "-Xclang",
         "-packed-fp32-ops", "--save-temps"]
KEEP = re.compile(r"^\s*(global_load|buffer_load|global_load_lds|s_waitcnt vmcnt|s_barrier|s_cbranch|v_mfma)")
KEEP_SCALAR = re.compile(r"^\s*(global_load|buffer_load|global_load_lds|s_load_|s_buffer_load_|s_waitcnt|s_barrier|s_cbranch|"
                         r"v_mfma)")
VLOAD = re.compile(r"^\s*(global_load|buffer_load)")
# Kernel-argument preload (gfx950: leading pointer / scalar kernel parameters arrive in user SGPRs at
# wave launch). Mirrors tensorflow_distributed_amd/_build.py: the same flags for the same files.
PRELOAD_FLAGS = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
PRELOAD_SOURCES = ("mnist.hip", "mnist_tail_sched.hip", "mnist_tail_ema.hip", "kernarg_probe.hip")


def flags_for(src):
    return FLAGS + (PRELOAD_FLAGS if os.path.basename(src) in PRELOAD_SOURCES else [])


def compile_asm(src):
    """the gfx950 assembly of `src` compiled with the build's flags, as a list of lines"""
    src = os.path.abspath(src)
    with tempfile.TemporaryDirectory() as d:
        cmd = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"), *flags_for(src), "-I",
               os.path.join(ROOT, "csrc"), "-c", src, "-o", os.path.join(d, "k.o")]
        p = subprocess.run(cmd, cwd=d, capture_output=True, text=True)
        if p.returncode:
            sys.exit(p.stderr[-2000:])
        return open(glob.glob(os.path.join(d, "*gfx950*.s"))[0]).read().splitlines()


def kernel_bodies(asm):
    """{mangled name: the kernel's lines}, without the no-preload fallback prologue"""
    out = {}
    starts = [i for i, ln in enumerate(asm) if re.match(r"^_Z\S+:\s", ln)]
    for s in starts:
        end = next((j for j in range(s + 1, len(asm)) if asm[j].startswith(".Lfunc_end")), len(asm))
        body = asm[s + 1:end]
        # fallback prologue: s_load of the preloaded dwords, wait, s_branch over the padding to +256 B
        br = next((j for j, ln in enumerate(body[:40]) if ln.strip().startswith("s_branch")), None)
        if br is not None and br + 1 < len(body) and ".p2align" in body[br + 1]:
            body = body[br + 2:]
        out[asm[s].split(":")[0]] = body
    return out


def preload_lengths(asm):
    """{mangled name: .amdhsa_user_sgpr_kernarg_preload_length} (dwords granted by the compiler)"""
    out, cur = {}, None
    for ln in asm:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.match(r"^\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", ln)
        if m and cur:
            out[cur] = int(m.group(1))
    return out


def scalar_waits(body, lines=600):
    """(lgkmcnt waits before the first vector load, before the last vector load of the first batch,
    vector loads in that batch). The first batch ends at the first s_waitcnt vmcnt behind a vector load
    (or at the first MFMA)."""
    mf = next((j for j, ln in enumerate(body) if "v_mfma" in ln), None)
    stop = mf if mf is not None else min(len(body), lines)
    waits = nload = 0
    before_first = before_last = None
    for ln in body[:stop]:
        t = ln.strip()
        if VLOAD.match(ln):
            if before_first is None:
                before_first = waits
            before_last = waits
            nload += 1
        elif t.startswith("s_waitcnt"):
            if "vmcnt" in t and nload:
                break
            if "lgkmcnt" in t:
                waits += 1
    return before_first, before_last, nload


def _sregs(tok):
    m = re.match(r"^s\[(\d+):(\d+)\]$", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^s(\d+)$", tok)
    return [int(m.group(1))] if m else []


def path_waits(body, cap=8):
    """The scalar side of a kernel's prologue per ROLE instead of in listing order (a kernel whose
    blocks or waves take different roles, or with a fallback chain behind a branch, has no meaningful
    listing order). Walks the control-flow paths from the entry; a path ends with its first vector load
    batch (at the first s_waitcnt vmcnt behind a vector load, the first MFMA or the end of the program).
    Paths are grouped by the vector load they reach first -- one group per role -- and each group reports
    its BEST path, with the worst one beside it (worst_batch_arg / worst_batch_all). The best path is the
    figure to hold a kernel to because the walk cannot tell which paths a wave can take: structurised
    control flow joins a role's code to code that only other blocks run (the optimizer tail's fc-region
    loads are reachable, on paper, through the `*step += 1` of the launch that has no fc-region blocks, and
    through a conv-region wave's LDS reduction), and every such path would be charged to the role. The
    minimum errs the other way only if a role's every real path is longer than an impossible one to the same
    load; the worst figure is printed so that a reader sees when the two differ and can read the listing.
    Returns {first-load index: dict} with
        load        the instruction text
        first_arg   ARGUMENT waits before that first load
        first_all   lgkmcnt waits of any kind before it
        batch_arg   argument waits before the LAST vector load of the batch
        batch_all   lgkmcnt waits of any kind before it
        arg_waits_at  instruction indices of the batch's argument waits
        batch_loads   the vector loads of the batch, in order (what tells one role from another)
        worst_batch_arg, worst_batch_all   the same two batch figures on the longest path to that load
    An ARGUMENT wait is an s_waitcnt lgkmcnt with a scalar load of the kernel-argument segment
    outstanding (base s[0:1], a copy of it, or s[0:1] plus a constant): one serial round trip to the
    argument segment. A wait for a scalar load through a device pointer (*step, the rows[B] tag, t) or
    for LDS only counts in the _all figures; a wait with no scalar load or LDS operation outstanding
    counts nowhere. A wait instruction counts once per path however often a loop runs it; a path ends
    after `cap` of them."""
    ins, label_at = [], {}
    for ln in body:
        t = ln.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            label_at[m.group(1)] = len(ins)
        elif t and not t.startswith(".") and not t.endswith(":"):
            ins.append(t)
    sites, worst, seen = {}, {}, set()
    # state: pc, kernarg aliases, low halves of a pointer + constant under way, argument load outstanding,
    # wait instructions met (all, argument), first load (index, counts there), counts at the last load
    stack = [(0, frozenset({(0, 1)}), frozenset(), (False, False), frozenset(), frozenset(), None, None)]
    while stack:
        pc, al, lows, (pend, busy), wall, warg, first, last = stack.pop()
        alive = True
        while alive and pc < len(ins):
            t = ins[pc]
            op, _, rest = t.partition(" ")
            ops = [x.strip() for x in re.split(r",(?![^\[]*\])", rest)] if rest.strip() else []
            if VLOAD.match(t):
                last = (len(warg), len(wall), tuple(sorted(warg)), (last[3] if last else ()) + (pc,))
                if first is None:
                    first = (pc,) + last[:2]
            elif op == "s_waitcnt":
                if "vmcnt" in t and first is not None:
                    break
                if "lgkmcnt" in t:
                    if busy:  # (a wait with nothing outstanding costs nothing)
                        wall = wall | {pc}
                    if pend:
                        warg = warg | {pc}
                    if "lgkmcnt(0)" in t:
                        pend = busy = False
                    if len(wall) >= cap:
                        break
            elif op.startswith("v_mfma") or op == "s_endpgm":
                break
            elif op.startswith(("s_load_", "s_buffer_load_")):
                busy = True
                if len(ops) > 1 and tuple(_sregs(ops[1])) in al:
                    pend = True
            elif op.startswith("ds_"):
                busy = True
            # SGPR definitions: copies of the kernarg pointer, pointer + constant, and what overwrites them
            dst = [] if not ops or op.startswith(("s_cmp", "s_cbranch", "s_branch", "s_bitcmp", "s_waitcnt", "s_barrier",
                                                  "s_nop")) else _sregs(ops[0])
            if dst and op.startswith(("s_", "v_readfirstlane", "v_readlane", "v_cmp")):
                src = [tuple(_sregs(o)) for o in ops[1:]]
                add = None
                if op == "s_mov_b64" and src and src[0] in al:
                    add = tuple(dst)
                elif op == "s_add_u32" and src and len(src[0]) == 1 and any(src[0][0] == pr[0] for pr in al):
                    lows = lows | {(dst[0], next(pr[1] for pr in al if pr[0] == src[0][0]))}
                    dst = []
                elif op == "s_addc_u32" and src and len(src[0]) == 1 and (dst[0] - 1, src[0][0]) in lows:
                    add = (dst[0] - 1, dst[0])
                    dst = []
                al = frozenset(pr for pr in al if not set(pr) & set(dst))
                lows = frozenset(x for x in lows if x[0] not in dst)
                if add:
                    al = al | {add}
            nxt = [pc + 1]
            if op == "s_branch":
                nxt = [label_at.get(ops[0], len(ins))]
            elif op.startswith("s_cbranch"):
                nxt = [label_at.get(ops[0], len(ins)), pc + 1]
            if len(nxt) > 1 or op == "s_branch":
                keys = [(n, al, lows, (pend, busy), wall, warg, first, last) for n in nxt]
                keys = [k for k in keys if k not in seen]
                seen.update(keys)
                stack.extend(keys[:-1])
                if not keys:
                    alive = False
                else:
                    pc = keys[-1][0]
                continue
            pc += 1
        if alive and first is not None:
            rec = (first[1], last[0], first[2], last[1], last[2], last[3])
            if first[0] not in sites or rec < sites[first[0]][0]:
                sites[first[0]] = (rec, ins[first[0]])
            w = worst.get(first[0], (0, 0))
            worst[first[0]] = (max(w[0], last[0]), max(w[1], last[1]))
    return {pc: {"load": ld, "first_arg": r[0], "batch_arg": r[1], "first_all": r[2], "batch_all": r[3],
                 "arg_waits_at": list(r[4]), "batch_loads": [ins[i] for i in r[5]], "worst_batch_arg": worst[pc][0], "worst_batch_all": worst[pc][1]}
            for pc, (r, ld) in sorted(sites.items())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("--kernel", default="", help="substring of the kernel's mangled name")
    ap.add_argument("--lines", type=int, default=600, help="asm lines scanned per kernel when it has no MFMA")
    ap.add_argument("--masked", action="store_true", help="count exec-masked branches (s_and_saveexec ... s_or_b64 exec)"
                    " that hold a load AND a wait: the conv1 weight reads of round 6 were ten of these in a row")
    ap.add_argument("--scalar", action="store_true", help="also list s_load / s_buffer_load and s_waitcnt lgkmcnt, "
                    "and report per kernel the lgkmcnt waits in front of the first vector load batch")
    a = ap.parse_args(argv)
    asm = compile_asm(a.src)
    if a.masked:
        return masked_waits(asm, a.kernel)
    if a.scalar:
        return scalar_listing(asm, a.kernel, a.lines)
    starts = [i for i, ln in enumerate(asm) if re.match(r"^_Z\S+:", ln) and "GLOBAL__N" in ln or
              re.match(r"^_Z\S+:\s", ln)]
    for s in starts:
        name = asm[s].split(":")[0]
        if a.kernel and a.kernel not in name:
            continue
        end = next((j for j in range(s + 1, len(asm)) if asm[j].strip().startswith("s_endpgm")), len(asm))
        body = asm[s + 1:end]
        mf = next((j for j, ln in enumerate(body) if "v_mfma" in ln), None)
        stop = mf + 1 if mf is not None else min(len(body), a.lines)
        loads = 0
        print(f"== {name}  ({end - s} lines; first MFMA at +{mf})")
        for j, ln in enumerate(body[:stop]):
            if not KEEP.match(ln):
                continue
            t = ln.strip()
            if "load" in t.split()[0]:
                loads += 1
            print(f"  +{j:5d} [{loads:3d} loads] {t[:90]}")


def scalar_listing(asm, kernel="", lines=600):
    pre = preload_lengths(asm)
    for name, body in kernel_bodies(asm).items():
        if kernel and kernel not in name:
            continue
        mf = next((j for j, ln in enumerate(body) if "v_mfma" in ln), None)
        stop = mf + 1 if mf is not None else min(len(body), lines)
        first, last, nload = scalar_waits(body, lines)
        print(f"== {name}  (first MFMA at +{mf}; kernarg preload {pre.get(name, 0)} dwords)")
        print(f"   in listing order: lgkmcnt waits before the first vector load: {first}; before the last load of the "
              f"first batch ({nload} loads): {last}")
        for pc, r in path_waits(body).items():
            print(f"   role at +{pc:5d}: argument waits before its first vector load {r['first_arg']}, before the last load "
                  f"of that batch {r['batch_arg']}  (lgkmcnt waits of any kind: {r['first_all']}, {r['batch_all']}; longest path: "
                  f"{r['worst_batch_arg']}, {r['worst_batch_all']})  "
                  f"{r['load'][:50]}  argument waits at {r['arg_waits_at']}")
        loads = 0
        for j, ln in enumerate(body[:stop]):
            if not KEEP_SCALAR.match(ln):
                continue
            t = ln.strip()
            if VLOAD.match(ln):
                loads += 1
            print(f"  +{j:5d} [{loads:3d} loads] {t[:90]}")


def masked_waits(asm, kernel=""):
    cur, counts = None, {}
    for i, ln in enumerate(asm):
        m = re.match(r"^(_Z\S+):", ln)
        if m:
            cur = m.group(1)
        if cur is None or "s_and_saveexec" not in ln or (kernel and kernel not in cur):
            continue
        blk = asm[i:i + 12]
        end = next((j for j, b in enumerate(blk) if "s_or_b64 exec" in b), None)
        if end is None:
            continue
        inner = "\n".join(blk[:end])
        if re.search(r"ds_read|global_load|buffer_load", inner) and "s_waitcnt" in inner:
            counts[cur] = counts.get(cur, 0) + 1
    for k, v in sorted(counts.items(), key=lambda x: -x[1]):
        print(f"{v:4d}  {k}")


if __name__ == "__main__":
    main()
