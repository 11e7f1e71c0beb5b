"""Static check of the compiled kernels (gfx950 ISA): no buffer load / store may sit in a "waterfall" loop — the
readfirstlane / compare / s_and_saveexec loop the compiler wraps around a buffer access whose resource descriptor it takes for
lane-dependent.  The operand streams of every K-loop are raw buffer loads with the descriptor in SGPRs; when an index the
descriptor is built from stops being provably wave-uniform the kernels stay correct and silently lose ~10 % (seen once: the
sub-diagonal kernel's slab loop, 31.1 -> 34.1 us per block column).  Nor may an MFMA block of a K-loop wait for the loads issued
just before it (fresh_load_waits), the budgeted kernels keep their scratch size, and no loop of the tile builder waits for a
program byte from global memory (decode_waits).   python tools/check_isa.py  -> exit status 0 / 1"""
import re, shutil, subprocess, sys, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent


def waterfalled_accesses(asm_text):
    bad = {}
    cur = None
    lines = asm_text.split("\n")
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
        if cur and ("buffer_load" in l or "buffer_store" in l) and any("s_and_saveexec" in x for x in lines[max(0, i - 3):i]):
            bad[cur] = bad.get(cur, 0) + 1
        if "s_endpgm" in l:
            cur = None
    return bad


def fresh_load_waits(asm_text):
    """MFMA blocks (s_setprio 1 ... s_setprio 0) inside a loop that wait on a load just issued: {kernel: [vmcnt values]}.
    A K-loop slab issues the buffer loads of the NEXT slab after the barrier and multiplies the current one inside the priority
    block; vmcnt counts loads still allowed in flight, oldest retired first, so an s_waitcnt vmcnt(N) in the block with N smaller
    than the number of buffer loads issued since the preceding s_barrier blocks on some of those — the prefetch is exposed.
    "Since the preceding s_barrier" follows the control flow, not the layout (the dataflow kernel's flag polls sit between one
    slab's code and the next one's, its barrier elsewhere): the count entering a basic block is the largest any predecessor leaves.
    "Inside a loop" is the compiler's own `in Loop:` / `Loop Header:` annotation of the block that holds the s_setprio 1."""
    bad = {}
    cur, body = None, []
    for l in asm_text.split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur, body = m.group(1), []
        elif cur is not None:
            body.append(l)
            if l.split(";")[0].strip() == "s_endpgm":
                w = _kernel_fresh_load_waits(body)
                if w:
                    bad[cur] = w
                cur = None
    return bad


def _kernel_fresh_load_waits(lines):
    # basic blocks: [label, in_loop of each instruction's block, instructions, successors]
    blocks, index = [], {}
    def new_block(label):
        blocks.append({"label": label, "ins": [], "succ": [], "fall": True})
        if label:
            index[label] = len(blocks) - 1
    new_block(None)
    in_loop = False
    for l in lines:
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            new_block(m.group(1)); in_loop = "Loop" in l
            continue
        if l.startswith("; %bb."):
            in_loop = "Loop" in l
            continue
        if l.startswith(";") and "Loop" in l and not blocks[-1]["ins"]:
            in_loop = True                      # continuation lines of a loop header's annotation
            continue
        ins = l.split(";")[0].split()
        if not ins:
            continue
        blocks[-1]["ins"].append((ins, in_loop, l))
        if ins[0].startswith("s_cbranch") or ins[0] == "s_branch":
            blocks[-1]["succ"].append(ins[1])
            blocks[-1]["fall"] = ins[0] != "s_branch"
            new_block(None)
    entry = [0] * len(blocks)                   # buffer loads issued since the last barrier, on entry (largest over predecessors)
    def run(i, report):
        fresh, block_fresh = entry[i], None
        for ins, loop, l in blocks[i]["ins"]:
            op = ins[0]
            if op == "s_barrier":
                fresh = 0
            elif op.startswith("buffer_load"):
                fresh = min(fresh + 1, 64)
            elif op == "s_setprio":
                block_fresh = fresh if (ins[1] == "1" and loop) else None
            elif op == "s_waitcnt" and block_fresh is not None and report is not None:
                m = re.search(r"vmcnt\((\d+)\)", l)
                if m and int(m.group(1)) < block_fresh:
                    report.append(int(m.group(1)))
        return fresh
    work = list(range(len(blocks)))
    while work:
        i = work.pop()
        out = run(i, None)
        succ = [index[s] for s in blocks[i]["succ"] if s in index]
        if blocks[i]["fall"] and i + 1 < len(blocks):
            succ.append(i + 1)
        for s in succ:
            if out > entry[s]:
                entry[s] = out; work.append(s)
    report = []
    for i in range(len(blocks)):
        run(i, report)
    return report


def decode_waits(asm_text, kernel_frag="k_cov_tiles"):
    """Loops of the tile builder that wait for an opcode from global memory: {kernel: count}.
    k_cov_tiles walks a particle's program once per pass, 16 times per tile.  Fetching each opcode with a global_load_ubyte and
    waiting for it (s_waitcnt vmcnt(0)) before the scalar dispatch — and then once more for the parameters — put two exposed L2 round
    trips on every node of every pass; the kernel stages the program in LDS once per tile instead.  Counted: a global_load_ubyte
    inside a loop (the compiler's `in Loop:` / `Loop Header:` annotation) that an s_waitcnt vmcnt(0) of the same loop follows.  Wider
    loads (the log|dt| table values of programs that use it, rank tables read in place) are not program bytes and may stay."""
    bad = {}
    cur, in_loop, pending = None, False, False
    for l in asm_text.split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1) if kernel_frag in m.group(1) else None
            in_loop = pending = False
            continue
        if cur is None:
            continue
        if re.match(r"^\.LBB\w+:", l) or l.startswith("; %bb."):
            in_loop = "Loop" in l
            pending = pending and in_loop
            continue
        ins = l.split(";")[0].split()
        if not ins:
            continue
        if ins[0] == "s_endpgm":
            cur = None
        elif in_loop and ins[0] == "global_load_ubyte":
            pending = True
        elif in_loop and pending and ins[0] == "s_waitcnt" and re.search(r"vmcnt\(0\)", l):
            bad[cur] = bad.get(cur, 0) + 1
            pending = False
    return bad


KERNEL_UNITS = ("agp_kernels.hip", "agp_kernels_flow.hip", "agp_kernels_grad.hip")
# scratch (spilled registers) budget in bytes per kernel: the K-loops of the large-population kernels must not spill at all; the
# dataflow kernel carries both tile bodies and a few hoisted constants (88 - 96 B); a rewrite of the diagonal K-loop once took it
# to 376 B — and the 64-particle share from 3.8 to 4.1 ms — without a single test noticing
SCRATCH_BUDGET = {"k_chol_updateILb1ELi4ELb1ELi2ELi2E": 0, "k_chol_updateILb1ELi4ELb1ELi2ELi1E": 0, "k_chol_updateILb1ELi4ELb1ELi2ELi0E": 0,
                  "k_chol_diagILi4ELi2E": 64, "k_chol_flowILi4ELi2E": 128, "k_chol_flowILi4ELi1E": 160, "k_chol_flowILi4ELi0E": 128}


def scratch_bytes(asm_text):
    out = {}
    cur = None
    for l in asm_text.split("\n"):
        m = re.match(r"^\s+\.amdhsa_kernel (_Z\w+)", l)
        if m:
            cur = m.group(1)
        m = re.match(r"^\s+\.amdhsa_private_segment_fixed_size (\d+)", l)
        if m and cur:
            out[cur] = int(m.group(1)); cur = None
    return out


def main():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    bad, over, waits, decode, n_kernels = {}, [], {}, {}, 0
    with tempfile.TemporaryDirectory() as td:
        jobs = []
        for u in KERNEL_UNITS:
            out = Path(td) / (u + ".s")
            jobs.append((out, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                                                str(ROOT / "autogp.jl_amd" / "csrc" / u)], stderr=subprocess.DEVNULL)))
        for out, pr in jobs:
            if pr.wait() != 0:
                print("compilation failed:", out.name); return 1
            txt = out.read_text()
            bad.update(waterfalled_accesses(txt))
            waits.update(fresh_load_waits(txt))
            decode.update(decode_waits(txt))
            sb = scratch_bytes(txt)
            n_kernels += len(sb)
            for k, v in sb.items():
                for frag, lim in SCRATCH_BUDGET.items():
                    if frag in k and v > lim:
                        over.append(f"{k}: {v} B of scratch (budget {lim})")
    for k, v in bad.items():
        print(f"{v} buffer accesses inside waterfall loops: {k}")
    for o in over:
        print("register spills over budget:", o)
    for k, v in waits.items():
        print(f"MFMA block waits on loads just issued (vmcnt {' '.join(map(str, v))}): {k}")
    for k, v in decode.items():
        print(f"{v} loops wait for an opcode from global memory: {k}")
    if bad or over or waits or decode:
        return 1
    print(f"no buffer access inside a waterfall loop, no MFMA block waiting on a fresh load, no opcode fetched from global memory in a loop of the tile builder, spills within budget ({n_kernels} kernels of {', '.join(KERNEL_UNITS)})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
