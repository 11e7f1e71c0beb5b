"""tools/check_isa.py on the compiled gfx950 kernels: no MFMA block of a K-loop waits for the loads issued just before it, and
the budgeted kernels keep their scratch size.

A slab of the K-loops (chol_tile, gemm_slabs) issues the buffer loads of the next slab, then multiplies the current one inside an
s_setprio 1 .. s_setprio 0 block.  With a run-time "is there a next slab" guard around the loads and the staging store the compiler
put s_waitcnt vmcnt(3) (2) (1) (0) in front of the k-steps of every other slab: the wave waited for the eight loads it had issued a
dozen instructions earlier.  The kernels stay correct and no functional test notices; this one reads the assembly."""
import importlib.util
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def isa():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("check_isa", ROOT / "tools" / "check_isa.py")
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(isa, tmp_path_factory):
    """assembly of the three kernel units, compiled side by side with the tool's flags"""
    td = tmp_path_factory.mktemp("isa")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    jobs = [(u, td / (u + ".s")) for u in isa.KERNEL_UNITS]
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(o),
                               str(ROOT / "autogp.jl_amd" / "csrc" / u)], stderr=subprocess.DEVNULL) for u, o in jobs]
    assert all(p.wait() == 0 for p in procs), "compilation failed"
    return {u: o.read_text() for u, o in jobs}


def test_rule_flags_a_wait_on_fresh_loads(isa):
    """the rule itself, on hand-written blocks: eight loads after the barrier, then vmcnt(3) inside the priority block of a loop is a
    wait on five of them; vmcnt(8) is not; the same wait outside a loop, or with the loads in front of the barrier, is not either"""
    def kernel(wait, loop=True, loads_before_barrier=False):
        loads = ["\tbuffer_load_dwordx4 v[0:3], v9, s[0:3], 0 offen"] * 8
        head = ".LBB0_1:                                ; =>This Inner Loop Header: Depth=1" if loop else ".LBB0_1:"
        body = (loads if loads_before_barrier else []) + ["\ts_barrier"] + ([] if loads_before_barrier else loads)
        return "\n".join(["_Z1kv:", head] + body + ["\ts_setprio 1", f"\ts_waitcnt vmcnt({wait}) lgkmcnt(3)", "\tv_mfma_f64_16x16x4_f64 v[0:7], v[8:9], v[10:11], v[0:7]",
                                                    "\ts_setprio 0", "\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm"])
    assert isa.fresh_load_waits(kernel(3)) == {"_Z1kv": [3]}
    assert isa.fresh_load_waits(kernel(7)) == {"_Z1kv": [7]}
    assert isa.fresh_load_waits(kernel(8)) == {}
    assert isa.fresh_load_waits(kernel(3, loop=False)) == {}
    assert isa.fresh_load_waits(kernel(3, loads_before_barrier=True)) == {}


def test_rule_follows_branches(isa):
    """loads in a skipped-over block still count (the run-time guard of the old loop), and a block entered by a jump takes the
    count of the block that jumps, not of the one laid out in front of it"""
    loads = ["\tbuffer_load_dwordx4 v[0:3], v9, s[0:3], 0 offen"] * 4
    guarded = "\n".join(["_Z1gv:", ".LBB1_1:                                ; =>This Inner Loop Header: Depth=1", "\ts_barrier", "\ts_cbranch_scc1 .LBB1_3",
                         "; %bb.2:                                ;   in Loop: Header=BB1_1 Depth=1"] + loads +
                        [".LBB1_3:                                ;   in Loop: Header=BB1_1 Depth=1", "\ts_setprio 1", "\ts_waitcnt vmcnt(1)", "\ts_setprio 0",
                         "\ts_cbranch_scc1 .LBB1_1", "\ts_endpgm"])
    assert isa.fresh_load_waits(guarded) == {"_Z1gv": [1]}
    jumped = "\n".join(["_Z1jv:", ".LBB2_1:                                ; =>This Inner Loop Header: Depth=1", "\ts_barrier", "\ts_branch .LBB2_3",
                        ".LBB2_2:                                ;   in Loop: Header=BB2_1 Depth=1"] + loads + ["\ts_branch .LBB2_1",
                        ".LBB2_3:                                ;   in Loop: Header=BB2_1 Depth=1", "\ts_setprio 1", "\ts_waitcnt vmcnt(1)", "\ts_setprio 0",
                        "\ts_cbranch_scc1 .LBB2_2", "\ts_endpgm"])
    assert isa.fresh_load_waits(jumped) == {}


def test_no_mfma_block_waits_on_fresh_loads(isa, asm):
    offenders = {}
    for u, txt in asm.items():
        offenders.update(isa.fresh_load_waits(txt))
    assert not offenders, "\n".join(f"{k}: vmcnt {v}" for k, v in offenders.items())


def test_the_k_loops_are_seen(isa, asm):
    """the rule has something to look at: the kernels of the slab loops carry priority blocks inside loops"""
    for u, frag in (("agp_kernels.hip", "k_chol_updateILb1ELi4ELb1ELi2ELi2E"), ("agp_kernels_flow.hip", "k_chol_flowILi4ELi2E"),
                    ("agp_kernels_grad.hip", "k_kinv_tiles"), ("agp_kernels_grad.hip", "k_trtri_chainILb1E")):
        txt = asm[u]
        lines = txt.split("\n")
        start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and frag in l.split(":")[0])
        body = lines[start:]
        body = body[:next(i for i, l in enumerate(body) if "s_endpgm" in l)]
        assert sum("s_setprio 1" in l for l in body) >= 2 and any("Loop Header" in l for l in body), frag


def test_scratch_budgets_hold(isa, asm):
    over, seen = [], set()
    for txt in asm.values():
        for k, v in isa.scratch_bytes(txt).items():
            for frag, lim in isa.SCRATCH_BUDGET.items():
                if frag in k:
                    seen.add(frag)
                    if v > lim:
                        over.append(f"{k}: {v} B of scratch (budget {lim})")
    assert seen == set(isa.SCRATCH_BUDGET), set(isa.SCRATCH_BUDGET) - seen
    assert not over, "\n".join(over)
