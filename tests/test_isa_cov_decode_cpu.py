"""tools/check_isa.py, rule decode_waits, on the compiled tile builder: no loop of k_cov_tiles<4> / <8> waits for an opcode from
global memory.

The builder walks a particle's program once per pass, 16 passes per tile.  With opcodes and parameters behind plain global pointers
every node of every pass cost two exposed L2 round trips (global_load_ubyte -> s_waitcnt vmcnt(0) -> v_readfirstlane -> scalar
branch, then the parameters); the kernel stages one record per node in LDS once per tile (stage_node_records).  No functional test
notices when that is lost; this one reads the assembly."""
import importlib.util
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
KERNELS = ("_ZN3agp11k_cov_tilesILi4EEEvNS_7CovArgsE", "_ZN3agp11k_cov_tilesILi8EEEvNS_7CovArgsE")


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
    """assembly of the unit that holds k_cov_tiles, compiled with the tool's flags"""
    out = tmp_path_factory.mktemp("isa_cov") / "agp_kernels.s"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(out),
                    str(ROOT / "autogp.jl_amd" / "csrc" / "agp_kernels.hip")], stderr=subprocess.DEVNULL, check=True)
    return out.read_text()


def _kernel(body, name="_ZN3agp11k_cov_tilesILi4EEEvNS_7CovArgsE"):
    return "\n".join([name + ":"] + body + ["\ts_endpgm"])


LOOP = ".LBB0_1:                                ; =>This Inner Loop Header: Depth=1"
FETCH = ["\tglobal_load_ubyte v4, v[2:3], off", "\ts_waitcnt vmcnt(0)", "\tv_readfirstlane_b32 s4, v4"]


def test_rule_flags_an_opcode_fetch_in_a_loop(isa):
    """the rule itself, on hand-written blocks"""
    name = KERNELS[0]
    assert isa.decode_waits(_kernel([LOOP] + FETCH + ["\ts_cbranch_scc1 .LBB0_1"])) == {name: 1}
    # the same fetch in front of the loop (staging, the one-node fast path) is not a finding
    assert isa.decode_waits(_kernel(FETCH + [LOOP, "\tds_read_b128 v[0:3], v9", "\ts_waitcnt lgkmcnt(0)", "\ts_cbranch_scc1 .LBB0_1"])) == {}
    # wider loads inside the loop (table values) may stay, and so may a counted wait that leaves the byte in flight
    assert isa.decode_waits(_kernel([LOOP, "\tglobal_load_dwordx4 v[0:3], v[8:9], off", "\ts_waitcnt vmcnt(0)", "\ts_cbranch_scc1 .LBB0_1"])) == {}
    assert isa.decode_waits(_kernel([LOOP, "\tglobal_load_ubyte v4, v[2:3], off", "\ts_waitcnt vmcnt(1)", "\ts_cbranch_scc1 .LBB0_1"])) == {}
    # a block behind the loop does not inherit the loop's pending fetch
    assert isa.decode_waits(_kernel([LOOP, "\tglobal_load_ubyte v4, v[2:3], off", "\ts_cbranch_scc1 .LBB0_1", "; %bb.2:", "\ts_waitcnt vmcnt(0)"])) == {}
    # other kernels are not this rule's business
    assert isa.decode_waits(_kernel([LOOP] + FETCH + ["\ts_cbranch_scc1 .LBB0_1"], name="_ZN3agp12k_lag_tablesENS_7LagArgsE")) == {}


def test_both_instantiations_are_seen(asm):
    """the rule has something to look at: both kernels exist and carry loops"""
    lines = asm.split("\n")
    for k in KERNELS:
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        body = lines[start:]
        body = body[:next(i for i, l in enumerate(body) if "s_endpgm" in l)]
        assert sum("Loop Header" in l for l in body) >= 2, k


def test_no_loop_of_the_tile_builder_waits_for_an_opcode(isa, asm):
    offenders = isa.decode_waits(asm)
    assert not offenders, "\n".join(f"{k}: {v} loops" for k, v in offenders.items())
