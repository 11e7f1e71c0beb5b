"""The host-only particle helpers (autogp.jl_amd/csrc/agp_particles.hpp: views, dedup, packing, scatter, composite programs),
checked by a stand-alone C++ program under address and undefined-behaviour sanitizers.  No GPU, nothing loaded into Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_particles_header_standalone(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the host-only header is checked by a native program")
    exe = tmp_path / "particles_test"
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'autogp.jl_amd' / 'csrc'}",
            str(ROOT / "tests" / "native" / "particles_test.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr):      # the sanitizer runtimes are not installed
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "particles_test: ok" in r.stdout
