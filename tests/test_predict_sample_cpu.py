"""Host-side checks of posterior predictive sampling (agp_predict_sample_batch): the Philox4x64-10 header csrc/agp_philox.hpp compiled
with g++ against numpy.random.Philox and the restatement of tests/_pred_sample_ref.py, the known answer of the generator, the
uniform map, the component inverse CDF and u -> ndtri; plus the Python layer's argument handling that needs no device."""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.special import ndtri

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _pred_sample_ref as R      # noqa: E402

SRC = r"""
#include <stdint.h>
#include "agp_philox.hpp"
extern "C" {
void v_block(const uint64_t* c, uint64_t k0, uint64_t* out) {
  const agp::Philox4 b = agp::philox4x64_10(c[0], c[1], c[2], c[3], k0, 0);
  for (int i = 0; i < 4; ++i) out[i] = b.w[i];
}
double v_uniform(uint64_t w) { return agp::philox_uniform(w); }
}
"""


@pytest.fixture(scope="module")
def philox_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("philox")
    (d / "p.cpp").write_text(SRC)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", str(ROOT / "autogp.jl_amd" / "csrc"), str(d / "p.cpp"),
                    "-o", str(d / "p.so")], check=True)
    lib = ctypes.CDLL(str(d / "p.so"))
    lib.v_block.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.v_uniform.argtypes = [ctypes.c_uint64]; lib.v_uniform.restype = ctypes.c_double
    return lib


def header_block(lib, seed, c):
    ca = np.array(c, dtype=np.uint64); out = np.zeros(4, dtype=np.uint64)
    lib.v_block(ca.ctypes.data, seed, out.ctypes.data)
    return [int(v) for v in out]


def test_known_answer():
    assert R.philox_block(0, 0, 0, 0, 0)[0] == 0x16554d9eca36314c


def test_header_matches_numpy_philox(philox_lib):
    rng = np.random.default_rng(1)
    M = (1 << 64) - 1
    cases = [(0, (0, 0, 0, 0)), (0, (1, 0, 0, 0)), (7, (0, 3, 1, 0)), (M, (M, M, M, M)), (123456789, (5, 0, 0, 0))]
    cases += [(int(rng.integers(0, 2**63)), tuple(int(v) for v in rng.integers(0, 2**63, 4))) for _ in range(20)]
    for seed, c in cases:
        assert header_block(philox_lib, seed, c) == R.philox_block(seed, *c), (seed, c)


def test_uniform_map(philox_lib):
    M = (1 << 64) - 1
    for w in (0, 1, 2047, 2048, 1 << 63, M - 4096, M - 2048, M):
        u = philox_lib.v_uniform(w)
        assert u == R.uniform(w) and 0.0 < u < 1.0, w
    assert R.uniform(0) == 2.0 ** -54
    assert R.uniform(M) == 1.0 - 2.0 ** -53      # (the one word that rounds to 1)
    rng = np.random.default_rng(2)
    for w in rng.integers(0, 2**63, 200, dtype=np.int64):
        w = int(w) * 2 + 1
        assert philox_lib.v_uniform(w) == R.uniform(w)


def test_component_inverse_cdf():
    S = 4000
    w = np.array([0.0, 0.2, 0.0, 0.5, 0.3, 0.0])
    c = R.components(11, w, S)
    assert set(np.unique(c)) <= {1, 3, 4}
    freq = np.bincount(c, minlength=6) / S
    assert np.all(np.abs(freq - w) <= 5 * np.sqrt(w * (1 - w) / S) + 1e-12)
    # the rule itself: first p with u < cum[p]
    cum = np.cumsum(w)
    for s in range(50):
        u = R.uniform(R.philox_block(11, s, 0, 0, 0)[0])
        assert c[s] == int(np.argmax(u < cum))
    # rounding at the top end: cum[-1] < 1 falls to the last particle of positive weight
    w2 = np.array([0.25, 0.25, 0.5 - 1e-9, 0.0])
    c2 = R.components(3, w2, 2000)
    assert 3 not in c2 and (c2 == 2).any()
    u_all = np.array([R.uniform(R.philox_block(3, s, 0, 0, 0)[0]) for s in range(2000)])
    assert np.array_equal(c2[u_all >= np.cumsum(w2)[-1]], np.full((u_all >= np.cumsum(w2)[-1]).sum(), 2))


def test_normals_restatement():
    z = R.normals(5, 7, [0, 3, 10])
    for j, s in enumerate([0, 3, 10]):
        for i in range(7):
            u = R.uniform(R.philox_block(5, i // 4, s, 1, 0)[i % 4])
            assert z[i, j] == ndtri(u)
    zz = R.normals(9, 5, range(4000)).ravel()
    assert abs(zz.mean()) < 5 / np.sqrt(zz.size) and abs(zz.var() - 1) < 5 * np.sqrt(2 / zz.size)
    # a column depends on its own sample index only
    assert np.array_equal(R.normals(5, 7, [10])[:, 0], z[:, 2])


def test_python_layer_is_wired(pkg):
    assert "agp_predict_sample_batch" in pkg.EXPORTED_SYMBOLS
    assert callable(pkg.predict_rand) and hasattr(pkg.MvNormal, "rand") and hasattr(pkg.GPEngine, "predict_sample_batch")
