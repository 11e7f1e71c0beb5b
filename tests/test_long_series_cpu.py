"""CPU tests of the long-series entry (agp_logpdf_long_series_batch): its declaration, export, documentation and Julia binding, the
max_n parameter of the packing helpers, the Python-side refusals, and the bad-pivot particles of tests/test_gpu_long_series.py on
the oracle's matrix."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _series_cases as S
import test_gpu_long_series as TL

ROOT = Path(__file__).resolve().parent.parent


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert "agp_logpdf_long_series_batch" in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint agp_logpdf_long_series_batch\s*\(", hdr)
    assert "agp_logpdf_long_series_batch" in (ROOT / "INTEGRATION.md").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and "agp_logpdf_long_series_batch" in seen
    m = re.search(r"#define\s+AGP_LONG_SERIES_MAX_N\s+(\d+)", hdr)
    assert m and pkg.LONG_SERIES_MAX_N == int(m.group(1)) == 512 and pkg.LONG_SERIES_MAX_N > pkg.SERIES_MAX_N
    m = re.search(r"#define\s+AGP_LONG_SERIES_ALL\s+(\d+)", hdr)
    assert m and pkg.LONG_SERIES_ALL == int(m.group(1)) == 1
    assert hasattr(pkg.GPEngine, "logpdf_long_series_batch")
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    assert re.search(r"const LONG_SERIES_MAX_N = %d\b" % pkg.LONG_SERIES_MAX_N, shim)
    assert re.search(r"const LONG_SERIES_ALL = Int32\(%d\)" % pkg.LONG_SERIES_ALL, shim)
    # the docstring sits directly above its own definition
    assert re.search(r'"\nfunction logpdf_long_series_batch\(', shim)
    # the kernel's cap and the table stride are the header's
    args = (ROOT / "autogp.jl_amd" / "csrc" / "agp_args.hpp").read_text()
    assert re.search(r"constexpr int LONG_SERIES_MAX_N = %d;" % pkg.LONG_SERIES_MAX_N, args)
    assert re.search(r"constexpr int LONG_SIG_STRIDE = %d;" % pkg.LONG_SERIES_MAX_N, args)


def test_pack_series_max_n(pkg):
    N = pkg.LONG_SERIES_MAX_N
    ok = (np.zeros(4), np.zeros(4))
    pt_off, ts, xs = pkg.pack_series([ok, (np.zeros(N), np.zeros(N))], max_n=N)
    assert pt_off.tolist() == [0, 4, 4 + N] and ts.shape == xs.shape == (4 + N,)
    with pytest.raises(ValueError, match=r"series 2 has 513 points.*LONG_SERIES_MAX_N \(512\)"):
        pkg.pack_series([ok, ok, (np.zeros(N + 1), np.zeros(N + 1))], max_n=N)
    # the default is the short entries' cap, as before
    n = pkg.SERIES_MAX_N + 1
    with pytest.raises(ValueError, match=r"series 1 has 177 points.*SERIES_MAX_N \(176\)"):
        pkg.pack_series([ok, (np.zeros(n), np.zeros(n))])
    with pytest.raises(ValueError, match="series 1"):
        pkg.series_call_args([ok, (np.zeros(n), np.zeros(n))], [pkg.Constant(1.0)], [0.1], [0])
    packed = pkg.series_call_args([ok, (np.zeros(n), np.zeros(n))], [pkg.Constant(1.0)], [0.1], [1], max_n=N)
    assert packed[0].tolist() == [0, 4, 4 + n] and packed[4] == 1


class NoLibrary:
    """stands where the loaded library would: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def test_bad_shapes_raise_before_any_library_call(pkg):
    eng = object.__new__(pkg.GPEngine)      # no library is loaded, no device is opened
    eng._lib = NoLibrary(); eng._ctx = None
    N = pkg.LONG_SERIES_MAX_N
    ok = (np.zeros(4), np.zeros(4))
    k = pkg.Constant(1.0)
    with pytest.raises(ValueError, match="series 1 has 513 points"):
        eng.logpdf_long_series_batch([ok, (np.zeros(N + 1), np.zeros(N + 1))], [k], [0.1], [0])
    with pytest.raises(ValueError, match="series 0"):
        eng.logpdf_long_series_batch([(np.zeros(4), np.zeros(5))], [k], [0.1], [0])
    with pytest.raises(ValueError, match="series 0"):
        eng.logpdf_long_series_batch([(np.zeros((2, 2)), np.zeros((2, 2)))], [k], [0.1], [0])
    with pytest.raises(ValueError, match="one noise per particle"):
        eng.logpdf_long_series_batch([ok], [k, k], [0.1], [0, 0])
    with pytest.raises(ValueError, match="one series index per particle"):
        eng.logpdf_long_series_batch([ok], [k, k], [0.1, 0.1], [0], all_long=True)


def test_changepoint_particles_fail_at_the_chosen_point(pkg):
    """CPU twin of tests/test_gpu_long_series.py::test_bad_pivots_at_chosen_points: on the oracle's matrix the first leading minor
    that cannot be factored is k + 1"""
    from oracle import oracle as O
    ts = TL.cp_ts()
    assert ts.size == pkg.LONG_SERIES_MAX_N == TL.CP_N
    for k in TL.CP_POINTS:
        K = O.compute_cov_matrix_vectorized(TL.changepoint_particle(pkg, k).to_tuple(), TL.CP_NOISE, ts)
        d = np.diag(K)
        assert np.allclose(d[:k], 0.5, atol=1e-7) and np.allclose(d[k:], -0.499, atol=1e-7)
        assert np.abs(K[:k, k:]).max(initial=0.0) <= 1e-11
        assert S.first_bad_minor(K) == k + 1, k
