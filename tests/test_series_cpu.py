"""CPU tests of the many-short-series entry (agp_logpdf_series_batch): its declaration, export, documentation and Julia binding,
and the pure packing helper pack_series."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _series_cases as S

ROOT = Path(__file__).resolve().parent.parent


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert "agp_logpdf_series_batch" in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint agp_logpdf_series_batch\s*\(", hdr)
    assert "agp_logpdf_series_batch" in (ROOT / "INTEGRATION.md").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and "agp_logpdf_series_batch" in seen
    m = re.search(r"#define\s+AGP_SERIES_MAX_N\s+(\d+)", hdr)
    assert m and pkg.SERIES_MAX_N == int(m.group(1)) and pkg.SERIES_MAX_N >= 160
    assert hasattr(pkg.GPEngine, "logpdf_series_batch")
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    assert re.search(r"const SERIES_MAX_N = %d\b" % pkg.SERIES_MAX_N, shim)
    # the docstring sits directly above its own definition
    assert re.search(r'"\nfunction logpdf_series_batch\(', shim)


def test_pack_series_offsets_and_types(pkg):
    rng = np.random.default_rng(0)
    lens = [3, 0, 17, 1, pkg.SERIES_MAX_N, 0]
    series = [(rng.random(n), rng.standard_normal(n)) for n in lens]
    series[2] = (list(series[2][0]), series[2][1].astype(np.float32).astype(np.float64)[::1])      # any array-like
    pt_off, ts, xs = pkg.pack_series(series)
    assert pt_off.dtype == np.int64 and ts.dtype == np.float64 and xs.dtype == np.float64
    assert pt_off.flags.c_contiguous and ts.flags.c_contiguous and xs.flags.c_contiguous
    assert pt_off.tolist() == [0] + list(np.cumsum(lens))
    assert ts.shape == xs.shape == (sum(lens),)
    for s, (t, x) in enumerate(series):
        assert np.array_equal(ts[pt_off[s]:pt_off[s + 1]], np.asarray(t, dtype=np.float64))
        assert np.array_equal(xs[pt_off[s]:pt_off[s + 1]], np.asarray(x, dtype=np.float64))
    pt_off, ts, xs = pkg.pack_series([])
    assert pt_off.tolist() == [0] and ts.shape == (0,) and xs.shape == (0,) and pt_off.dtype == np.int64


def test_pack_series_rejects_bad_input(pkg):
    ok = (np.zeros(4), np.zeros(4))
    with pytest.raises(ValueError, match="series 1"):
        pkg.pack_series([ok, (np.zeros(4), np.zeros(5))])
    with pytest.raises(ValueError, match="series 0"):
        pkg.pack_series([(np.zeros((2, 2)), np.zeros((2, 2)))])
    n = pkg.SERIES_MAX_N + 1
    with pytest.raises(ValueError, match="series 2"):
        pkg.pack_series([ok, ok, (np.zeros(n), np.zeros(n))])
    pkg.pack_series([(np.zeros(n - 1), np.zeros(n - 1))])


def test_changepoint_particles_fail_at_the_chosen_point(pkg):
    """CPU twin of tests/test_gpu_series.py::test_info_at_every_sub_step_and_block: on the oracle's matrix the first leading minor
    that cannot be factored is k + 1"""
    from oracle import oracle as O
    assert pkg.SERIES_MAX_N == S.N_CAP == S.CP_TS.size
    for k in S.CP_POINTS:
        K = O.compute_cov_matrix_vectorized(S.changepoint_particle(pkg, k).to_tuple(), S.CP_NOISE, S.CP_TS)
        d = np.diag(K)
        assert np.allclose(d[:k], 0.5, atol=1e-12) and np.allclose(d[k:], -0.499, atol=1e-12)
        assert np.abs(K[:k, k:]).max(initial=0.0) <= 1e-15
        assert S.first_bad_minor(K) == k + 1, k


def test_exact_particles_are_exact(pkg):
    """the covariance of tests/test_gpu_series_probe.py::test_probe_is_the_production_code does not depend on the order of evaluation:
    the oracle's float64 matrix equals the one computed in longdouble, entry for entry"""
    from oracle import oracle as O
    for n in (1, 17, 176):
        ts, particles = S.exact_particles(pkg, n)
        t = ts.astype(np.longdouble)
        want = [np.full((n, n), 0.5, dtype=np.longdouble) + 0.5 * np.eye(n),
                0.5 + 2.0 * np.outer(t - 0.25, t - 0.25) + 0.25 * np.eye(n)]
        for (node, noise), W in zip(particles, want):
            K = O.compute_cov_matrix_vectorized(node.to_tuple(), noise, ts)
            assert (K.astype(np.longdouble) == W).all()
            assert S.first_bad_minor(K) is None
