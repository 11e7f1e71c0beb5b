"""CPU side of the long-series kernel's factor probe (agp_debug_long_series_factor, tests/test_gpu_long_series_probe.py): the entry
is declared, exported and wrapped; the shared cases are what they claim (bad pivots, exact particles); and a float64 twin of the
kernel's block algorithm (tests/_long_factor_ref.py) with planted faults shows why the probe exists — a panel entry off by 1e-9
relative fails the probe's bounds by two orders of magnitude and moves the log-density by less than 1e-12 relative, four orders
below the 1e-8 comparison of tests/test_gpu_long_series.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.linalg as sla

import _factor_ref as R
import _long_factor_ref as T
import _long_series_cases as LS
from test_gpu_factor_probe import M, M_SOLVE, BENIGN_CAP

ROOT = Path(__file__).resolve().parent.parent
VALUE_TOL = 1e-8      # tests/test_gpu_long_series.py: |d| <= 1e-8 max(1, |logpdf|)


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert "agp_debug_long_series_factor" in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint agp_debug_long_series_factor\s*\(", hdr)
    assert "agp_debug_long_series_factor" in (ROOT / "INTEGRATION.md").read_text()
    assert "agp_debug_long_series_factor" in (ROOT / "DESIGN.md").read_text()
    assert hasattr(pkg.GPEngine, "debug_long_series_factor")
    src = (ROOT / "autogp.jl_amd" / "csrc" / "agp_series.hip").read_text()
    assert re.search(r"\bint agp_debug_long_series_factor\s*\(", src)
    assert LS.N_CAP == pkg.LONG_SERIES_MAX_N and LS.NINE_UP_TO == pkg.SERIES_MAX_N + 1
    # the sizes name every loop body of stage (b): C = c first runs at n = 64 (c - 1) + 17
    assert {64 * (c - 1) + 17 for c in (1, 2, 6, 7, 8)} <= set(LS.SIZES) and LS.SIZES[-1] == LS.N_CAP


def test_shape_errors_raise_before_any_library_call(pkg):
    class NoLibrary:
        """stands where the loaded library would: any call into it fails the test"""
        def __getattr__(self, name):
            def reached(*args):
                raise AssertionError(f"the library was reached ({name})")
            return reached
    eng = object.__new__(pkg.GPEngine)      # no library is loaded, no device is opened
    eng._lib = NoLibrary(); eng._ctx = None
    with pytest.raises(ValueError, match=r"\(P, n, n\)"):
        eng.debug_long_series_factor(np.zeros((2, 3)))
    with pytest.raises(ValueError, match=r"\(P, n\)"):
        eng.debug_long_series_factor(np.zeros((2, 3, 3)), np.zeros((2, 4)))


# ---- the shared cases ----
def test_batches_have_the_stated_members():
    for n in (1, 17, 177):
        labels, K, y, kap = LS.batch(n)
        assert len(labels) == 9 and K.shape == (9, n, n) and y.shape == (9, n) and kap.shape == (9,)
        assert np.array_equal(y, R.batch_rhs(n)) and not K.flags.writeable
    labels, K, y, kap = LS.batch(337)
    assert tuple(labels) == R.FAMILIES and K.shape == (5, 337, 337)
    assert np.array_equal(y, R.batch_rhs(337)[:5]) and np.array_equal(K[3], R.family("se_grid", 337))
    assert LS.batch(337) is LS.batch(337)
    assert (kap >= 1.0).all() and kap[0] <= 8.0 and kap[1] <= 8.0


@pytest.mark.parametrize("spec", LS.INFO_SPECS, ids=LS.info_name)
def test_info_probes_fail_at_the_stated_pivot(spec):
    """the reference factor stops at exactly the stated pivot, LAPACK reports it, and so does the twin"""
    K, want = LS.info_probe(spec)
    assert (K == K.T).all() and K.shape[0] <= LS.N_CAP
    with pytest.raises(ArithmeticError, match=rf"pivot {want - 1} is not positive"):
        R.ref_chol(K)
    _, info = sla.lapack.dpotrf(K, lower=1)
    assert info == want
    L, alpha, _, lp, tinfo = T.long_factor(K)
    assert tinfo == want and L is None and np.isnan(lp)


def test_info_probes_cover_the_issue_list():
    names = [LS.info_name(s) for s in LS.INFO_SPECS]
    assert len(names) == len(set(names)) == 18 + 2 + 3 + 2 + 1
    assert LS.info_probe(("indefinite", 512, (272, 40)))[1] == 41 and LS.info_probe(("indefinite", 512, (16, 17)))[1] == 17
    # [272, 40]: the later pivot's block row belongs to a lower-numbered wave than the earlier one's
    assert (272 // 16) % 4 < (40 // 16) % 4


def test_exact_particles_are_exact(pkg):
    """the covariance of tests/test_gpu_long_series_probe.py::test_probe_is_the_production_code does not depend on the order of
    evaluation: the oracle's float64 matrix equals the one computed in longdouble, entry for entry; the Linear particle's matrix is
    positive definite with smallest eigenvalue 0.25 (its noise)"""
    from oracle import oracle as O
    for n in (1, 17, 177, 512):
        ts, particles = LS.exact_particles(pkg, n)
        assert ts[-1] < 1.0 and np.array_equal(ts * 512, np.arange(n))
        t = ts.astype(np.longdouble)
        want = [np.full((n, n), 0.5, dtype=np.longdouble) + 0.5 * np.eye(n),
                0.5 + 2.0 * np.outer(t - 0.25, t - 0.25) + 0.25 * np.eye(n)]
        for (node, noise), W in zip(particles, want):
            K = O.compute_cov_matrix_vectorized(node.to_tuple(), noise, ts)
            assert (K.astype(np.longdouble) == W).all()
            ev = np.linalg.eigvalsh(K)
            assert ev[0] >= 0.25 * (1 - 1e-9)
    assert abs(ev[0] - 0.25) <= 1e-9      # (the Linear particle at n = 512: rank two + 0.25 I)


# ---- the twin and its planted faults ----
def _ratios(K, y, L, alpha):
    n = K.shape[0]
    return R.omega(K, L) / R.gamma(n + 1), R.omega_solve(L, alpha, y) / R.gamma(n)


def _within_bounds(fam, kap, w, ws):
    cap = min(kap, BENIGN_CAP.get(fam, np.inf))
    return w <= min(M[fam], cap) and ws <= min(M_SOLVE[fam], cap)


@pytest.mark.parametrize("n", (512, 497))
@pytest.mark.parametrize("fam", ("wishart", "graded"))
def test_bounds_reject_a_scaled_entry_the_value_cannot_see(fam, n):
    """the reason for the probe: on the benign families the clean twin passes the bounds of test_gpu_long_series_probe.py, an entry of
    a panel block scaled by 1 + 1e-9 — in block row 31 and in a middle block row — fails them, and the same fault moves the twin's
    log-density by less than the value tolerance"""
    i = R.FAMILIES.index(fam)
    labels, Ks, ys, kaps = LS.batch(n)
    assert labels[i] == fam
    K, y, kap = Ks[i], ys[i], kaps[i]
    L, alpha, part, lp, info = T.long_factor(K, y)
    assert info == 0 and np.array_equal(L, np.tril(L))
    w, ws = _ratios(K, y, L, alpha)
    print(f"n {n} {fam}: clean omega/gamma {w:.4f} solve {ws:.4f} kappa_blk {kap:.3f} logpdf {lp!r}")
    assert _within_bounds(fam, kap, w, ws)
    # the twin's value is the reference's to well within the value tolerance
    Lr = R.ref_chol(K)
    want = -(n * np.log(2 * np.pi) + 2 * np.log(np.diag(Lr)).sum() + (R.ref_forward(Lr, y.astype(R.LD)) ** 2).sum()) / 2
    assert abs(lp - float(want)) <= 1e-12 * max(1.0, abs(lp))
    for fault in (("scale", 31, 10, 0, 7, 1e-9), ("scale", 15, 6, 5, 7, 1e-9)):
        Lf, af, _, lpf, info = T.long_factor(K, y, fault=fault)
        assert info == 0
        wf, wsf = _ratios(K, y, Lf, af)
        moved = abs(lpf - lp) / max(1.0, abs(lp))
        print(f"n {n} {fam} {fault}: omega/gamma {wf:.4g} solve {wsf:.4g}, logpdf moved {moved:.3g} relative")
        assert not _within_bounds(fam, kap, wf, wsf)
        assert wf > 10 * min(M[fam], kap, BENIGN_CAP[fam])      # (not a near miss)
        assert moved < 1e-4 * VALUE_TOL


def test_a_lost_k_step_is_seen_by_both():
    """a gross fault — one element of one k-step of stage (b) lost — fails the bounds, and the value sees it too (where the entry
    is not tiny): the gap the probe closes is the subtle faults"""
    n, fam = 512, "wishart"
    _, Ks, ys, kaps = LS.batch(n)
    K, y, kap = Ks[0], ys[0], kaps[0]
    _, _, _, lp, _ = T.long_factor(K, y)
    Lf, af, _, lpf, info = T.long_factor(K, y, fault=("kstep", 31, 12, 3, 0, 4))
    assert info == 0
    wf, wsf = _ratios(K, y, Lf, af)
    assert not _within_bounds(fam, kap, wf, wsf) and wf > 1e6
    assert abs(lpf - lp) > VALUE_TOL * max(1.0, abs(lp))


def test_leaving_out_the_refinement_changes_no_factor_and_hardly_the_value():
    """the refinement step of (d) touches alpha only: L is the clean twin's bit for bit, and the log-density moves by less than
    1e-12 relative — invisible to the value comparison; what it buys is the forward solve's backward error, which the probe bounds
    (omega_solve / gamma_n) and the value does not"""
    n = 497
    labels, Ks, ys, _ = LS.batch(n)
    for i in (0, 4):
        L, alpha, _, lp, _ = T.long_factor(Ks[i], ys[i])
        Lf, af, _, lpf, _ = T.long_factor(Ks[i], ys[i], fault=("no_refine",))
        assert np.array_equal(L, Lf) and not np.array_equal(alpha, af)
        assert abs(lpf - lp) <= 1e-12 * max(1.0, abs(lp)), labels[i]
