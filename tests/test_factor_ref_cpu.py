"""The host reference of the factor probe tests (tests/_factor_ref.py) checked on its own: its metrics accept a correct factor
(LAPACK's, within Higham's bounds), reject planted faults of the sizes a wrong kernel would produce, and its indefinite matrices
fail at the pivot they claim."""
import numpy as np
import pytest
import scipy.linalg as sla

import _factor_ref as R
import _series_cases as S

SIZES = (5, 16, 17, 129, 300)
# pivots the GPU tests pin (tests/test_gpu_factor_probe.py): every 4 / 16 / 128 boundary of the diagonal tile's sub-steps
PIVOTS = (0, 1, 2, 3, 4, 15, 16, 127, 128, 129, 255, 256, 299)


@pytest.fixture(scope="module")
def planted():
    """n = 300 members of the two families with benign diagonal blocks (kappa_blk <= 8) with LAPACK's factor, a right-hand side and
    the detection thresholds: a fault counts as detected when it exceeds the bound times kappa_blk."""
    out = []
    for name in ("wishart", "graded"):
        K = R.family(name, 300)
        L = np.linalg.cholesky(K)
        y = np.random.default_rng(11).standard_normal(300)
        kb = R.kappa_blk(L)
        assert kb <= 8.0, (name, kb)
        out.append((name, K, L, y, R.gamma(301) * kb, R.gamma(300) * kb))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_lapack_factor_is_within_highams_bound(name, n):
    K = R.family(name, n)
    assert (K == K.T).all()
    L = sla.cholesky(K, lower=True)
    w = R.omega(K, L) / R.gamma(n + 1)
    y = np.random.default_rng(n).standard_normal(n)
    ws = R.omega_solve(L, sla.solve_triangular(L, y, lower=True), y) / R.gamma(n)
    kb = R.kappa_blk(L)
    print(f"{name:9s} n={n:3d} omega/gamma={w:.3f} omega_solve/gamma={ws:.3f} kappa_blk={kb:.3g}")
    assert 0.0 < w <= 1.0 and ws <= 1.0 and kb >= 1.0
    # the longdouble reference factor sits well inside the bound (it is what kappa_blk is computed from in the GPU tests)
    assert R.omega(K, R.ref_chol(K).astype(np.float64)) <= R.gamma(n + 1)


def test_kappa_blk_ranges():
    """benign families stay below 10 at every size (below 8 at n = 300, where the faults are planted); the ill-conditioned ones are
    the ones that exercise explicit inverses"""
    for n in SIZES:
        for name in ("wishart", "graded"):
            assert R.kappa_blk(R.ref_chol(R.family(name, n))) <= 10.0
    assert R.kappa_blk(R.ref_chol(R.family("se_grid", 300))) > 1e3
    assert R.kappa_blk(R.ref_chol(R.family("spec", 16))) > 1e4


def test_fault_one_entry_scaled(planted):
    for name, K, L, y, thr, _ in planted:
        assert R.omega(K, L) <= R.gamma(301)
        for (i, j) in ((299, 0), (299, 299), (256, 130)):      # last tile row: first column, last pivot, inside tile (2, 1)
            Lf = L.copy()
            Lf[i, j] *= 1.0 + 1e-11
            assert R.omega(K, Lf) > thr, (name, i, j)


def test_fault_dropped_k_slab(planted):
    """tile (2, 1) of a left-looking update recomputed without the 16-wide slab of columns 32 .. 47"""
    for name, K, L, y, thr, _ in planted:
        keep = np.r_[0:32, 48:128]
        for cols, expect_fault in ((np.r_[0:128], False), (keep, True)):
            C = K[256:300, 128:256] - L[256:300, cols] @ L[128:256, cols].T
            Lf = L.copy()
            Lf[256:300, 128:256] = sla.solve_triangular(L[128:256, 128:256], C.T, lower=True).T
            w = R.omega(K, Lf)
            assert (w > thr) == expect_fault, (name, expect_fault, w, thr)


def _chol_bad_pivot(K, jbad, rel):
    """right-looking Cholesky in double whose column jbad is scaled with a reciprocal root that is off by `rel`"""
    A = K.copy(); n = A.shape[0]; L = np.zeros_like(A)
    for j in range(n):
        ri = 1.0 / np.sqrt(A[j, j])
        if j == jbad:
            ri *= 1.0 + rel
        L[j, j] = A[j, j] * ri
        L[j + 1:, j] = A[j + 1:, j] * ri
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def test_fault_unrefined_reciprocal_root(planted):
    for name, K, L, y, thr, _ in planted:
        assert R.omega(K, _chol_bad_pivot(K, -1, 0.0)) <= thr
        for jbad in (0, 130, 299):
            assert R.omega(K, _chol_bad_pivot(K, jbad, 2.0 ** -23)) > thr, (name, jbad)


def test_fault_solve_skipped_block(planted):
    for name, K, L, y, _, thr in planted:
        assert R.omega_solve(L, R.ref_forward(L, y), y) <= R.gamma(300)
        for blk in ((18, 3), (1, 0), (18, 17)):
            assert R.omega_solve(L, R.ref_forward(L, y, skip_block=blk), y) > thr, (name, blk)


@pytest.mark.parametrize("js", [[j] for j in PIVOTS] + [[129, 40], [16, 17]])
def test_indefinite_fails_at_the_first_negative_pivot(js):
    K = R.indefinite(300, js)
    assert (K == K.T).all()
    _, info = sla.lapack.dpotrf(K, lower=1)
    assert info == min(js) + 1


@pytest.mark.parametrize("j", (0, 128))
def test_zero_pivot(j):
    _, info = sla.lapack.dpotrf(R.zero_pivot(300, j), lower=1)
    assert info == j + 1


# ---- what tests/test_gpu_series_probe.py takes for granted (sizes up to the short-series kernel's cap) ----
@pytest.mark.parametrize("n", S.SIZES)
def test_reference_factor_exists_at_every_series_probe_size(n):
    """every member of the batch of nine has a longdouble factor (kappa_blk, the per-matrix cap, is computed from it); at n = 1
    the cap is exactly 1: no explicit inverse excuses anything there"""
    for name, K in R.batch_of_nine(n):
        assert (K == K.T).all()
        L = R.ref_chol(K)
        kb = R.kappa_blk(L)
        assert np.isfinite(kb) and kb >= 1.0, (name, n, kb)
        if n == 1:
            assert kb == 1.0, (name, kb)


def test_series_info_probes_fail_at_the_stated_pivot():
    for K, want, name in S.info_probes():
        assert (K == K.T).all() and K.shape[0] <= S.N_CAP
        with pytest.raises(ArithmeticError, match=rf"pivot {want - 1} is not positive"):
            R.ref_chol(K)
        _, info = sla.lapack.dpotrf(K, lower=1)
        assert info == want, name
