"""The block Cholesky inside the long-series value kernel (k_long_series_logpdf, csrc/agp_long_series_kernel.hpp) on caller-supplied
matrices (GPEngine.debug_long_series_factor: the kernel's probe instantiation, whose stages 3 (b) - (e) and 4 are the production
statements): backward error of L and of the carried forward solve, the log-det / quadratic-form partials and the value against the L
and alpha they came from, LAPACK info at every pivot boundary, isolation of failed matrices, run-to-run determinism, bitwise
agreement of the probe with logpdf_long_series_batch on particles whose covariance is exact in float64, and the same bits from an
engine whose workspace starts as NaNs.  The value alone cannot see what these see: tests/test_long_series_probe_cpu.py.

Sizes and matrices: tests/_long_series_cases.py (every loop body of stage (b), C = 1 .. 8, prefetching and not).

Bounds.  The long kernel shares factor16 and the explicit block inverses with the tile schedules (csrc/agp_lds_chol.hpp), so it may
lose no more than they do.  Up to n = 300 the margins are M / M_SOLVE of tests/test_gpu_factor_probe.py.  For the larger sizes the
tile schedules were measured at n = 337, 401, 465, 497, 512 on members 0 - 4 of the batch of nine (the last block of
profiles/factor_probe_accuracy.txt, appended by tools/gpu_factor_probe_accuracy.py --append --sizes 337,401,465,497,512 --members
0,1,2,3,4); TILE_LARGE below is that block's per-family maxima and M_LONG = max(M, 8 x ratio), three bits for reduction orders and
compiler releases as everywhere.  Every bound is capped per matrix by kappa_blk of the longdouble reference factor and by 8 on the
benign families.  No number here was measured on the kernel under test; what it measures is recorded in
profiles/long_series_probe_accuracy.txt (tools/gpu_long_series_probe_accuracy.py), which nothing reads."""
import ctypes as C

import numpy as np
import pytest

import _factor_ref as R
import _long_series_cases as LS
from test_gpu_factor_probe import M, M_SOLVE, BENIGN_CAP

pytestmark = pytest.mark.gpu

# profiles/factor_probe_accuracy.txt, "# n = 337, 401, 465, 497, 512, members 0,1,2,3,4": largest omega / gamma_(n+1) and
# omega_solve / gamma_n of the tile schedules per family
TILE_LARGE = {"wishart": (0.0330, 0.0124), "graded": (0.0441, 0.0377), "spec": (0.0493, 0.0041), "se_grid": (97.1783, 0.0042),
              "se_irreg": (6.6381, 0.0026)}
M_LONG = {fam: max(M[fam], 8 * TILE_LARGE[fam][0]) for fam in R.FAMILIES}
M_SOLVE_LONG = {fam: max(M_SOLVE[fam], 8 * TILE_LARGE[fam][1]) for fam in R.FAMILIES}
LARGE_FROM = 301      # M / M_SOLVE were measured up to n = 300

NAMES = ("L", "alpha", "partial", "logpdf")
LOG_2PI = np.log(8 * np.arctan(R.LD(1)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def margins(n):
    return (M_LONG, M_SOLVE_LONG) if n >= LARGE_FROM else (M, M_SOLVE)


def test_margins_are_admissible():
    for table in (M_LONG, M_SOLVE_LONG):
        assert set(table) == set(R.FAMILIES)
        for fam, m in table.items():
            assert 1.0 <= m <= BENIGN_CAP.get(fam, np.inf), (fam, m)


@pytest.mark.parametrize("n", LS.SIZES)
def test_backward_error_solve_partials_and_value(engine, n):
    labels, K, y, kap = LS.batch(n)
    Mf, Ms = margins(n)
    L, alpha, part, lp, info = engine.debug_long_series_factor(K, y)
    assert (info == 0).all(), info
    fails = []
    for i, fam in enumerate(labels):
        assert np.array_equal(L[i], np.tril(L[i])), "L is not exactly lower triangular"
        cap = min(kap[i], BENIGN_CAP.get(fam, np.inf))
        # (a) backward error of the factor, and of the carried forward solve against the L it was computed with
        w = R.omega(K[i], L[i]) / R.gamma(n + 1)
        ws = R.omega_solve(L[i], alpha[i], y[i]) / R.gamma(n)
        print(f"n {n} {fam:9s}[{i}]: omega/gamma {w:.4f} (M {Mf[fam]:.3f}) solve {ws:.4f} (M {Ms[fam]:.3f}) kappa_blk {kap[i]:.4g}")
        if not w <= min(Mf[fam], cap):
            fails.append(f"{fam}[{i}]: omega / gamma_(n+1) = {w:.4g} > min(M = {Mf[fam]:.4g}, cap = {cap:.4g})")
        if not ws <= min(Ms[fam], cap):
            fails.append(f"{fam}[{i}]: omega_solve / gamma_n = {ws:.4g} > min(M = {Ms[fam]:.4g}, cap = {cap:.4g})")
        # (b) the log-det partial against the returned diagonal: one 1-ulp log per term + the sum
        lg = 2 * np.log(np.diag(L[i]).astype(R.LD))
        if not abs(R.LD(part[i, 0]) - lg.sum()) <= R.gamma(n + 2) * np.abs(lg).sum():
            fails.append(f"{fam}[{i}]: logdet {part[i, 0]!r} vs {float(lg.sum())!r} (bound {float(R.gamma(n + 2) * np.abs(lg).sum()):.3g})")
        # ... alpha'alpha against the returned alpha
        aa = (alpha[i].astype(R.LD) ** 2).sum()
        if not abs(R.LD(part[i, 1]) - aa) <= R.gamma(n) * aa:
            fails.append(f"{fam}[{i}]: alpha'alpha {part[i, 1]!r} vs {float(aa)!r}")
        # ... and the value against the two partials: a rounded constant, a product and two sums
        want = -(n * LOG_2PI + R.LD(part[i, 0]) + R.LD(part[i, 1])) / 2
        tol = 4 * R.U * (n * LOG_2PI + abs(R.LD(part[i, 0])) + R.LD(part[i, 1]))
        if not abs(R.LD(lp[i]) - want) <= tol:
            fails.append(f"{fam}[{i}]: logpdf {lp[i]!r} vs {float(want)!r} (bound {float(tol):.3g})")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("spec", LS.INFO_SPECS, ids=LS.info_name)
def test_info_at_every_pivot_boundary(engine, spec):
    """LAPACK's info = 1 + the first non-positive pivot, whichever 4-wide sub-step, block, wave and round of the four waves it falls
    in; the value is NaN exactly where info != 0"""
    K, want = LS.info_probe(spec)
    _, _, _, lp, info = engine.debug_long_series_factor(K[None], None)
    assert info[0] == want
    assert np.isnan(lp[0])


@pytest.mark.parametrize("n", (1, 497, 512))
def test_info_is_zero_on_a_definite_matrix(engine, n):
    K = R.family("wishart", n)
    _, _, _, lp, info = engine.debug_long_series_factor(K[None], None)
    assert info[0] == 0 and np.isfinite(lp[0])


def test_failed_matrices_are_isolated_and_runs_repeat(engine):
    """what logpdf_long_series_batch relies on with check=False: a failed particle changes no bit of its neighbours, whatever the
    batch (everything here is bitwise: no reference factor)"""
    n = LS.N_CAP
    K = np.stack([k for _, k in R.batch_of_nine(n)])
    y = R.batch_rhs(n)
    Kbad = np.array(K)
    Kbad[2] = R.indefinite(n, [5]); Kbad[8] = R.indefinite(n, [400], seed=1)
    good = [0, 1, 3, 4, 5, 6, 7]
    ref = engine.debug_long_series_factor(K, y)
    got = engine.debug_long_series_factor(Kbad, y)
    again = engine.debug_long_series_factor(Kbad, y)
    assert got[4].tolist() == [0, 0, 6, 0, 0, 0, 0, 0, 401]
    assert (ref[4] == 0).all()
    assert np.isnan(got[3][[2, 8]]).all() and np.isfinite(got[3][good]).all()
    for a, b, c, name in zip(ref, got, again, NAMES):
        assert np.array_equal(bits(a[good]), bits(b[good])), f"{name}: a failed matrix changed its neighbours"
        assert np.array_equal(bits(b[good]), bits(c[good])), f"{name}: two identical calls differ"
    assert np.array_equal(got[4], again[4])
    for i in good:
        one = engine.debug_long_series_factor(K[i:i + 1], y[i:i + 1])
        assert one[4][0] == 0
        for a, b, name in zip(one, got, NAMES):
            assert np.array_equal(bits(a[0]), bits(b[i])), f"{name} of matrix {i}: batch of nine and P = 1 differ"


@pytest.mark.parametrize("n", (1, 17, 177, 337, 465, 512))
def test_probe_is_the_production_code(pkg, engine, n):
    """on a covariance that is exact in float64 the production instantiations factor the very matrix the probe is given: the
    values agree bit for bit"""
    from oracle import oracle as O
    ts, particles = LS.exact_particles(pkg, n)
    xs = np.random.default_rng(77 + n).standard_normal(n)
    for node, noise in particles:
        K = O.compute_cov_matrix_vectorized(node.to_tuple(), noise, ts)
        # precondition (a failure here means the inputs are not exact, not that the engine is wrong)
        assert np.array_equal(bits(K), bits(engine.cov_matrix(node, noise, ts))), "the covariance is not exact: choose other dyadic values"
        lp, info = engine.logpdf_long_series_batch([(ts, xs)], [node], [noise], [0], all_long=True)
        _, _, _, lp_probe, info_probe = engine.debug_long_series_factor(K[None], xs[None])
        assert info[0] == 0 and info_probe[0] == 0
        assert bits(lp_probe)[0] == bits(lp)[0], (n, type(node).__name__, lp_probe[0], lp[0])


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    """a second GPEngine created under AGP_POISON=1 (every `values` buffer of the slot, the factor workspace among them, is NaN bytes
    before the call) returns the unpoisoned engine's bits: no block of the workspace is read before it is written, also not by the
    read-back of the probe (ragged last block row at 497, the cap)"""
    monkeypatch.setenv("AGP_POISON", "1")
    e = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_POISON")
    try:
        for n in (497, 512):
            _, K, y, _ = LS.batch(n)
            ref = engine.debug_long_series_factor(K, y)
            got = e.debug_long_series_factor(K, y)
            assert (ref[4] == 0).all() and np.array_equal(ref[4], got[4])
            for a, b, name in zip(ref, got, NAMES):
                assert np.array_equal(bits(a), bits(b)), (n, name, np.flatnonzero(bits(a).ravel() != bits(b).ravel())[:8])
        assert e.poison_stats()["bytes"] > 0
    finally:
        e.close()


def test_argument_errors(pkg, engine):
    cap = pkg.LONG_SERIES_MAX_N
    assert cap == LS.N_CAP

    def valid():
        K = LS.batch(17)[1][:1]
        L, _, _, _, info = engine.debug_long_series_factor(K, None)
        assert info[0] == 0 and R.omega(K[0], L[0]) <= 8 * R.gamma(18)      # (wishart: BENIGN_CAP)

    with pytest.raises(pkg.AGPError, match=str(cap)):
        engine.debug_long_series_factor(np.zeros((1, 0, 0)), None)
    valid()
    with pytest.raises(pkg.AGPError, match=str(cap)):
        engine.debug_long_series_factor(np.eye(cap + 1)[None], None)
    valid()
    with pytest.raises(pkg.AGPError, match="256"):
        engine.debug_long_series_factor(np.zeros((0, 5, 5)), None)
    valid()
    with pytest.raises(pkg.AGPError, match="256"):
        engine.debug_long_series_factor(np.broadcast_to(np.eye(2), (257, 2, 2)), None)
    valid()
    n = 5
    out = (np.zeros((1, n, n)), np.zeros((1, n)), np.zeros((1, 2)), np.zeros(1))
    info = np.zeros(1, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    rc = engine._lib.agp_debug_long_series_factor(engine._ctx, None, None, n, 1, *(o.ctypes.data_as(dp) for o in out),
                                                  info.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == -1
    with pytest.raises(pkg.AGPError, match="null"):
        engine._check(rc)
    valid()
