"""The factorisation inside the short-series value kernel (k_series_logpdf, csrc/agp_series_kernel.hpp) on caller-supplied matrices
(GPEngine.debug_series_factor: the kernel's probe instantiation, whose stages 4 and 5 are the production statements): backward error
of L and of the carried forward solve, the log-det / quadratic-form partials and the value against the L and alpha they came from,
LAPACK info at every 4 / 16 boundary and in a ragged last block, isolation of failed matrices, run-to-run determinism, and bitwise
agreement of the probe with logpdf_series_batch on particles whose covariance is exact in float64.

Bounds.  The series kernel shares the block steps of the tile schedules (csrc/agp_lds_chol.hpp: 16 x 16 diagonal blocks with explicit
inverses, one refinement step per block of the forward solve), so it may lose no more than they do: the margins M, M_SOLVE and BENIGN_CAP are the
tables of tests/test_gpu_factor_probe.py (8 x what the tile schedules measured at n up to 300), capped per matrix by kappa_blk of
the longdouble reference factor.  No number here was measured on the kernel under test; what it measures is recorded in
profiles/series_probe_accuracy.txt (tools/gpu_series_probe_accuracy.py), which nothing reads."""
import ctypes as C

import numpy as np
import pytest

import _factor_ref as R
import _series_cases as S
from test_gpu_factor_probe import M, M_SOLVE, BENIGN_CAP, MEMBERS, batch, cases

pytestmark = pytest.mark.gpu

SIZES = S.SIZES
NAMES = ("L", "alpha", "partial", "logpdf")
LOG_2PI = np.log(8 * np.arctan(R.LD(1)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("P", (1, 3, 9))
@pytest.mark.parametrize("n", SIZES)
def test_backward_error_solve_partials_and_value(engine, n, P):
    labels, K, y, kap = batch(n)
    idx = list(MEMBERS[P])
    L, alpha, part, lp, info = engine.debug_series_factor(K[idx], y[idx])
    assert (info == 0).all(), info
    fails = []
    for j, i in enumerate(idx):
        fam = labels[i]
        assert np.array_equal(L[j], np.tril(L[j])), "L is not exactly lower triangular"
        cap = min(kap[i], BENIGN_CAP.get(fam, np.inf))
        # (a) backward error of the factor, and of the carried forward solve against the L it was computed with
        w = R.omega(K[i], L[j]) / R.gamma(n + 1)
        ws = R.omega_solve(L[j], alpha[j], y[i]) / R.gamma(n)
        print(f"n {n} P {P} {fam:9s}: omega/gamma {w:.4f} (M {M[fam]:.3f}) solve {ws:.4f} (M {M_SOLVE[fam]:.3f}) kappa_blk {kap[i]:.4g}")
        if not w <= min(M[fam], cap):
            fails.append(f"{fam}[{i}]: omega / gamma_(n+1) = {w:.4g} > min(M = {M[fam]:.4g}, cap = {cap:.4g})")
        if not ws <= min(M_SOLVE[fam], cap):
            fails.append(f"{fam}[{i}]: omega_solve / gamma_n = {ws:.4g} > min(M = {M_SOLVE[fam]:.4g}, cap = {cap:.4g})")
        # (b) the log-det partial against the returned diagonal: one 1-ulp log per term + the sum
        lg = 2 * np.log(np.diag(L[j]).astype(R.LD))
        if not abs(R.LD(part[j, 0]) - lg.sum()) <= R.gamma(n + 2) * np.abs(lg).sum():
            fails.append(f"{fam}[{i}]: logdet {part[j, 0]!r} vs {float(lg.sum())!r} (bound {float(R.gamma(n + 2) * np.abs(lg).sum()):.3g})")
        # ... alpha'alpha against the returned alpha
        aa = (alpha[j].astype(R.LD) ** 2).sum()
        if not abs(R.LD(part[j, 1]) - aa) <= R.gamma(n) * aa:
            fails.append(f"{fam}[{i}]: alpha'alpha {part[j, 1]!r} vs {float(aa)!r}")
        # ... and the value against the two partials: a rounded constant, a product and two sums
        want = -(n * LOG_2PI + R.LD(part[j, 0]) + R.LD(part[j, 1])) / 2
        tol = 4 * R.U * (n * LOG_2PI + abs(R.LD(part[j, 0])) + R.LD(part[j, 1]))
        if not abs(R.LD(lp[j]) - want) <= tol:
            fails.append(f"{fam}[{i}]: logpdf {lp[j]!r} vs {float(want)!r} (bound {float(tol):.3g})")
    assert not fails, "\n".join(fails)


def test_info_at_every_pivot_boundary(engine):
    """LAPACK's info = 1 + the first non-positive pivot, whichever 4-wide sub-step and 16-wide block it falls in; the value is NaN
    exactly where info != 0"""
    probes = S.info_probes() + [(batch(n)[1][0], 0, f"wishart({n})") for n in (1, 127, 129, 176)]
    wrong = []
    for K, want, name in probes:
        _, _, _, lp, info = engine.debug_series_factor(K[None], None)
        if info[0] != want:
            wrong.append(f"{name}: info {info[0]}, expected {want}")
        if np.isnan(lp[0]) != (info[0] != 0):
            wrong.append(f"{name}: logpdf {lp[0]} with info {info[0]}")
    assert not wrong, "\n".join(wrong)


def test_failed_matrices_are_isolated_and_runs_repeat(engine):
    """what logpdf_series_batch relies on with check=False: a failed particle changes no bit of its neighbours, whatever the batch"""
    n = S.N_CAP
    _, K, y, _ = batch(n)
    Kbad = np.array(K)
    Kbad[2] = R.indefinite(n, [5]); Kbad[8] = R.indefinite(n, [150], seed=1)
    good = [0, 1, 3, 4, 5, 6, 7]
    ref = engine.debug_series_factor(K, y)
    got = engine.debug_series_factor(Kbad, y)
    again = engine.debug_series_factor(Kbad, y)
    assert got[4].tolist() == [0, 0, 6, 0, 0, 0, 0, 0, 151]
    assert (ref[4] == 0).all()
    assert np.isnan(got[3][[2, 8]]).all() and np.isfinite(got[3][good]).all()
    for a, b, c, name in zip(ref, got, again, NAMES):
        assert np.array_equal(bits(a[good]), bits(b[good])), f"{name}: a failed matrix changed its neighbours"
        assert np.array_equal(bits(b), bits(c)), f"{name}: two identical calls differ"
    assert np.array_equal(got[4], again[4])
    for i in good:
        one = engine.debug_series_factor(K[i:i + 1], y[i:i + 1])
        assert one[4][0] == 0
        for a, b, name in zip(one, got, NAMES):
            assert np.array_equal(bits(a[0]), bits(b[i])), f"{name} of matrix {i}: batch of nine and P = 1 differ"


@pytest.mark.parametrize("n", (1, 17, 80, 129, 176))
def test_probe_is_the_production_code(pkg, engine, n):
    """on a covariance that is exact in float64 the production instantiations factor the very matrix the probe is given: the
    values agree bit for bit"""
    from oracle import oracle as O
    ts, particles = S.exact_particles(pkg, n)
    xs = np.random.default_rng(77 + n).standard_normal(n)
    for node, noise in particles:
        K = O.compute_cov_matrix_vectorized(node.to_tuple(), noise, ts)
        # precondition (a failure here means the inputs are not exact, not that the engine is wrong)
        assert np.array_equal(bits(K), bits(engine.cov_matrix(node, noise, ts))), "the covariance is not exact: choose other dyadic values"
        lp, info = engine.logpdf_series_batch([(ts, xs)], [node], [noise], [0])
        _, _, _, lp_probe, info_probe = engine.debug_series_factor(K[None], xs[None])
        assert info[0] == 0 and info_probe[0] == 0
        assert bits(lp_probe)[0] == bits(lp)[0], (n, type(node).__name__, lp_probe[0], lp[0])


def test_tile_schedules_and_series_kernel_factor_alike(engine):
    """one blocked LDS Cholesky (csrc/agp_lds_chol.hpp) behind both kernels: up to one tile (n <= 128) every tile schedule and the
    series kernel run the same statements on the same 16 x 16 blocks, and the tile's identity padding contributes exact zeros, so L,
    alpha and info agree bit for bit.  Sizes: a lone sub-block, a ragged block, a full block, a full block plus one, a look-ahead
    step, a ragged and a full tile.  (The partials are not compared: 128 and 256 logs summed in two fixed orders.)"""
    schedules = sorted({s for s, _, _ in cases()} - {3})      # (the hybrid rule is refused below three tile rows)
    assert schedules == [-1, 0, 1, 2, 4]
    differ = []
    for n in (1, 5, 16, 17, 33, 127, 128):
        _, K, y, _ = batch(n)
        idx = list(MEMBERS[3])
        Ls, als, _, _, infos = engine.debug_series_factor(K[idx], y[idx])
        for s in schedules:
            Lt, alt, _, infot = engine.debug_factor_batch(K[idx], y[idx], schedule=s)
            dL, da = int((bits(Ls) != bits(Lt)).sum()), int((bits(als) != bits(alt)).sum())
            print(f"n {n} schedule {s}: {dL} entries of L and {da} of alpha differ, info {infos.tolist()} / {infot.tolist()}")
            if dL or da or not np.array_equal(infos, infot):
                differ.append(f"n {n} schedule {s}: {dL} entries of L, {da} of alpha differ; info {infos.tolist()} vs {infot.tolist()}")
    assert not differ, "\n".join(differ)


def test_argument_errors(pkg, engine):
    cap = pkg.SERIES_MAX_N
    assert cap == S.N_CAP

    def valid():
        K = batch(17)[1][:1]
        L, _, _, _, info = engine.debug_series_factor(K, None)
        assert info[0] == 0 and R.omega(K[0], L[0]) <= 8 * R.gamma(18)      # (wishart: BENIGN_CAP)

    with pytest.raises(pkg.AGPError):
        engine.debug_series_factor(np.zeros((1, 0, 0)), None)
    valid()
    with pytest.raises(pkg.AGPError, match=str(cap)):
        engine.debug_series_factor(np.eye(cap + 1)[None], None)
    valid()
    n = 5
    out = (np.zeros((1, n, n)), np.zeros((1, n)), np.zeros((1, 2)), np.zeros(1))
    info = np.zeros(1, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    rc = engine._lib.agp_debug_series_factor(engine._ctx, None, None, n, 1, *(o.ctypes.data_as(dp) for o in out),
                                             info.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == -1
    with pytest.raises(pkg.AGPError, match="null"):
        engine._check(rc)
    valid()
