"""Every factorisation schedule of the batched Cholesky on caller-supplied matrices (GPEngine.debug_factor_batch): backward error
of L and of the fused forward solve, the log-det / quadratic-form partials against the L and beta they came from, LAPACK info at
every 4 / 16 / 128 pivot boundary, isolation of failed particles and run-to-run determinism.

Margins.  The engine multiplies by explicit inverses (reciprocal roots, 4 x 4 and 16 x 16 block inverses), so Higham's bounds
gamma_{n+1} (factor) and gamma_n (substitution) are met up to a factor M per family: 8 x the largest ratio omega / gamma measured on
an MI355X over all sizes and schedules (profiles/factor_probe_accuracy.txt, written by tools/gpu_factor_probe_accuracy.py; three
bits for reduction orders and compiler releases), at least 1 -- and never more than kappa_blk of the matrix at hand (the reference
factor's max || |L_bb^-1| |L_bb| ||_inf over its 16 x 16 diagonal blocks), nor than 8 for the two benign families: a schedule
that needs more loses more accuracy than its block inverses explain.  M and M_SOLVE below are that table's last lines.

The forward solve refines each 16-wide block solve once against the block (alpha += W (r - L alpha)), so its omega_solve is
substitution's (below 0.7 gamma_n everywhere) although the factor's omega reaches 145 gamma_(n+1) on se_grid at n = 300; without that
step it was 1.9 gamma_1 at n = 1 (cap 1) and 0.96 of the cap on se_irreg at n = 129."""
import numpy as np
import pytest

import _factor_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 16, 17, 127, 128, 129, 300)
# profiles/factor_probe_accuracy.txt: largest measured omega / gamma_{n+1} per family x 8, at least 1 ...
M = {"wishart": 5.021, "graded": 2.641, "spec": 21.448, "se_grid": 1163.76, "se_irreg": 424.153}
# ... and the same for omega_solve / gamma_n
M_SOLVE = {"wishart": 3.064, "graded": 1.883, "spec": 1.698, "se_grid": 1.357, "se_irreg": 5.393}
BENIGN_CAP = {"wishart": 8.0, "graded": 8.0}
PIVOTS = (0, 1, 2, 3, 4, 15, 16, 127, 128, 129, 255, 256, 299)
MEMBERS = {9: tuple(range(9)), 3: (2, 3, 4), 1: (3,)}      # of the batch of nine: all; spec, se_grid, se_irreg; se_grid

_CACHE = {}


def batch(n):
    """The batch of nine at size n with right-hand sides and kappa_blk of the reference factors (computed once, never modified)."""
    if n not in _CACHE:
        nine = R.batch_of_nine(n)
        K = np.stack([k for _, k in nine]); K.setflags(write=False)
        y = R.batch_rhs(n); y.setflags(write=False)
        kap = np.array([R.kappa_blk(R.ref_chol(k)) for k in K])
        _CACHE[n] = ([l for l, _ in nine], K, y, kap)
    return _CACHE[n]


def cases():
    out = [(s, n, P) for s in (0, 1, 2, 4) for n in SIZES for P in (1, 3, 9)]
    out += [(3, 300, P) for P in (1, 3, 9)]          # the hybrid rule needs three tile rows to switch
    out += [(-1, 300, 9), (-1, 300, 1)]              # what logpdf_batch runs at those sizes
    return out


@pytest.mark.parametrize("schedule, n, P", cases())
def test_backward_error_solve_and_partials(engine, schedule, n, P):
    labels, K, y, kap = batch(n)
    idx = list(MEMBERS[P])
    L, beta, part, info = engine.debug_factor_batch(K[idx], y[idx], schedule=schedule)
    assert (info == 0).all(), info
    fails = []
    for j, i in enumerate(idx):
        fam = labels[i]
        assert np.array_equal(L[j], np.tril(L[j])), "L is not exactly lower triangular"
        cap = min(kap[i], BENIGN_CAP.get(fam, np.inf))
        # (a) backward error of the factor
        w = R.omega(K[i], L[j]) / R.gamma(n + 1)
        # (b) the fused forward solve against the L it was computed with
        ws = R.omega_solve(L[j], beta[j], y[i]) / R.gamma(n)
        print(f"schedule {schedule} n {n} P {P} {fam:9s}: omega/gamma {w:.4f} (M {M[fam]:.3f}) solve {ws:.4f} (M {M_SOLVE[fam]:.3f}) "
              f"kappa_blk {kap[i]:.4g}")
        if not w <= min(M[fam], cap):
            fails.append(f"{fam}[{i}]: omega / gamma_(n+1) = {w:.4g} > min(M = {M[fam]:.4g}, cap = {cap:.4g})")
        if not ws <= min(M_SOLVE[fam], cap):
            fails.append(f"{fam}[{i}]: omega_solve / gamma_n = {ws:.4g} > min(M = {M_SOLVE[fam]:.4g}, cap = {cap:.4g})")
        # ... the log-det partial against the returned diagonal: one 1-ulp log per term + the sum
        lg = 2 * np.log(np.diag(L[j]).astype(R.LD))
        if not abs(R.LD(part[j, 0]) - lg.sum()) <= R.gamma(n + 2) * np.abs(lg).sum():
            fails.append(f"{fam}[{i}]: logdet {part[j, 0]!r} vs {float(lg.sum())!r} (bound {float(R.gamma(n + 2) * np.abs(lg).sum()):.3g})")
        # ... and beta'beta against the returned beta
        bb = (beta[j].astype(R.LD) ** 2).sum()
        if not abs(R.LD(part[j, 1]) - bb) <= R.gamma(n) * bb:
            fails.append(f"{fam}[{i}]: beta'beta {part[j, 1]!r} vs {float(bb)!r}")
    assert not fails, "\n".join(fails)


def test_margins_are_admissible():
    """M >= 1, and at most 8 for the benign families (the per-matrix cap kappa_blk is applied where the bound is used)"""
    for table in (M, M_SOLVE):
        assert set(table) == set(R.FAMILIES)
        for fam, m in table.items():
            assert 1.0 <= m <= BENIGN_CAP.get(fam, np.inf), (fam, m)


@pytest.mark.parametrize("schedule", (0, 1, 2, 3, 4, -1))
def test_info_at_every_pivot_boundary(engine, schedule):
    """LAPACK's info = 1 + the first non-positive pivot, whichever 4-wide sub-step, 16-wide block or 128-wide tile it falls in"""
    probes = [(R.indefinite(300, [j]), j + 1, f"indefinite(300, [{j}])") for j in PIVOTS]
    probes += [(R.indefinite(300, [129, 40]), 41, "indefinite(300, [129, 40])"), (R.indefinite(300, [16, 17]), 17, "indefinite(300, [16, 17])")]
    probes += [(R.zero_pivot(300, j), j + 1, f"zero_pivot(300, {j})") for j in (0, 128)]
    if schedule != 3:
        # the only real row of a ragged tile; padding rows are never reported
        probes += [(R.indefinite(129, [128]), 129, "indefinite(129, [128])"), (R.zero_pivot(129, 128), 129, "zero_pivot(129, 128)")]
        probes += [(batch(n)[1][0], 0, f"wishart({n})") for n in (1, 127, 129)]
    wrong = []
    for K, want, name in probes:
        _, _, _, info = engine.debug_factor_batch(K[None], None, schedule=schedule)
        if info[0] != want:
            wrong.append(f"{name}: info {info[0]}, expected {want}")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("schedule", (0, 1, 2, 3, 4))
def test_failed_particles_are_isolated_and_runs_repeat(engine, schedule):
    """what the sweeps rely on with check=False: a failed particle changes no bit of its neighbours, whatever the batch"""
    _, K, y, _ = batch(300)
    Kbad = np.array(K)
    Kbad[2] = R.indefinite(300, [5]); Kbad[8] = R.indefinite(300, [200], seed=1)
    good = [0, 1, 3, 4, 5, 6, 7]
    ref = engine.debug_factor_batch(K, y, schedule=schedule)
    got = engine.debug_factor_batch(Kbad, y, schedule=schedule)
    again = engine.debug_factor_batch(Kbad, y, schedule=schedule)
    assert got[3].tolist() == [0, 0, 6, 0, 0, 0, 0, 0, 201]
    assert (ref[3] == 0).all()
    names = ("L", "beta", "partial")
    for a, b, c, name in zip(ref, got, again, names):
        assert np.array_equal(a[good].view(np.uint64), b[good].view(np.uint64)), f"{name}: a failed particle changed its neighbours"
        assert np.array_equal(b[good].view(np.uint64), c[good].view(np.uint64)), f"{name}: two identical calls differ"
    assert np.array_equal(got[3], again[3])
    for i in good:
        one = engine.debug_factor_batch(K[i:i + 1], y[i:i + 1], schedule=schedule)
        assert one[3][0] == 0
        for a, b, name in zip(one, got, names):
            assert np.array_equal(a[0].view(np.uint64), b[i].view(np.uint64)), f"{name} of particle {i}: batch of nine and P = 1 differ"


def test_a_schedule_that_cannot_run_is_refused(pkg, engine):
    K = batch(128)[1][:1]
    with pytest.raises(pkg.AGPError, match="hybrid"):
        engine.debug_factor_batch(K, None, schedule=3)          # two tile rows at most: the hybrid rule never switches
    with pytest.raises(pkg.AGPError):
        engine.debug_factor_batch(K, None, schedule=5)
