"""The slab loops of the MFMA K-loops (chol_tile, gemm_slabs) at sizes that span short and long trip counts.  The loops are
unrolled by two with a peeled tail (the last pair of slabs: one that still prefetches, one that does not), so what can go wrong is
the trip structure: a slab multiplied twice or not at all, a staging buffer read before its store, the last slab taken from the
wrong register set.

  factorisation   n = 641 (six tile rows: K-loops of 8 .. 40 slabs, the main loop runs 3 .. 19 times before the tail), members
                  (2, 3, 4) of the batch of nine, schedules 0 mixed, 1 split, 3 hybrid, 4 dataflow: backward error of L and of the
                  fused forward solve as tests/test_gpu_factor_probe.py computes them
  gemm_slabs      the element-wise gradient (k_trtri_chain, k_kinv_tiles) at n = 385 on irregular times, against the oracle
  Schur pass      predict_batch at n = 257 with 300 off-lattice queries (k_chol_update<false, ...>), against the oracle

Margins of the factorisation: 8 x the largest omega / gamma_(n+1) (omega_solve / gamma_n) that tools/gpu_factor_probe_accuracy.py
measured at n = 641 on an MI355X with the library of the commit BEFORE the slab loops were changed (the rows "n = 641" appended to
profiles/factor_probe_accuracy.txt), at least 1, and never more than kappa_blk of the matrix at hand."""
import numpy as np
import pytest

import _factor_ref as R
from oracle import gradcheck as GC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_FACTOR = 641
MEMBERS = (2, 3, 4)                   # spec, se_grid, se_irreg
SCHEDULES = (0, 1, 3, 4)
# profiles/factor_probe_accuracy.txt, "n = 641, members 2,3,4": max(1, 8 x largest omega / gamma_(n+1)) ...
M = {"spec": 1.0, "se_grid": 78.527, "se_irreg": 17.373}
# ... and max(1, 8 x largest omega_solve / gamma_n)
M_SOLVE = {"spec": 1.0, "se_grid": 1.0, "se_irreg": 1.0}
GRAD_TOL = 1e-7
PRED_TOL = 1e-8

_CACHE = {}


def factor_inputs():
    """members (2, 3, 4) of the batch of nine at n = 641, right-hand sides and kappa_blk of the reference factors (once, read-only)"""
    if "in" not in _CACHE:
        nine = R.batch_of_nine(N_FACTOR)
        idx = list(MEMBERS)
        K = np.stack([nine[i][1] for i in idx]); K.setflags(write=False)
        y = R.batch_rhs(N_FACTOR)[idx]; y.setflags(write=False)
        kap = np.array([R.kappa_blk(R.ref_chol(k)) for k in K])
        _CACHE["in"] = ([nine[i][0] for i in idx], K, y, kap)
    return _CACHE["in"]


def factored(engine, schedule):
    """one debug_factor_batch call per schedule on the three matrices together, shared by that schedule's cases"""
    if schedule not in _CACHE:
        _, K, y, _ = factor_inputs()
        _CACHE[schedule] = engine.debug_factor_batch(K, y, schedule=schedule)
    return _CACHE[schedule]


@pytest.mark.parametrize("member", range(len(MEMBERS)))
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_factorisation_six_tile_rows(engine, schedule, member):
    labels, K, y, kap = factor_inputs()
    L, beta, part, info = factored(engine, schedule)
    assert (info == 0).all(), info
    n, j, fam = N_FACTOR, member, labels[member]
    assert np.array_equal(L[j], np.tril(L[j])), "L is not exactly lower triangular"
    w = R.omega(K[j], L[j]) / R.gamma(n + 1)
    ws = R.omega_solve(L[j], beta[j], y[j]) / R.gamma(n)
    print(f"schedule {schedule} n {n} {fam:9s}: omega/gamma {w:.4f} (M {M[fam]:.3f}) solve {ws:.4f} (M {M_SOLVE[fam]:.3f}) kappa_blk {kap[j]:.4g}")
    assert w <= min(M[fam], kap[j]), f"{fam}: omega / gamma_(n+1) = {w:.4g} > min(M = {M[fam]:.4g}, cap = {kap[j]:.4g})"
    assert ws <= min(M_SOLVE[fam], kap[j]), f"{fam}: omega_solve / gamma_n = {ws:.4g} > min(M = {M_SOLVE[fam]:.4g}, cap = {kap[j]:.4g})"


def test_margins_are_admissible():
    for table in (M, M_SOLVE):
        assert set(table) == {"spec", "se_grid", "se_irreg"} and all(m >= 1.0 for m in table.values())


def irregular_series(n, seed):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.random(n))
    ts[n // 2] = ts[n // 2 - 1]              # a duplicated time
    xs = 0.5 * rng.standard_normal(n) + np.sin(6 * ts)
    return ts, xs


def test_elementwise_gradient_four_tile_rows(pkg):
    """n = 385: four tile rows, so k_trtri_chain's sums run over 8 .. 24 slabs and k_kinv_tiles' over 8 .. 32 (the last tile row
    holds one real point); one-leaf and three-leaf trees, the lag domain off"""
    G = pkg
    n = 385
    ts, xs = irregular_series(n, seed=385)
    kernels = [G.SquaredExponential(0.3, 1.0),
               G.GammaExponential(0.2, 1.3, 0.9) + G.Periodic(0.8, 0.25, 0.6) * G.Linear(0.3, 0.2, 0.7),
               G.SquaredExponential(0.15, 0.8) * G.Linear(0.6, 0.1, 0.5) + G.Periodic(0.9, 0.11, 0.4)]
    assert [k.size() for k in kernels] == [1, 5, 5]          # 1 and 3 leaves
    noises = np.array([0.1, 0.02, 0.3])
    e = pkg.GPEngine(0)
    try:
        e.set_grad_lag_domain(False)
        e.set_data(ts, xs)
        lp, grads, gn, info = e.logpdf_grad_batch(kernels, noises)
        assert (info == 0).all(), info
        assert e.grad_lag_domain_particles() == 0
        for k, nz, l, g, gnz in zip(kernels, noises, lp, grads, gn):
            lpo, go, gno = O.gp_logpdf_grad(k.to_tuple(), float(nz), ts, xs)
            sc = max(1.0, np.abs(go).max(), abs(gno))
            print(f"[kloop grad] {k}: |g - ref| / scale = {max(np.abs(g - go).max(), abs(gnz - gno)) / sc:.3e}")
            assert abs(l - lpo) <= 1e-8 * max(1.0, abs(lpo))
            assert g.shape == go.shape
            assert np.abs(g - go).max() <= GRAD_TOL * sc, (k, g, go)
            assert abs(gnz - gno) <= GRAD_TOL * sc, k
            GC.assert_grad_components(g, gnz, GC.reference(k.to_tuple(), float(nz), ts, xs), ctx=(n, k))
    finally:
        e.close()


def test_schur_pass_off_lattice_queries(pkg):
    """n = 257 training points (three tile rows) and 300 query points (three more) away from the series' grid: the predictive
    blocks are updated by the non-factoring K-loop over 24 slabs of training columns"""
    G = pkg
    n, m = 257, 300
    ts, xs = pkg.prior.synthetic_series(n, seed=11)
    rng = np.random.default_rng(300)
    tp = np.sort(rng.uniform(0.0, 1.2, m))
    kernels = [G.SquaredExponential(0.3, 1.0),
               G.GammaExponential(0.2, 1.3, 0.9) + G.Periodic(0.8, 0.25, 0.6) * G.Linear(0.3, 0.2, 0.7),
               G.SquaredExponential(0.15, 0.8) * G.Linear(0.6, 0.1, 0.5) + G.Periodic(0.9, 0.11, 0.4)]
    noises = np.array([0.1, 0.05, 0.3])
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        mean, var, cov, info = e.predict_batch(kernels, noises, tp, want_cov=True)
        assert (np.asarray(info) == 0).all(), info
        for i, (k, nz) in enumerate(zip(kernels, noises)):
            mu, cv = O.predict_mvn(k.to_tuple(), float(nz), ts, xs, tp)
            e1 = np.abs(mean[i] - mu).max() / max(1.0, np.abs(mu).max())
            e2 = np.abs(var[i] - np.diag(cv)).max() / max(1.0, np.abs(cv).max())
            e3 = np.abs(cov[i] - cv).max() / max(1.0, np.abs(cv).max())
            print(f"[kloop predict] {k}: mean {e1:.2e} var {e2:.2e} cov {e3:.2e}")
            assert e1 <= PRED_TOL and e2 <= PRED_TOL and e3 <= PRED_TOL, (k, e1, e2, e3)
    finally:
        e.close()
