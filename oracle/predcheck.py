"""PREDICTIVE CHECKER — TEST INFRASTRUCTURE ONLY (the sibling of oracle/gradcheck.py).

One assertion for every comparison of a predictive mean, marginal variance or covariance of the suite, output by output:

    |mean_j - m80_j|  <= mult R_mean sigma_j         + 4 eps S_mean_j
    |var_j  - v80_j|  <= mult R_var  v80_j           + 4 eps S_var_j
    |cov_ij - c80_ij| <= mult R_cov  sigma_i sigma_j + 4 eps S_cov_ij          sigma_j = sqrt(v80_j)

m80, v80, c80: the predictive of the particle with the factorisation, the solves and the sums in 80-bit arithmetic (np.longdouble)
on covariance entries the oracle evaluated in double.  The particle-wide criterion |d| <= 1e-8 max(1, max|ref|) says nothing about a
small output: at the model's noise floor (the jitter, 1e-5) the variance at a training time is 1e-7 .. 1e-5, for a kernel of amplitude
1e-4 everywhere, and quantiles, predictive log-densities and samples consume (y - mean) / sqrt(var).  This one measures each output
on its own scale, sigma_j for a mean and v80_j for a variance.

What a CORRECT double-precision implementation loses on that scale depends on the conditioning of the particle, so it is measured,
not assumed: R_mean, R_var and R_cov are the worst distance from the 80-bit values, in the norms above, of three double-precision
computations of the same outputs —
  * oracle.predict_mvn, the reference's order of operations (LU solves);
  * a LAPACK Cholesky route, v = L^-1 k, z = L^-1 (x - mean);
  * that Cholesky route on entries multiplied by 1 + 2 eps xi, xi symmetric and uniform in [-1, 1] from a fixed seed: a correct
    implementation whose covariance entries differ from the oracle's in the last places, which is what the device is.
The three differ among themselves by up to 14x per particle and R is the worst of them, so a fourth correct route is expected
within a small multiple of R: mult = 8, twice the 4x gradcheck allows its arbiter.  The term 4 eps S — S the sum of the magnitudes of
the terms of the output, S_mean_j = |mean_pred_j| + sum_a |v_aj| |z_a|, S_var_j = |k**_jj| + |noise_pred| + sum_a v_aj^2, S_cov_ij
likewise — covers the rounding of the output itself and of its last two additions; everything else the three routes do too.

Caps (not measurements: they keep an ill-conditioned particle from making the check vacuous): every particle used must have
R_mean <= CAP_R_MEAN and R_var <= CAP_R_VAR, a positive 80-bit variance everywhere and finite references.  A case that exceeds a cap
is replaced by another input; the caps are never raised.  The helper also asserts the suite's old criterion (against
oracle.predict_mvn), so nothing is relaxed.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
from threadpoolctl import threadpool_limits

from oracle import oracle as O

EPS = float(np.finfo(np.float64).eps)
MULT = 8.0
CAP_R_MEAN = 2e-5
CAP_R_VAR = 2e-7
OLD_TOL = 1e-8          # the suite's particle-wide criterion: |d| <= OLD_TOL max(1, max|ref|)
XI_SEED = 20261019
LD = np.longdouble


def _means(mean, ts, ts_pred):
    if mean is None:
        return np.zeros(ts.shape[0]), np.zeros(ts_pred.shape[0])
    return (np.array([mean(t) for t in ts], dtype=np.float64).reshape(ts.shape[0]),
            np.array([mean(t) for t in ts_pred], dtype=np.float64).reshape(ts_pred.shape[0]))


def _solve_80bit(K, n, noise, resid):
    """(V, z) = (L^-1 K12, L^-1 resid) with K11 + noise I = L L' factored and solved in np.longdouble; K: the joint matrix in double."""
    # right-looking on the rows of [K11 + noise I | K12 | resid]: row j becomes row j of [L' | V | z].  Whole-array operations only
    # (they release the GIL, so references() scales with its threads; a longdouble matrix product does not)
    K = K.astype(LD)
    W = np.concatenate([K[:n, :n] + LD(noise) * np.eye(n, dtype=LD), K[:n, n:], resid.astype(LD)[:, None]], axis=1)
    for j in range(n):
        W[j, j:] /= np.sqrt(W[j, j])
        w = W[j, j + 1:]
        W[j + 1:, j + 1:] -= w[:n - j - 1, None] * w[None, :]
    return W[:, n:-1], W[:, -1]


def _predict_80bit(K, n, noise, resid, mu2, noise_pred, cov, solved=None):
    """(m80, v80, c80 or None, V, z) in np.longdouble from the joint matrix K (double); solved: (V, z) computed before"""
    V, z = _solve_80bit(K, n, noise, resid) if solved is None else solved
    K22 = K[n:, n:].astype(LD)
    m80 = mu2.astype(LD) + V.T @ z
    v80 = np.diag(K22) - (V ** 2).sum(axis=0) + LD(noise_pred)
    c80 = K22 - V.T @ V + LD(noise_pred) * np.eye(K.shape[0] - n, dtype=LD) if cov else None
    return m80, v80, c80, V, z


def predict_80bit(tree, noise, ts, xs, ts_pred, noise_pred, mean=None, cov=False):
    """Predictive mean and marginal variance (and the covariance with cov=True) with the factorisation, the solves and the sums in
    80-bit arithmetic (covariance entries from the oracle in double), rounded to double: the judge where the conditioning leaves
    double-precision passes only 1e-9."""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); ts_pred = np.asarray(ts_pred, dtype=np.float64)
    n = ts.shape[0]
    K = O.compute_cov_matrix_vectorized(tree, 0.0, np.concatenate([ts, ts_pred]))
    mu1, mu2 = _means(mean, ts, ts_pred)
    out = _predict_80bit(K, n, noise, xs - mu1, mu2, noise_pred, cov)[:3 if cov else 2]
    return tuple(a.astype(np.float64) for a in out)


def cholesky_route(K, n, noise, resid, mu2, noise_pred, cov=False):
    """The LAPACK Cholesky route on the joint matrix K (double): (mean, var, cov or None)."""
    m = K.shape[0] - n
    if n == 0:
        V = np.zeros((0, m)); z = np.zeros(0)
    else:
        L = np.linalg.cholesky(K[:n, :n] + noise * np.eye(n))
        V = sla.solve_triangular(L, K[:n, n:], lower=True, check_finite=False)
        z = sla.solve_triangular(L, resid, lower=True, check_finite=False)
    mean = mu2 + V.T @ z
    var = (np.diag(K[n:, n:]) - (V * V).sum(axis=0)) + noise_pred
    c = (K[n:, n:] - V.T @ V) + noise_pred * np.eye(m) if cov else None
    return mean, var, c


def perturbed_entries(K, seed=XI_SEED):
    """K's entries multiplied by 1 + 2 eps xi, xi symmetric and uniform in [-1, 1]."""
    xi = np.random.default_rng(seed).uniform(-1.0, 1.0, K.shape)
    xi = np.triu(xi) + np.triu(xi, 1).T
    return K * (1.0 + 2.0 * EPS * xi)


class PredRef:
    """The 80-bit predictive of one particle, the distance R of three correct double-precision routes from it and the sums of
    magnitudes S of every output's terms (see the module docstring).  want_cov: also c80, R_cov and S_cov."""

    def __init__(self, tree, noise, ts, xs, ts_pred, noise_pred, mean=None, want_cov=False, solved=None):
        self.tree, self.noise, self.noise_pred = tree, float(noise), float(noise_pred)
        ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); tp = np.asarray(ts_pred, dtype=np.float64)
        self.n, self.m = n, m = ts.shape[0], tp.shape[0]
        K = O.compute_cov_matrix_vectorized(tree, 0.0, np.concatenate([ts, tp]))
        mu1, mu2 = _means(mean, ts, tp)
        resid = xs - mu1
        m80, v80, c80, V, z = _predict_80bit(K, n, self.noise, resid, mu2, self.noise_pred, want_cov, solved)      # (solved: references()' threads)
        aV = np.abs(V).astype(np.float64)
        self.S_mean = np.abs(mu2) + aV.T @ np.abs(z).astype(np.float64)
        self.S_var = np.abs(np.diag(K[n:, n:])) + abs(self.noise_pred) + (aV * aV).sum(axis=0)
        self.S_cov = np.abs(K[n:, n:]) + abs(self.noise_pred) * np.eye(m) + aV.T @ aV if want_cov else None
        self._m80, self._v80, self._c80 = m80, v80, c80
        self.m80, self.v80 = m80.astype(np.float64), v80.astype(np.float64)
        self.c80 = None if c80 is None else c80.astype(np.float64)
        self.finite = bool(np.isfinite(self.m80).all() and np.isfinite(self.v80).all() and (self.v80 > 0).all())
        with np.errstate(invalid="ignore"):
            self.sigma = np.sqrt(np.where(self.v80 > 0, self.v80, np.nan))
        self.sig2 = np.outer(self.sigma, self.sigma)
        # the three double-precision routes
        mu_lu, cov_lu = O.predict_mvn(tree, self.noise, ts, xs, tp, noise_pred=self.noise_pred, mean=mean)
        self.mean_lu, self.var_lu = mu_lu, np.diag(cov_lu).copy()
        self.cov_lu = cov_lu if want_cov else None
        self.old_scale_mean = max(1.0, float(np.abs(mu_lu).max())) if m else 1.0
        self.old_scale_var = max(1.0, float(np.abs(cov_lu).max())) if m else 1.0
        self.finite = self.finite and bool(np.isfinite(mu_lu).all() and np.isfinite(cov_lu).all())
        routes = [(mu_lu, self.var_lu, cov_lu if want_cov else None),
                  cholesky_route(K, n, self.noise, resid, mu2, self.noise_pred, want_cov),
                  cholesky_route(perturbed_entries(K), n, self.noise, resid, mu2, self.noise_pred, want_cov)]
        self.route_dist = [self.distance(*r) for r in routes]          # per route: (mean, var, cov) in the R norms
        self.R_mean = max(d[0] for d in self.route_dist)
        self.R_var = max(d[1] for d in self.route_dist)
        self.R_cov = max(d[2] for d in self.route_dist) if want_cov else None

    def distance(self, mean, var, cov=None):
        """(max_j |mean - m80|_j / sigma_j, max_j |var - v80|_j / v80_j, max_ij |cov - c80|_ij / (sigma_i sigma_j) or None)"""
        if self.m == 0:
            return 0.0, 0.0, (0.0 if cov is not None else None)
        dm = float(np.max(np.abs(np.asarray(mean) - self._m80).astype(np.float64) / self.sigma))
        dv = float(np.max(np.abs(np.asarray(var) - self._v80).astype(np.float64) / self.v80))
        dc = None
        if cov is not None and self._c80 is not None:
            dc = float(np.max(np.abs(np.asarray(cov) - self._c80).astype(np.float64) / self.sig2))
        return dm, dv, dc

    def ratios(self, mean, var, cov=None):
        """distance(...) divided by (R_mean, R_var, R_cov): what assert_predictive returns where it accepts"""
        ratio = lambda d, R: None if d is None else 0.0 if d == 0.0 else (d / R if R > 0 else np.inf)
        dm, dv, dc = self.distance(mean, var, cov)
        return ratio(dm, self.R_mean), ratio(dv, self.R_var), ratio(dc, self.R_cov)

    def needed_mult(self, mean, var, cov=None):
        """the smallest mult at which assert_predictive's bounds hold for (mean, var, cov): max over the outputs of
        (|d| - 4 eps S) / (R scale), 0 where the 4 eps S term alone covers every output"""
        em, ev, ec = self.errors(mean, var, cov)
        need = [np.max((em - 4.0 * EPS * self.S_mean) / (self.R_mean * self.sigma)), np.max((ev - 4.0 * EPS * self.S_var) / (self.R_var * self.v80))]
        if cov is not None:
            need.append(np.max((ec - 4.0 * EPS * self.S_cov) / (self.R_cov * self.sig2)))
        return max(0.0, float(max(need)))

    def bounds(self, mult=MULT):
        """(bound_mean[m], bound_var[m], bound_cov[m, m] or None)"""
        bm = mult * self.R_mean * self.sigma + 4.0 * EPS * self.S_mean
        bv = mult * self.R_var * self.v80 + 4.0 * EPS * self.S_var
        bc = None if self.S_cov is None else mult * self.R_cov * self.sig2 + 4.0 * EPS * self.S_cov
        return bm, bv, bc

    def errors(self, mean, var, cov=None):
        """|device - 80-bit| per output (double)"""
        em = np.abs(np.asarray(mean, dtype=np.float64) - self._m80).astype(np.float64)
        ev = np.abs(np.asarray(var, dtype=np.float64) - self._v80).astype(np.float64)
        ec = None if cov is None else np.abs(np.asarray(cov, dtype=np.float64) - self._c80).astype(np.float64)
        return em, ev, ec


def _one_blas_thread():
    """LAPACK on one thread while the references are computed: at n <= 420 its worker threads cost five times what they save, and R
    (which moves by some 20 % with LAPACK's summation order) then does not depend on how many of them the machine has"""
    return threadpool_limits(limits=1, user_api="blas")


def reference(tree, noise, ts, xs, ts_pred, noise_pred, mean=None, want_cov=False):
    with _one_blas_thread():
        return PredRef(tree, noise, ts, xs, ts_pred, noise_pred, mean=mean, want_cov=want_cov)


def references(nodes, noises, ts, xs, ts_pred, noise_pred, mean=None, want_cov=False, threads=8):
    """PredRef of every (node, noise, noise_pred) of a population on one series and one query set (nodes: oracle trees or objects
    with .to_tuple(); noise_pred: a scalar or one per particle).  The 80-bit solves run in threads (whole-array operations: they release the GIL).  Nothing is caught: a particle whose reference cannot be computed is the caller's to replace."""
    from concurrent.futures import ThreadPoolExecutor
    trees = [t if isinstance(t, tuple) else t.to_tuple() for t in nodes]
    npred = np.broadcast_to(np.asarray(noise_pred, dtype=np.float64), (len(trees),))

    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); tp = np.asarray(ts_pred, dtype=np.float64)
    tall = np.concatenate([ts, tp])
    resid = xs - _means(mean, ts, tp)[0]

    def solve(a):
        return _solve_80bit(O.compute_cov_matrix_vectorized(a[0], 0.0, tall), ts.shape[0], float(a[1]), resid)
    with ThreadPoolExecutor(threads) as ex:
        solved = list(ex.map(solve, zip(trees, noises)))
    # (the double-precision routes one after the other)
    with _one_blas_thread():
        return [PredRef(t, float(nz), ts, xs, tp, float(npd), mean=mean, want_cov=want_cov, solved=sv)
                for t, nz, npd, sv in zip(trees, noises, npred, solved)]


def assert_caps(ref, ctx=None):
    """The conditions under which the check means something (module docstring)."""
    assert ref.finite, (ctx, "reference not finite or a variance not positive", float(np.min(ref.v80)) if ref.m else None)
    assert ref.R_mean <= CAP_R_MEAN, (ctx, "R_mean", ref.R_mean, "above the cap", CAP_R_MEAN, "- choose another input")
    assert ref.R_var <= CAP_R_VAR, (ctx, "R_var", ref.R_var, "above the cap", CAP_R_VAR, "- choose another input")


def passes_old_criterion(mean, var, ref, cov=None):
    """The suite's particle-wide criterion against oracle.predict_mvn: |d| <= 1e-8 max(1, max|ref|), the variance (and the
    covariance) on the scale of the largest entry of the predictive covariance."""
    mean = np.asarray(mean, dtype=np.float64); var = np.asarray(var, dtype=np.float64)
    if ref.m == 0:
        return mean.size == 0 and var.size == 0
    ok = np.isfinite(mean).all() and np.isfinite(var).all()
    ok = ok and np.abs(mean - ref.mean_lu).max() <= OLD_TOL * ref.old_scale_mean
    ok = ok and np.abs(var - ref.var_lu).max() <= OLD_TOL * ref.old_scale_var
    if cov is not None:
        ok = ok and np.abs(np.asarray(cov, dtype=np.float64) - ref.cov_lu).max() <= OLD_TOL * ref.old_scale_var
    return bool(ok)


class BoundMiss(AssertionError):
    """an output further from its 80-bit value than its bound (every other assertion of the helper is a plain AssertionError)"""


def _worst(err, bound, what, ctx, extra):
    miss = ~(err <= bound)
    if miss.any():
        k = np.unravel_index(int(np.argmax(np.where(miss, err / bound, 0.0))), err.shape)
        raise BoundMiss((ctx, what, "outputs over the bound", int(miss.sum()), "worst at", tuple(int(i) for i in k),
                              "|d|", float(err[k]), "bound", float(bound[k]), "|d| / bound", float(err[k] / bound[k]), *extra))


def assert_predictive(mean, var, ref, cov=None, mult=MULT, ctx=None):
    """Assert a predictive (mean[m], var[m], optionally cov[m, m]) of ref's particle output by output (module docstring), the caps
    on ref and the suite's old criterion.  Returns the worst accepted ratios (r_mean, r_var, r_cov): the distance from the 80-bit
    values in the R norms divided by R_mean, R_var, R_cov (r_cov None without cov)."""
    assert_caps(ref, ctx)
    mean = np.asarray(mean, dtype=np.float64); var = np.asarray(var, dtype=np.float64)
    assert mean.shape == (ref.m,) and var.shape == (ref.m,), (ctx, mean.shape, var.shape, ref.m)
    assert np.isfinite(mean).all() and np.isfinite(var).all(), (ctx, "not finite")
    if cov is not None:
        assert ref.c80 is not None, (ctx, "reference built without want_cov")
        cov = np.asarray(cov, dtype=np.float64)
        assert cov.shape == (ref.m, ref.m) and np.isfinite(cov).all(), (ctx, cov.shape)
    if ref.m == 0:
        return 0.0, 0.0, (0.0 if cov is not None else None)
    em, ev, ec = ref.errors(mean, var, cov)
    bm, bv, bc = ref.bounds(mult)
    dm, dv, dc = ref.distance(mean, var, cov)
    _worst(em, bm, "mean", ctx, ("R_mean", ref.R_mean, "distance / R_mean", dm / ref.R_mean if ref.R_mean else np.inf))
    _worst(ev, bv, "variance", ctx, ("R_var", ref.R_var, "distance / R_var", dv / ref.R_var if ref.R_var else np.inf))
    if cov is not None:
        _worst(ec, bc, "covariance", ctx, ("R_cov", ref.R_cov, "distance / R_cov", dc / ref.R_cov if ref.R_cov else np.inf))
    assert passes_old_criterion(mean, var, ref, cov), (ctx, "the particle-wide criterion",
                                                       float(np.abs(mean - ref.mean_lu).max() / ref.old_scale_mean),
                                                       float(np.abs(var - ref.var_lu).max() / ref.old_scale_var))
    return ref.ratios(mean, var, cov)
