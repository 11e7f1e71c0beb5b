"""Reference restatement of the predictive log-density (src/api.jl:686-699, test/experiment_hmc.jl:125):
logpdf(MvNormal(node, noise, ts, xs, ts_pred; noise_pred, mean), y) with the predictive built as src/GP.jl:731-758 builds it —
LU solves, 1/2 Sigma + 1/2 Sigma', + noise_pred I (oracle.predict_mvn) — and scored by an m x m Cholesky (oracle.mvnormal_logpdf).

reference() also returns the error scale S = m log 2pi + sum_i |2 log L_ii| + ||L^-1 (y - mu)||^2 of the result (the magnitudes of
the terms it is summed from); a device result is right when |lp - ref| <= tol S.  Two arbiters decide a miss: an mpmath twin
(n, m <= 40, oracle_mp.predict_mvn_mp) and a joint Cholesky in 80-bit arithmetic on the fp64 kernel values.
"""
import math

import numpy as np
import scipy.linalg as sla

from oracle import oracle as O

LOG2PI = math.log(2.0 * math.pi)


def _means(mean_train, mean_pred, n, m):
    mt = np.zeros(n) if mean_train is None else np.asarray(mean_train, dtype=np.float64)
    mp_ = np.zeros(m) if mean_pred is None else np.asarray(mean_pred, dtype=np.float64)
    return mt, mp_


def predictive(tree, noise, ts, xs, ts_pred, noise_pred=None, mean_train=None, mean_pred=None):
    """(mu*, Sigma*) of src/GP.jl:731-758; the mean function enters as its values at the training and query points."""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); ts_pred = np.asarray(ts_pred, dtype=np.float64)
    mt, mp_ = _means(mean_train, mean_pred, len(ts), len(ts_pred))
    mu, cov = O.predict_mvn(tree, noise, ts, xs - mt, ts_pred, noise_pred=noise_pred)
    return mp_ + mu, cov


def reference(tree, noise, ts, xs, ts_pred, y, noise_pred=None, mean_train=None, mean_pred=None):
    """(logpdf, S).  Raises oracle.PosDefException where the m x m factorisation fails."""
    y = np.asarray(y, dtype=np.float64)
    m = y.shape[0]
    if m == 0:
        return 0.0, 0.0
    mu, cov = predictive(tree, noise, ts, xs, ts_pred, noise_pred, mean_train, mean_pred)
    lp = O.mvnormal_logpdf(y, cov, mu)
    L = sla.cholesky(cov, lower=True, check_finite=False)
    a = sla.solve_triangular(L, y - mu, lower=True, check_finite=False)
    S = m * LOG2PI + float(np.sum(np.abs(2.0 * np.log(np.diag(L))))) + float(a @ a)
    return lp, S


def reference_mp(tree, noise, ts, xs, ts_pred, y, noise_pred=None, mean_train=None, mean_pred=None, dps=40):
    """The same in mpmath (n, m <= 40): predict_mvn_mp, then an m x m Cholesky at dps digits."""
    import mpmath as mp
    from oracle import oracle_mp as OM
    y = np.asarray(y, dtype=np.float64)
    m = y.shape[0]
    if m == 0:
        return 0.0
    mt, mp_ = _means(mean_train, mean_pred, len(ts), m)
    with mp.workdps(dps):
        mu, cov = OM.predict_mvn_mp(tree, noise, list(map(float, ts)), list(map(float, np.asarray(xs) - mt)), list(map(float, ts_pred)),
                                    noise_pred=noise_pred)
        C = mp.matrix(m, m)
        for i in range(m):
            for j in range(m):
                C[i, j] = (cov[i, j] + cov[j, i]) / 2
        L = mp.cholesky(C)
        d = mp.matrix([mp.mpf(float(y[i])) - mp.mpf(float(mp_[i])) - mu[i] for i in range(m)])
        a = mp.lu_solve(L, d)
        ld = 2 * mp.fsum(mp.log(L[i, i]) for i in range(m))
        ss = mp.fsum(a[i] ** 2 for i in range(m))
        return float(-(m * mp.log(2 * mp.pi) + ld + ss) / 2)


def reference_ld(tree, noise, ts, xs, ts_pred, y, noise_pred=None, mean_train=None, mean_pred=None):
    """80-bit arbiter: the joint matrix [K11 + noise I, K12; K21, K22 + noise_pred I] (fp64 kernel values) factored in long double,
    the query block's log-det and forward-solve norm."""
    ts = np.asarray(ts, dtype=np.float64); ts_pred = np.asarray(ts_pred, dtype=np.float64)
    n, m = len(ts), len(ts_pred)
    if m == 0:
        return 0.0
    noise_pred = noise if noise_pred is None else noise_pred
    mt, mp_ = _means(mean_train, mean_pred, n, m)
    K = O.compute_cov_matrix_vectorized(tree, 0.0, np.concatenate([ts, ts_pred])).astype(np.longdouble)
    N = n + m
    K[np.arange(n), np.arange(n)] += np.longdouble(noise)
    K[np.arange(n, N), np.arange(n, N)] += np.longdouble(noise_pred)
    r = np.concatenate([np.asarray(xs, dtype=np.float64) - mt, np.asarray(y, dtype=np.float64) - mp_]).astype(np.longdouble)
    L = np.zeros((N, N), dtype=np.longdouble)
    for j in range(N):
        d = K[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise O.PosDefException(j + 1)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    a = np.zeros(N, dtype=np.longdouble)
    for j in range(N):
        a[j] = (r[j] - L[j, :j] @ a[:j]) / L[j, j]
    ld = 2 * np.sum(np.log(np.diag(L)[n:]))
    return float(-(m * np.longdouble(LOG2PI) + ld + a[n:] @ a[n:]) / 2)


def arbiter(tree, noise, ts, xs, ts_pred, y, **kw):
    """The arbiter for a miss, or None above n + m = 300 (no arbiter: the fp64 reference decides)."""
    n, m = len(ts), len(ts_pred)
    if n <= 40 and m <= 40:
        return reference_mp(tree, noise, ts, xs, ts_pred, y, **kw)
    if n + m <= 300:
        return reference_ld(tree, noise, ts, xs, ts_pred, y, **kw)
    return None


def assert_close(lp, tree, noise, ts, xs, ts_pred, y, tol=1e-8, ctx=None, **kw):
    """|lp - ref| <= tol S; a miss is re-judged against the arbiter where there is one."""
    ref, S = reference(tree, noise, ts, xs, ts_pred, y, **kw)
    if abs(lp - ref) <= tol * S:
        return ref, S
    arb = arbiter(tree, noise, ts, xs, ts_pred, y, **kw)
    assert arb is not None and abs(lp - arb) <= tol * S, (ctx, lp, ref, arb, S)
    return ref, S
