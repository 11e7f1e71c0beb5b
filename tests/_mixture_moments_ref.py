"""Restatement of the mixture moments (agp_mixture_moments / agp_predict_mixture_batch; Distributions.mean / var / cov of a
MixtureModel of MvNormal or MvLogNormal components) in exact arithmetic, the error bounds the device results are held to, and the
generator of the test mixtures.

The mixture is that of the probabilities w / sum(w): isprobvec admits sum(w) = 1 +- sqrt(eps), and the moments of a distribution do
not move with a shift of its support only for normalised weights (the device's sums about a pivot are shift-invariant by construction:
with W = sum(w) they differ from the moments under w / W by (W - 1) times the quantities the bounds below are made of).

space 0: every double is an integer multiple of 2^-K; the sums  B = sum W MU,  A = sum W (C 2^K + MU MU'),  SW = sum W  are exact
  Python integers and  mean = B / (SW 2^K),  cov = (A SW - B B') / (SW^2 2^2K)  are rounded once (fractions.Fraction -> float).
  math.fsum (exactly rounded) gives the weighted absolute sums the bounds need.
space 1: mpmath at 200 bits: e_i = exp(mu_i + C_ii / 2), C'_ij = e_i e_j expm1(C_ij) (Distributions' MvLogNormal; the reference's
  Transforms.unapply_mean_var(::LogTransform) on the diagonal), then the same moments.

Bounds (eps = 2^-52), with ebar the exact mean and r_i = max over positive-weight p of |e_p,i - ebar_i|:
  mean  |d_i|  <= 4 (P + 8) eps sum w_p |e_p,i - ebar_i| + eps |ebar_i|
  cov   |d_ij| <= 8 (P + 8) eps (sum w_p |C_p,ij| + 4 r_i r_j)              (any admissible pivot is within 2 r of every mean)
space 1 adds the elementwise errors of the device functions: e_dev = e (1 + de), |de| <= (EXP_ULP_DEV + |arg| / 2) eps (exp_f, and
the rounding of its argument fma(0.5, C_ii, mu)); a log-normal covariance term e_i e_j expm1(c) carries de_i + de_j + (EXPM1_ULP_DEV +
2) eps (two products); and moving every e_p,i by eps_p,i = e_p,i de_p,i moves cov_ij by
sum w (eps_p,i |e_p,j - ebar_j| + |e_p,i - ebar_i| eps_p,j + eps_p,i eps_p,j) (the shifts of ebar cancel: sum w (e - ebar) = 0).
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
LP_TOL = 1e-8             # agreement the suite demands between two predictive paths (tests/test_gpu_predict_logpdf.py)
# elementwise error bounds (ulps) of the device functions the log-normal components call: exp_f is documented at <~ 1.5 ulp
# (csrc/agp_math.hpp), the device library's expm1 at 1 ulp; tests/test_gpu_mixture_moments.py::test_device_exp_and_expm1_bounds
# measures both through GPEngine.debug_math (which = 0 and 9) against mpmath and holds them to these constants.  Measured on an
# MI355X (profiles/predict_mixture_perf.txt): exp_f 0.587 ulp, expm1 1.048 ulp
# (largest of the test's and the tool's argument sets; exp_f up to 709.78, where exp overflows).
EXP_ULP_DEV = 2.0
EXPM1_ULP_DEV = 2.0


def ulp_err(got, x, fn, dps=40):
    """max |got - fn(x)| in ulps (eps |fn(x)|) over the arrays, fn an mpmath function."""
    worst = 0.0
    with mp.workdps(dps):
        for g, v in zip(np.asarray(got, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64).ravel()):
            t = fn(mp.mpf(float(v)))
            if t == 0:
                assert g == 0.0, (v, g)
                continue
            worst = max(worst, float(abs(mp.mpf(float(g)) - t) / (abs(t) * mp.mpf(EPS))))
    return worst


def _to_int(a, K):
    """float64 array -> object array of Python ints a * 2^K (exact; K large enough for every element)."""
    a = np.asarray(a, dtype=np.float64)
    mant, ex = np.frexp(a)
    mi = (mant * 2.0 ** 53).astype(np.int64).astype(object)
    sh = ex.astype(np.int64) - 53 + K
    assert (sh[a != 0] >= 0).all()
    return mi * np.power(2, np.maximum(sh, 0).astype(object))


def _scale(*arrays):
    K = 0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        nz = a[a != 0]
        if nz.size:
            K = max(K, 53 - int(np.frexp(nz)[1].min()))
    return K


def _pairs(m, pairs):
    if pairs is None:
        return [(i, j) for j in range(m) for i in range(j, m)]
    return [(max(i, j), min(i, j)) for i, j in pairs]


def moments(means, weights, vars=None, covs=None, space=0, pairs=None):
    """Exact moments and bounds.  means (P, m); vars (P, m) or covs (P, m, m); weights (P,).  Returns a dict: mean, var (m,),
    mean_bound, var_bound (m,), and with covs: pairs [(i, j), i >= j], cov / cov_bound (values per pair) and cov_full (m, m; NaN where
    no pair was asked for).  `pairs` (default: the whole lower triangle) limits the covariance elements evaluated."""
    means = np.asarray(means, dtype=np.float64); w = np.asarray(weights, dtype=np.float64)
    P, m = means.shape
    if covs is not None:
        covs = np.asarray(covs, dtype=np.float64)
        vars = np.einsum("pii->pi", covs).copy()
    vars = np.asarray(vars, dtype=np.float64)
    pr = _pairs(m, pairs) if covs is not None else []
    return (_moments_normal if space == 0 else _moments_lognormal)(means, w, vars, covs, pr, P, m)


def _finish(out, covs, pr, m):
    if covs is not None:
        full = np.full((m, m), np.nan)
        for (i, j), v in zip(pr, out["cov"]):
            full[i, j] = full[j, i] = v
        out["pairs"] = pr
        out["cov_full"] = full
    return out


def _moments_normal(means, w, vars, covs, pr, P, m):
    K = _scale(means, w, vars if covs is None else covs)
    W = _to_int(w, K); MU = _to_int(means, K); V = _to_int(vars, K)
    SW = int(W.sum())
    B = [int(sum(int(W[p]) * int(MU[p, i]) for p in range(P))) for i in range(m)]
    mean_q = [Fraction(B[i], SW << K) for i in range(m)]
    mean = np.array([float(q) for q in mean_q])
    pos = np.flatnonzero(w > 0)
    wn = w / math.fsum(w)
    dev = np.array([[float(Fraction(float(means[p, i])) - mean_q[i]) for i in range(m)] for p in range(P)]).reshape(P, m)
    r = np.abs(dev[pos]).max(axis=0) if m else np.zeros(0)
    sabs = np.array([math.fsum(wn[p] * abs(dev[p, i]) for p in range(P)) for i in range(m)])
    den = (SW * SW) << (2 * K)

    Bo = np.array(B, dtype=object)

    def elements(I, J, Cint):
        """exact values at the index lists (I, J); Cint (P, len(I)) the components' integer entries there"""
        A = np.zeros(len(I), dtype=object)
        for p in range(P):
            A = A + int(W[p]) * (Cint[p] * (1 << K) + MU[p][I] * MU[p][J])
        N = A * SW - Bo[I] * Bo[J]
        return np.array([float(Fraction(int(v), den)) for v in N])

    ar = np.arange(m)
    var = elements(ar, ar, V) if m else np.zeros(0)
    out = {"mean": mean, "var": var,
           "mean_bound": 4 * (P + 8) * EPS * sabs + EPS * np.abs(mean),
           "var_bound": 8 * (P + 8) * EPS * (np.abs(vars).T @ wn + 4 * r * r)}
    if covs is not None:
        I = np.array([i for i, _ in pr], dtype=np.int64); J = np.array([j for _, j in pr], dtype=np.int64)
        out["cov"] = elements(I, J, _to_int(covs[:, I, J], K))
        out["cov_bound"] = 8 * (P + 8) * EPS * (np.abs(covs[:, I, J]).T @ wn + 4 * r[I] * r[J])
    return _finish(out, covs, pr, m)


def _moments_lognormal(means, w, vars, covs, pr, P, m):
    with mp.workprec(200):
        wq = [mp.mpf(float(v)) for v in w]
        sw = mp.fsum(wq)
        wq = [v / sw for v in wq]
        pos = [p for p in range(P) if w[p] > 0]
        arg = means + 0.5 * vars                                    # (magnitudes for the bound only)
        e = [[mp.exp(mp.mpf(float(means[p, i])) + mp.mpf(float(vars[p, i])) / 2) for i in range(m)] for p in range(P)]
        ebar = [mp.fsum(wq[p] * e[p][i] for p in pos) for i in range(m)]
        de = (EXP_ULP_DEV + 0.5 * np.abs(arg)) * EPS                # (P, m) relative error of the device's e
        ef = np.array([[float(e[p][i]) for i in range(m)] for p in range(P)]).reshape(P, m)
        dev = np.array([[float(abs(e[p][i] - ebar[i])) for i in range(m)] for p in range(P)]).reshape(P, m)
        wf = np.array([float(v) for v in wq])
        epsf = ef * de
        r = dev[pos].max(axis=0) if m else np.zeros(0)

        def em1(x):
            return mp.expm1(mp.mpf(float(x))) if x != 0.0 else mp.mpf(0)

        def element(i, j, c):
            t = [e[p][i] * e[p][j] * em1(c[p]) for p in range(P)]
            v = mp.fsum(wq[p] * (t[p] + (e[p][i] - ebar[i]) * (e[p][j] - ebar[j])) for p in pos)
            tabs = np.array([float(abs(x)) for x in t])
            b = 8 * (P + 8) * EPS * (float(np.dot(wf[pos], tabs[pos])) + 4 * r[i] * r[j])
            b += float(np.dot(wf[pos], tabs[pos] * (de[pos, i] + de[pos, j] + (EXPM1_ULP_DEV + 2) * EPS)))
            b += float(np.dot(wf[pos], epsf[pos, i] * dev[pos, j] + dev[pos, i] * epsf[pos, j] + epsf[pos, i] * epsf[pos, j]))
            return float(v), b

        mean = np.array([float(x) for x in ebar])
        dg = [element(i, i, vars[:, i]) for i in range(m)]
        out = {"mean": mean, "var": np.array([d[0] for d in dg]), "var_bound": np.array([d[1] for d in dg]),
               "mean_bound": 4 * (P + 8) * EPS * (wf[:, None] * dev).sum(axis=0) + EPS * np.abs(mean) + (wf[:, None] * epsf).sum(axis=0)}
        if covs is not None:
            el = [element(i, j, covs[:, i, j]) for i, j in pr]
            out["cov"] = np.array([d[0] for d in el]); out["cov_bound"] = np.array([d[1] for d in el])
    return _finish(out, covs, pr, m)


LD_EPS = 2.0 ** -63      # x87 extended precision (64-bit significand): numpy's longdouble on x86-64


def moments_lognormal_extended(means, weights, covs):
    """The whole lower triangle of the log-normal moments at sizes where P mpmath evaluations per element are too slow: the same
    formulas, vectorised in extended precision (numpy longdouble, significand 64 bits; exp / expm1 of the C library's long double
    routines).  Every element is a sum of P terms each within ~8 LD_EPS relative, so the values are within
    ref_err = 16 (P + 8) LD_EPS (sum w |t| + 4 r_i r_j + r_i e_j + e_i r_j) of the exact ones: 2^-11 x (2 / 8) of the device's
    bound or less, and it is ADDED to the bound.  The caller checks these values against the mpmath ones on a sample of elements.
    Returns the dict of moments() (pairs: the whole lower triangle)."""
    ld = np.longdouble
    assert np.finfo(ld).eps <= LD_EPS, "numpy longdouble is not extended precision here"
    means = np.asarray(means, dtype=np.float64); covs = np.asarray(covs, dtype=np.float64); w = np.asarray(weights, dtype=np.float64)
    P, m = means.shape
    vars_ = np.einsum("pii->pi", covs)
    pos = np.flatnonzero(w > 0)
    wq = w.astype(ld) / w.astype(ld).sum()
    e = np.exp(means.astype(ld) + vars_.astype(ld) / 2)                          # (P, m)
    ebar = (wq[pos, None] * e[pos]).sum(axis=0)
    d = e - ebar
    I, J = np.tril_indices(m)
    order = np.lexsort((I, J))                                                   # moments()' order: column by column
    I, J = I[order], J[order]
    t = e[:, I] * e[:, J] * np.expm1(covs[:, I, J].astype(ld))                    # (P, pairs)
    cov = (wq[pos, None] * (t[pos] + d[pos][:, I] * d[pos][:, J])).sum(axis=0)
    # the bounds of _moments_lognormal, in float64
    arg = means + 0.5 * vars_
    de = (EXP_ULP_DEV + 0.5 * np.abs(arg)) * EPS
    ef = e.astype(np.float64); dev = np.abs(d).astype(np.float64); wf = wq.astype(np.float64); tabs = np.abs(t).astype(np.float64)
    epsf = ef * de
    r = dev[pos].max(axis=0)
    wp = wf[pos, None]
    swt = (wp * tabs[pos]).sum(axis=0)
    b = 8 * (P + 8) * EPS * (swt + 4 * r[I] * r[J])
    b += (wp * tabs[pos] * (de[pos][:, I] + de[pos][:, J] + (EXPM1_ULP_DEV + 2) * EPS)).sum(axis=0)
    b += (wp * (epsf[pos][:, I] * dev[pos][:, J] + dev[pos][:, I] * epsf[pos][:, J] + epsf[pos][:, I] * epsf[pos][:, J])).sum(axis=0)
    emax = ef[pos].max(axis=0)
    ref_err = 16 * (P + 8) * LD_EPS * (swt + 4 * r[I] * r[J] + r[I] * emax[J] + emax[I] * r[J])
    dg = I == J
    out = {"mean": ebar.astype(np.float64),
           "mean_bound": 4 * (P + 8) * EPS * (wf[:, None] * dev).sum(axis=0) + EPS * np.abs(ef.T @ wf) + (wf[:, None] * epsf).sum(axis=0),
           "var": cov[dg].astype(np.float64), "var_bound": (b + ref_err)[dg],
           "cov": cov.astype(np.float64), "cov_bound": b + ref_err, "ref_err": ref_err}
    return _finish(out, covs, list(zip(I.tolist(), J.tolist())), m)


def brute_force(means, weights, covs, space, dps=60):
    """The definition, term by term in mpmath (tiny cases): mean = sum w e, cov = sum w (C + (e - mean)(e - mean)') under w / sum w."""
    P, m = means.shape
    with mp.workdps(dps):
        w = [mp.mpf(float(v)) for v in weights]
        sw = mp.fsum(w)
        w = [v / sw for v in w]
        mu = [[mp.mpf(float(means[p, i])) for i in range(m)] for p in range(P)]
        C = [[[mp.mpf(float(covs[p, i, j])) for j in range(m)] for i in range(m)] for p in range(P)]
        if space == 1:
            e = [[mp.exp(mu[p][i] + C[p][i][i] / 2) for i in range(m)] for p in range(P)]
            C = [[[e[p][i] * e[p][j] * (mp.exp(C[p][i][j]) - 1) for j in range(m)] for i in range(m)] for p in range(P)]
            mu = e
        mean = [mp.fsum(w[p] * mu[p][i] for p in range(P)) for i in range(m)]
        cov = [[mp.fsum(w[p] * (C[p][i][j] + (mu[p][i] - mean[i]) * (mu[p][j] - mean[j])) for p in range(P)) for j in range(m)]
               for i in range(m)]
        return np.array([float(x) for x in mean]), np.array([[float(x) for x in row] for row in cov]).reshape(m, m)


def one_pass(means, weights, covs):
    """The formula the kernels must NOT use, in fp64: sum w (C + mu mu') - mean mean'."""
    mean = weights @ means
    return mean, np.einsum("p,pij->ij", weights, covs + means[:, :, None] * means[:, None, :]) - np.outer(mean, mean)


def random_mixture(rng, P, m, offset=0.0, spread=1.0, vscale=1.0):
    """means (P, m) = offset + spread N(0, 1) (a common offset far above the between-particle spread when offset >> spread); covs
    (P, m, m) symmetric positive semi-definite of scale vscale, with components of zero covariance and points of zero variance;
    weights with one dominant component (never the first where P > 2) and components of weight 0 (P > 2), summing to 1 to rounding.
    Returns (means, vars, covs, weights)."""
    means = offset + spread * rng.standard_normal((P, m))
    k = max(1, min(m, 3))
    F = rng.standard_normal((P, m, k)) * math.sqrt(vscale / k)
    d = vscale * rng.random((P, m)) * (rng.random((P, m)) < 0.7)
    covs = np.einsum("pik,pjk->pij", F, F)
    covs = 0.5 * (covs + covs.transpose(0, 2, 1))
    covs[:, np.arange(m), np.arange(m)] += d
    if P > 1:
        covs[rng.integers(1, P)] = 0.0                       # a point mass
    if m > 1:
        z = rng.integers(0, m)                               # a point every component knows exactly
        covs[:, z, :] = 0.0; covs[:, :, z] = 0.0
    w = rng.random(P) + 0.05
    if P > 2:
        w[rng.choice(P, max(1, P // 5), replace=False)] = 0.0
        w[0] = 0.0 if P > 3 else w[0]
        dom = int(rng.integers(1, P))
        w[dom] = 9.0 * max(w.sum() - w[dom], 0.1)
    w = w / w.sum()
    return means, np.einsum("pii->pi", covs).copy(), covs, w
