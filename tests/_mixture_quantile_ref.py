"""Restatement of Statistics.quantile(::MixtureModel, q; tol, max_iter) (src/api.jl:559-596), the search behind predict_quantile,
on the per-point mixtures of Normal(means[p, i], sqrt(vars[p, i])) with weights w[p]:

  (a) `quantile_loop`: a literal transcription of the reference's vectorised loop (all points step together until every one
      has converged or max_iter iterations have run);
  (b) `quantile_search`: one search per point with its own exit — on convergence, at max_iter, at a fixed point (an update
      that leaves x bitwise unchanged: every later iteration would repeat it), or early on a cycle of the state (x, x_max, x_min)
      (Brent's method; the search then runs only the updates that take it to where max_iter would end) — vectorised over the
      points still searching, and
      recording each point's decision margin: the minimum over its checks of |eps| and of ||eps| - tol|;
  (c) `mp_cdf`: the mixture CDF in mpmath.

(a) and (b) evaluate the same fp64 CDF, `mixture_cdf`: sum over w != 0 of w * normcdf((x - mu) / sigma) with
normcdf(z) = erfc(-z * invsqrt2) / 2 (StatsFuns' expression, from memory) and a step at sigma == 0 (0 below mu, 1 above, 1/2 at mu:
the sigma = 0 convention, a choice).  The search's x depends on the CDF only through the signs of eps = cdf(x) - q and through
|eps| < tol, so an implementation whose CDF differs from this one by less than a point's decision margin returns that point's x
and iteration count bit for bit."""
import math

import mpmath as mp
import numpy as np
from scipy.special import erfc

INVSQRT2 = 0.7071067811865476
# Error bounds of erfc over the arguments -z / sqrt 2 of z in [-40, 10], against mpmath, in ulps of max(erfc, ERFC_FLOOR): relative
# where erfc >= 2^-20 (cephes-style exp(-t^2) factors lose ~2 t^2 ulps further out, where a term is too small to matter: below the
# floor an error counts in ulps of 2^-20, i.e. absolutely).  scipy's (the restatement's) measured 9.4 by
# tests/test_mixture_quantile_cpu.py::test_erfc_bound_numpy; the device library's measured 2.5 on an MI355X and is pinned by
# tests/test_gpu_predict_quantile.py::test_device_erfc_bound_and_sqrt.
ERFC_FLOOR = 2.0 ** -20
ERFC_ULP_NP = 10.0
ERFC_ULP_DEV = 4.0


def erfc_err_ulps(got, t, dps=40):
    """max over the points of |got - erfc(t)| in ulps of max(erfc(t), ERFC_FLOOR) (mpmath reference)."""
    worst = 0.0
    with mp.workdps(dps):
        for a, g in zip(np.asarray(t, np.float64), np.asarray(got, np.float64)):
            ref = mp.erfc(mp.mpf(float(a)))
            worst = max(worst, float(abs(mp.mpf(float(g)) - ref) / mp.mpf(float(np.spacing(max(float(ref), ERFC_FLOOR))))))
    return worst


def delta(P):
    """Bound on |cdf_device(x) - cdf_ref(x)| for a P-component mixture (weights summing to 1): each normcdf within
    ERFC_ULP_DEV + ERFC_ULP_NP ulps (of max(phi, floor)) of the other, one rounding of w * phi each, the device's lane chains
    (ceil(P / 64) additions) and 6-level butterfly, numpy's pairwise sum (<= 16 + log2 P sequential additions), in units of 2^-52
    of a sum <= 1."""
    chain = math.ceil(P / 64) + 6 + 16 + math.ceil(math.log2(max(P, 2)))
    return (ERFC_ULP_DEV + ERFC_ULP_NP + 2 + chain) * 2.0 ** -52


def normcdf(x, mu, sg):
    """normcdf((x - mu) / sg) elementwise (broadcasting), with the sigma == 0 step."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = (x - mu) / sg
        phi = 0.5 * erfc(-z * INVSQRT2)
    step = np.where(x < mu, 0.0, np.where(x > mu, 1.0, 0.5))
    return np.where(sg == 0.0, step, phi)


def mixture_cdf(x, M, S, w):
    """x (k,), M / S (k, P) means and standard deviations, w (P,) -> (k,): sum over w != 0 of w * normcdf."""
    nz = w != 0.0
    M = np.ascontiguousarray(M[:, nz]); S = np.ascontiguousarray(S[:, nz])
    return np.sum(w[nz] * normcdf(x[:, None], M, S), axis=1)


def jl_min(a, b):
    """Julia's min on Float64 arrays (NaN if either is NaN; min(-0.0, 0.0) = -0.0)."""
    r = np.where((b < a) | (np.signbit(b) & ~np.signbit(a)), b, a)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def jl_max(a, b):
    r = np.where((b > a) | (np.signbit(a) & ~np.signbit(b)), b, a)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def components(means, vars):
    """(P, m) means / variances -> (m, P) means and standard deviations (correctly rounded sqrt), as the device packs them."""
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(np.asarray(means, np.float64).T), np.ascontiguousarray(np.sqrt(np.asarray(vars, np.float64)).T)


def quantile_loop(means, vars, w, q, tol=1e-5, max_iter=10**6):
    """(a) src/api.jl:573-595 as written.  Returns (x (m,), success)."""
    M, S = components(means, vars)
    w = np.asarray(w, np.float64)
    m = M.shape[0]
    x = np.zeros(m)
    it = 0
    x_max = np.repeat(np.inf, m)
    x_min = np.repeat(-np.inf, m)
    success = False
    while it < max_iter:
        epsilon = mixture_cdf(x, M, S, w) - q
        if np.all(np.abs(epsilon) < tol):
            success = True
            break
        x_max = np.where(epsilon > 0, x, x_max)
        x_min = np.where(epsilon < 0, x, x_min)
        with np.errstate(invalid="ignore", over="ignore"):
            x_hi = jl_min(x_max, 2.0 ** np.sign(x) * x + (x == 0))
            x_lo = jl_max(x_min, 2.0 ** -np.sign(x) * x - (x == 0))
            x_hi_mid = (x + x_hi) / 2
            x_lo_mid = (x + x_lo) / 2
        x = np.where(np.abs(epsilon) < tol, x, np.where(epsilon < 0, x_hi_mid, x_lo_mid))
        it += 1
    return x, success


def quantile_search(means, vars, w, q, tol=1e-5, max_iter=10**6, points=None):
    """(b) one search per point (the kernel's semantics).  points: indices of the points to search (default all).
    Returns dict(x, converged (bool), iters, margin) over those points."""
    M, S = components(means, vars)
    if points is not None:
        M, S = np.ascontiguousarray(M[points]), np.ascontiguousarray(S[points])
    w = np.asarray(w, np.float64)
    m = M.shape[0]
    x = np.zeros(m); x_max = np.full(m, np.inf); x_min = np.full(m, -np.inf)
    iters = np.zeros(m, dtype=np.int64); conv = np.zeros(m, dtype=bool); margin = np.full(m, np.inf)
    # cycles of the state (x, x_max, x_min) — eps == 0 exactly with tol <= 0 makes the search go round a few states — found by
    # Brent's method (the state saved at powers of two); with period lam found at update `it`, the x of max_iter updates is the
    # one (max_iter - it) % lam updates on, so the search runs just those
    saved = np.tile([0.0, np.inf, -np.inf], (m, 1)); power = np.ones(m, dtype=np.int64); lam = np.zeros(m, dtype=np.int64)
    limit = np.full(m, max(int(max_iter), 0), dtype=np.int64); cyc = np.zeros(m, dtype=bool)
    act = np.arange(m) if max_iter > 0 else np.arange(0)
    while act.size:
        xa = x[act]
        eps = mixture_cdf(xa, M[act], S[act], w) - q
        margin[act] = np.minimum(margin[act], np.minimum(np.abs(eps), np.abs(np.abs(eps) - tol)))
        done = np.abs(eps) < tol
        conv[act[done]] = True
        keep = ~done
        act, xa, eps = act[keep], xa[keep], eps[keep]
        if not act.size:
            break
        xm = np.where(eps > 0, xa, x_max[act]); xn_ = np.where(eps < 0, xa, x_min[act])
        x_max[act], x_min[act] = xm, xn_
        with np.errstate(invalid="ignore", over="ignore"):
            up = np.where(xa > 0, 2.0, np.where(xa < 0, 0.5, np.where(xa == 0, 1.0, xa)))
            dn = np.where(xa > 0, 0.5, np.where(xa < 0, 2.0, np.where(xa == 0, 1.0, xa)))
            z01 = np.where(xa == 0, 1.0, 0.0)
            x_hi = jl_min(xm, up * xa + z01)
            x_lo = jl_max(xn_, dn * xa - z01)
            xnew = np.where(eps < 0, (xa + x_hi) / 2, (xa + x_lo) / 2)
        iters[act] += 1
        fixed = same_bits(xnew, xa)
        x[act] = xnew
        # Brent's cycle search on the points still looking
        look = act[~fixed & ~cyc[act]]
        lam[look] += 1
        st = np.stack([x[look], x_max[look], x_min[look]], axis=1)
        hit = same_bits(st, saved[look]).all(axis=1)
        found = look[hit]
        cyc[found] = True
        limit[found] = iters[found] + (max_iter - iters[found]) % lam[found]
        save = look[~hit & (lam[look] == power[look])]
        saved[save] = np.stack([x[save], x_max[save], x_min[save]], axis=1)
        power[save] *= 2; lam[save] = 0
        act = act[~fixed & (iters[act] < limit[act])]
    return {"x": x, "converged": conv, "iters": iters, "margin": margin}


def same_bits(a, b):
    """elementwise: identical bits, or both NaN"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def mp_cdf(x, mus, sds, w, dps=40):
    """(c) the mixture CDF at one point in mpmath (components at weight 0 skipped; sigma == 0 a step)."""
    with mp.workdps(dps):
        s = mp.mpf(0)
        xm = mp.mpf(float(x))
        for mu, sd, wi in zip(mus, sds, w):
            if wi == 0.0:
                continue
            if sd == 0.0:
                s += mp.mpf(float(wi)) * (0 if x < mu else (1 if x > mu else mp.mpf(0.5)))
            else:
                s += mp.mpf(float(wi)) * mp.ncdf((xm - mp.mpf(float(mu))) / mp.mpf(float(sd)))
        return s


def random_mixture(rng, P, m, scale=1.0, shift=0.0):
    """means / vars (P, m) and weights (P,) of a smooth random population: a few clusters of particles (with exact copies, as after
    resampling), means and standard deviations varying along the points."""
    base = rng.standard_normal((max(1, P // 4 + 1), 2))
    pick = rng.integers(0, base.shape[0], P)
    t = np.linspace(0.0, 1.0, m)[None, :]
    means = shift + scale * (base[pick, :1] + 0.5 * np.sin(3.0 * t + base[pick, 1:]) + 0.1 * rng.standard_normal((P, 1)))
    sds = scale * (0.05 + 0.5 * rng.random((P, 1))) * (1.0 + t)
    if P > 2:
        dup = rng.integers(0, P, P // 8)
        means[dup] = means[0]; sds[dup] = sds[0]
    lw = rng.standard_normal(P)
    w = np.exp(lw - lw.max()); w /= w.sum()
    return means, sds * sds, w
