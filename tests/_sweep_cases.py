"""TEST INFRASTRUCTURE: case builders shared by the sweep tests (tests/test_gpu_lag.py, tests/test_gpu_calendar.py) and by
tools/gpu_sweep_refactor_ab.py, which drives every route through csrc/agp_engine.hip logpdf_batch_impl with them.  Builders only:
the assertions stay with the tests."""
import numpy as np


def grad_shapes(G):
    """(covered + polynomial, element-wise only, number of polynomial ones): kernels by the class a gradient sweep on a regular grid
    puts them in — sums of stationary subtrees and Linear leaves (lag domain; the Toeplitz class), Linear leaves inside products
    (moment histograms), and what keeps the element-wise contraction (ChangePoints, four Linear factors)"""
    se, ge, per = G.SquaredExponential(0.3, 0.8), G.GammaExponential(0.4, 1.3, 0.6), G.Periodic(0.7, 0.21, 1.1)
    lin, lin2, cst, wn = G.Linear(0.3, 0.2, 0.7), G.Linear(-0.4, 0.1, 0.5), G.Constant(0.4), G.WhiteNoise(0.05)
    covered = [se, ge, per, cst + wn, per * se, per * se + ge, lin, lin + ge, ge + lin, lin + lin2, (lin + per * se) + (ge + lin2),
               cst * per + wn]
    # Linear leaves inside products: moment histograms over the lags, (2d+1) n virtual elements (d = 1, 2, 3)
    lin3 = G.Linear(0.1, 0.3, 0.4)
    poly = [lin * se, lin * lin2, (lin + se) * per, se + lin * ge, (lin * per) * (lin2 + se) + wn, cst * lin + ge * lin2, lin * lin2 * lin3,
            (lin * se + lin2) * (lin3 * per) * lin]
    elementwise = [G.ChangePoint(se, per, 0.5, 0.05), lin * lin2 * lin3 * lin, G.ChangePoint(lin, se, 0.4, 0.02) + ge]
    return covered + poly, elementwise, len(poly)


def calendar_series(pkg, freq, n, seed, shuffle=True):
    """a calendar-indexed series: pkg.prior.calendar_series's frequencies, or "missing": a daily index with ~8 % of the observations
    missing"""
    if freq == "missing":
        ts, xs = pkg.prior.calendar_series(n + n // 12, "D", seed=seed)
        keep = np.sort(np.random.default_rng(seed).permutation(len(ts))[:n])
        keep[0], keep[-1] = 0, len(ts) - 1
        ts, xs = ts[keep], xs[keep]
        if shuffle:
            perm = np.random.default_rng(seed + 1).permutation(n)
            ts, xs = ts[perm], xs[perm]
        return np.ascontiguousarray(ts), np.ascontiguousarray(xs)
    return pkg.prior.calendar_series(n, freq, seed=seed, shuffle=shuffle)


def non_positive_definite_pair(G):
    """(kernels, noises): a smooth kernel at noise 0 — singular to rounding on 256 grid points — beside one that factors"""
    return [G.SquaredExponential(5.0, 1.0), G.SquaredExponential(0.1, 1.0) + G.Linear(0.2, 0.1, 1.0)], np.array([0.0, 0.05])


def dominated_linear(G):
    """a Linear leaf that dominates its stationary neighbour: the Toeplitz downdate T^-1 = K^-1 + V Q V' is refused on the device and
    the particle's gradient repeated with the explicit inverse"""
    return G.Linear(0.3, 0.2, 2000.0) + G.SquaredExponential(0.3, 1e-5)
