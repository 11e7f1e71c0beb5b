"""Mixture quantiles on the GPU (agp_mixture_quantile / agp_predict_quantile_batch; src/api.jl:547-596 predict_quantile) against
the restatement of tests/_mixture_quantile_ref.py.  The search's x depends on the CDF only through its branch decisions, so
wherever a point's decision margin (b) exceeds delta(P) — the pinned bound on the difference of the two fp64 CDFs — x and the
iteration count must be bitwise equal; every converged point must satisfy |F(x) - q| < tol + delta by mpmath."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mixture_quantile_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

QS = (0.025, 0.5, 0.975)
B_FULL = 300_000          # (b) over every point up to this m * P; a seeded sample of the points above it
MP_SAMPLE = 60            # points per case checked against the mpmath CDF


def check_against_search(x, conv, iters, means, vars_, w, q, tol, max_iter=10**6, seed=0, ctx=None, min_class=0.95):
    """x / conv / iters (m,) of one q from the device vs (b); returns the in-class fraction."""
    P, m = means.shape
    rng = np.random.default_rng(seed)
    pts = np.arange(m) if m * P <= B_FULL else np.sort(rng.choice(m, 256, replace=False))
    b = R.quantile_search(means, vars_, w, q, tol=tol, max_iter=max_iter, points=pts)
    d = R.delta(P)
    cls = b["margin"] > d
    frac = cls.mean() if pts.size else 1.0
    assert frac >= min_class, (ctx, frac)
    bad = cls & ~(R.same_bits(x[pts], b["x"]) & (iters[pts] == b["iters"]) & (conv[pts] == b["converged"]))
    assert not bad.any(), (ctx, pts[bad][:5], x[pts][bad][:5], b["x"][bad][:5], iters[pts][bad][:5], b["iters"][bad][:5])
    M, S = R.components(means, vars_)
    cpts = np.flatnonzero(conv)
    for i in rng.choice(cpts, min(max(6, MP_SAMPLE * 64 // max(P, 64)), cpts.size), replace=False) if cpts.size else []:
        F = R.mp_cdf(x[i], M[i], S[i], w)
        assert abs(F - q) < tol + d, (ctx, i, float(F), q)
    return frac


def test_device_erfc_bound_and_sqrt(engine):
    """The device library's erfc (what the kernel's normcdf calls) against mpmath on -z / sqrt 2, z in [-40, 10]: within
    ERFC_ULP_DEV ulps (of max(erfc, 2^-20)), the bound delta() is built from; sqrt (the packed sigma) correctly rounded."""
    rng = np.random.default_rng(0)
    z = np.concatenate([np.linspace(-40.0, 10.0, 4001), rng.uniform(-40.0, 10.0, 4000), rng.uniform(-1.0, 1.0, 1000)])
    t = -z * R.INVSQRT2
    worst = R.erfc_err_ulps(engine.debug_math(4, t), t)
    print("device erfc error (ulps of max(erfc, 2^-20)):", worst)
    assert worst <= R.ERFC_ULP_DEV, worst
    v = np.concatenate([np.exp(rng.uniform(-700.0, 700.0, 20000)), rng.random(5000), [0.0, -0.0, 5e-324, 1e-310, 2.0, 4.0, np.inf]])
    assert R.same_bits(engine.debug_math(5, v), np.sqrt(v)).all()


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 512, 2048])
def test_shapes_against_restatement(engine, P):
    fracs = []
    for m in (0, 1, 17, 4096):
        for nq in (1, 3):
            rng = np.random.default_rng(P * 7919 + m * 31 + nq)
            scale, shift = [(1.0, 0.0), (40.0, 200.0), (1e-3, -0.05)][(m + nq) % 3]
            means, vars_, w = R.random_mixture(rng, P, max(m, 1), scale=scale, shift=shift)
            means, vars_ = means[:, :m], vars_[:, :m]
            q = QS[1] if nq == 1 else np.array(QS)
            tol = 1e-5 if nq == 1 else 1e-6
            x, conv, iters = engine.mixture_quantile(means, vars_, w, q, tol=tol)
            x = x.reshape(m, nq); conv = conv.reshape(m, nq); iters = iters.reshape(m, nq)
            if m == 0:
                continue
            assert conv.all(), (P, m, nq)
            for k in range(nq):
                fracs.append(check_against_search(x[:, k], conv[:, k], iters[:, k], means, vars_, w, np.atleast_1d(q)[k], tol,
                                                  seed=m + k, ctx=(P, m, nq, k)))
    print(f"P={P}: in-class fractions {min(fracs):.4f}..{max(fracs):.4f}")


def test_query_order_and_subsets_are_bitwise_invariant(engine):
    rng = np.random.default_rng(4)
    P, m = 300, 700
    means, vars_, w = R.random_mixture(rng, P, m, scale=3.0)
    x, c, it = engine.mixture_quantile(means, vars_, w, QS, tol=1e-6)
    perm = rng.permutation(m)
    xp, cp, itp = engine.mixture_quantile(means[:, perm], vars_[:, perm], w, QS, tol=1e-6)
    assert R.same_bits(xp, x[perm]).all() and np.array_equal(cp, c[perm]) and np.array_equal(itp, it[perm])
    sub = np.sort(rng.choice(m, 37, replace=False))
    xs, cs, its = engine.mixture_quantile(means[:, sub], vars_[:, sub], w, QS[::-1], tol=1e-6)
    assert R.same_bits(xs, x[sub][:, ::-1]).all() and np.array_equal(its, it[sub][:, ::-1])
    x1, _, _ = engine.mixture_quantile(means[:, sub[:1]], vars_[:, sub[:1]], w, QS[2], tol=1e-6)
    assert R.same_bits(x1, x[sub[:1], 2]).all()


def test_weights_sigma_zero_and_unreachable_tol(engine):
    rng = np.random.default_rng(8)
    P, m = 70, 200
    means, vars_, w = R.random_mixture(rng, P, m)
    # zero weights on NaN components, underflowed weights, sigma = 0 components
    w[:5] = [0.0, 0.0, 1e-320, 5e-324, 1e-310]; w[5:] /= w[5:].sum()
    means[:2] = np.nan; vars_[:2] = np.nan
    vars_[10:20] = 0.0
    M, S = R.components(means, vars_)
    for q, tol in ((0.3, 1e-5), (0.5, 1e-7), (0.9, 1e-300), (0.4, 0.0), (0.2, -1.0)):
        x, conv, iters = engine.mixture_quantile(means, vars_, w, q, tol=tol, max_iter=100_000)
        reachable = tol >= 1e-7
        # (an unreachable tol ends every search among adjacent doubles, where eps is a few ulps: the decisions there are below
        # any margin, so x is checked by its property instead — a fixed point (or a cycle) at the quantile, well before max_iter)
        frac = check_against_search(x, conv, iters, means, vars_, w, q, tol, max_iter=100_000, ctx=(q, tol),
                                    min_class=0.9 if reachable else 0.0)
        if not reachable:
            # (tol = 1e-300 converges only where eps == 0 exactly — common among adjacent doubles at q = 0.9; tol <= 0 never)
            assert (iters < 100_000).all() and not (tol <= 0.0 and conv.any())
            for i in range(0, m, 9):          # (or next to the jump of a sigma = 0 component across q)
                jump = np.abs(means[10:20, i] - x[i]).min() <= 2 * np.spacing(abs(x[i]))
                assert abs(R.mp_cdf(x[i], M[i], S[i], w) - q) < 1e-12 or jump, (q, tol, i)
        print(q, tol, frac, iters.max())
    # max_iter: 0 -> x = 0, nothing converged; a few -> exactly that many updates
    x, conv, iters = engine.mixture_quantile(means, vars_, w, 0.3, max_iter=0)
    assert (x == 0).all() and not conv.any() and (iters == 0).all()
    x, conv, iters = engine.mixture_quantile(means, vars_, w, 0.3, max_iter=3)
    b = R.quantile_search(means, vars_, w, 0.3, max_iter=3)
    assert R.same_bits(x, b["x"]).all() and (iters == 3).all() and not conv.any()


def test_argument_errors(pkg, engine):
    rng = np.random.default_rng(1)
    means, vars_, w = R.random_mixture(rng, 4, 6)
    E = pkg.AGPError
    bad = [dict(q=0.0), dict(q=1.0), dict(q=np.nan), dict(q=[0.5, 1.5]), dict(q=-0.1)]
    for kw in bad:
        with pytest.raises(E):
            engine.mixture_quantile(means, vars_, w, kw["q"])
    for ww in (w * 2.0, np.where(np.arange(4) == 0, -0.1, w), np.where(np.arange(4) == 1, np.nan, w),
               np.where(np.arange(4) == 1, np.inf, w)):
        with pytest.raises(E):
            engine.mixture_quantile(means, vars_, ww, 0.5)
    for fld, val in (("m", np.nan), ("m", np.inf), ("v", -1e-9), ("v", np.nan)):
        mm, vv = means.copy(), vars_.copy()
        (mm if fld == "m" else vv)[2, 3] = val
        with pytest.raises(E):
            engine.mixture_quantile(mm, vv, w, 0.5)
        w0 = w.copy(); w0[2] = 0.0; w0 /= w0.sum()          # the same component at weight 0 is never evaluated
        engine.mixture_quantile(mm, vv, w0, 0.5)
    with pytest.raises(E):
        engine.mixture_quantile(np.zeros((0, 6)), np.zeros((0, 6)), np.zeros(0), 0.5)        # P == 0
    x, c, it = engine.mixture_quantile(np.zeros((4, 0)), np.zeros((4, 0)), w, QS)            # m == 0
    assert x.shape == (0, 3)
    # the C entry directly: NULL components, negative sizes
    lib, ctx = engine._lib, engine._ctx
    out = np.empty(6); qa = np.array([0.5])
    from autogp_jl_amd.engine import _dp
    assert lib.agp_mixture_quantile(ctx, 6, 4, None, _dp(vars_), _dp(w), _dp(qa), 1, 1e-5, 100, _dp(out), None, None) != 0
    assert lib.agp_mixture_quantile(ctx, -1, 4, _dp(means), _dp(vars_), _dp(w), _dp(qa), 1, 1e-5, 100, _dp(out), None, None) != 0
    assert lib.agp_mixture_quantile(ctx, 6, 4, _dp(means), _dp(vars_), _dp(w), _dp(qa), -1, 1e-5, 100, _dp(out), None, None) != 0


# ---- agp_predict_quantile_batch ---------------------------------------------------------------------------------------------

def fixture_kernels(G):
    base = [G.WhiteNoise(1), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
            G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1)]      # test/test_GP.jl:24-33
    return base + [base[2] + base[5], base[3] * base[4], G.ChangePoint(base[2], base[5], 0.5, 0.05),
                   G.ChangePoint(base[3] + base[4], base[2] * base[5], 0.3, 0.2)]


def weights_of(pkg, P, seed):
    lw = np.random.default_rng(seed).standard_normal(P) * 2.0
    return np.exp(pkg.dist.normalize_weights(lw)[1]), lw


def composed(pkg, eng, nodes, noises, tp, w, q, tol, yt, n=None, **kw):
    """predict_batch (marginal) -> numpy raw transform -> agp_mixture_quantile"""
    n = eng.n_max if n is None else n
    mean, var, _, info = eng.predict_batch(nodes, noises, tp, n=n, check=False, **kw)
    mr, vr, info = pkg.raw_components(mean, var, info, n, yt)
    assert (info == 0).all()
    return eng.mixture_quantile(mr, vr, w, q, tol=tol), (mr, vr)


def check_fused(pkg, eng, nodes, noises, tp, q, tol=1e-6, yt=(1.7, -0.3), n=None, oracle=None, **kw):
    P = len(nodes)
    w, _ = weights_of(pkg, P, len(tp) + P)
    x, conv, it, info = eng.predict_quantile_batch(nodes, noises, tp, w, q, n=n, y_transform=yt, tol=tol, **kw)
    assert (info == 0).all()
    (x2, c2, it2), (mr, vr) = composed(pkg, eng, nodes, noises, tp, w, q, tol, yt, n=n, **kw)
    assert R.same_bits(x, x2).all() and np.array_equal(conv, c2) and np.array_equal(it, it2)
    assert conv.all()
    X = x.reshape(len(tp), -1); Cv = conv.reshape(len(tp), -1); It = it.reshape(len(tp), -1)
    for k, qk in enumerate(np.atleast_1d(q)):
        check_against_search(X[:, k], Cv[:, k], It[:, k], mr, vr, w, qk, tol, seed=k, ctx=("fused", len(tp), k), min_class=0.9)
    if oracle is not None:
        # the oracle's predictive (O.predict_mvn, weights from O.particle_weights) through (b): the device's x satisfies the
        # oracle mixture's quantile condition, to the tolerance plus the predictive's own error
        ts, xs, npred = oracle
        mo = np.empty((P, len(tp))); vo = np.empty((P, len(tp)))
        for p in range(P):
            mu, cv = O.predict_mvn(nodes[p].to_tuple(), float(noises[p]), ts, xs, tp, noise_pred=npred)
            mo[p], vo[p] = mu, np.diag(cv)
        mro, vro, _ = pkg.raw_components(mo, vo, np.zeros(P, np.int32), len(ts), yt)
        wo = O.particle_weights(weights_of(pkg, P, len(tp) + P)[1])
        Mo, So = R.components(mro, vro)
        for k, qk in enumerate(np.atleast_1d(q)):
            bo = R.quantile_search(mro, vro, wo, qk, tol=tol)
            assert bo["converged"].all()
            rng = np.random.default_rng(k)
            for i in rng.choice(len(tp), min(25, len(tp)), replace=False):
                F = R.mp_cdf(X[i, k], Mo[i], So[i], wo)
                assert abs(F - qk) < tol + 1e-7, (i, k, float(F), qk)
            close = np.abs(X[:, k] - bo["x"]) <= 1e-3 * np.maximum(1.0, np.abs(bo["x"]))
            assert close.mean() >= 0.9


def test_fused_fixture_kernels_and_oracle(pkg, engine):
    G = pkg
    nodes = fixture_kernels(G)
    P = len(nodes)
    noises = np.full(P, 0.2)
    rng = np.random.default_rng(11)
    ts = np.sort(rng.random(150)); xs = 0.5 * rng.standard_normal(150)
    engine.set_data(ts, xs)
    tp = np.concatenate([ts[rng.integers(0, 150, 20)], rng.random(30), 1.0 + 0.02 * np.arange(40)])
    check_fused(pkg, engine, nodes, noises, tp, QS, oracle=(ts, xs, None))
    check_fused(pkg, engine, nodes, noises, tp, 0.5, tol=1e-5, yt=(0.25, 3.0), noise_pred=0.05, oracle=(ts, xs, 0.05))


def test_fused_prior_population_mean_functions(pkg, engine):
    rng = np.random.default_rng(5)
    ts, xs = pkg.prior.synthetic_series(600, seed=3, shuffle=True)
    engine.set_data(ts, xs)
    nodes, noises = pkg.prior.sample_particles(rng, 48, max_depth=4, min_depth=2)
    n = 400
    tp = np.concatenate([ts[:60], 1.0 + 0.01 * np.arange(100)])
    _, _, _, info = engine.predict_batch(nodes, noises, tp, n=n, check=False)
    ok = [p for p in range(48) if info[p] == 0]
    nodes = [nodes[p] for p in ok]; noises = noises[ok]
    check_fused(pkg, engine, nodes, noises, tp, QS, n=n)
    mt = 0.2 * ts[:n] - 0.1; mp_ = 0.2 * tp - 0.1
    check_fused(pkg, engine, nodes, noises, tp, QS, n=n, mean_train=mt, mean_pred=mp_, noise_pred=0.3 * noises)


def test_fused_regular_and_calendar_series(pkg, engine):
    """A regular grid with the queries on and after it (structured / lattice predictive paths) and a shuffled calendar series."""
    rng = np.random.default_rng(6)
    n = 512
    ts = np.arange(n) / 1023.0; xs = np.sin(9.0 * ts) + 0.1 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    nodes, noises = pkg.prior.sample_particles(rng, 40, max_depth=3)
    tp = np.concatenate([ts[-50:], (n + np.arange(200)) / 1023.0])
    _, _, _, info = engine.predict_batch(nodes, noises, tp, check=False)
    ok = [p for p in range(40) if info[p] == 0]
    check_fused(pkg, engine, [nodes[p] for p in ok], noises[ok], tp, QS)
    ts_c, xs_c = pkg.prior.calendar_series(400, "M", seed=3, shuffle=True)
    engine.set_data(ts_c, xs_c)
    tq = np.concatenate([ts_c[:30], 1.0 + (np.arange(1, 41) / 400.0)])
    _, _, _, info = engine.predict_batch(nodes, noises, tq, check=False)
    ok = [p for p in range(40) if info[p] == 0]
    check_fused(pkg, engine, [nodes[p] for p in ok], noises[ok], tq, QS)


def test_fused_nonpd_particle(pkg, engine):
    G = pkg
    rng = np.random.default_rng(2)
    ts = np.sort(rng.random(64)); xs = rng.standard_normal(64)
    ts[10] = ts[11]
    engine.set_data(ts, xs)
    nodes = [G.SquaredExponential(0.3, 1.0), G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1)]
    noises = np.array([0.1, 0.0, 0.2])          # duplicate time, zero noise: K11 singular for the Linear particle
    tp = np.linspace(1.0, 1.2, 9)
    w = np.array([0.5, 0.25, 0.25])
    x, conv, it, info = engine.predict_quantile_batch(nodes, noises, tp, w, QS, check=False)
    assert info[1] != 0 and info[0] == 0 and info[2] == 0
    assert np.isnan(x).all() and not conv.any()
    with pytest.raises(pkg.PosDefException):
        engine.predict_quantile_batch(nodes, noises, tp, w, QS)
    with pytest.raises(pkg.PosDefException):
        pkg.predict_quantile(engine, nodes, noises, np.log(w), tp, 0.5)


def test_module_level_predict_quantile_and_multi(pkg, engine):
    rng = np.random.default_rng(12)
    ts, xs = pkg.prior.synthetic_series(300, seed=4)
    engine.set_data(ts, xs)
    nodes, noises = pkg.prior.sample_particles(rng, 16, max_depth=3)
    tp = np.linspace(0.9, 1.3, 41)
    _, _, _, info = engine.predict_batch(nodes, noises, tp, check=False)
    ok = [p for p in range(16) if info[p] == 0]
    nodes = [nodes[p] for p in ok]; noises = noises[ok]
    lw = rng.standard_normal(len(nodes))
    yt = (0.5, 0.1)
    x, s = pkg.predict_quantile(engine, nodes, noises, lw, tp, 0.5, y_transform=yt, tol=1e-6)
    assert x.shape == (41,) and isinstance(s, bool) and s
    xv, sv = pkg.predict_quantile(engine, nodes, noises, lw, tp, QS, y_transform=yt, tol=1e-6)
    assert xv.shape == (41, 3) and sv.shape == (3,) and sv.all()
    assert R.same_bits(xv[:, 1], x).all()
    assert (xv[:, 0] < xv[:, 1]).all() and (xv[:, 1] < xv[:, 2]).all()
    w = np.exp(pkg.dist.normalize_weights(lw)[1])
    x2, _, _, _ = engine.predict_quantile_batch(nodes, noises, tp, w, 0.5, y_transform=yt, tol=1e-6)
    assert R.same_bits(x2, x).all()
    # the multi-device route (two contexts holding the same data): the gathered components searched on one device
    e2 = pkg.GPEngine(0)
    try:
        e2.set_data(ts, xs)
        xm, cm, itm, im = pkg.predict_quantile_multi([engine, e2], nodes, noises, tp, w, QS, y_transform=yt, tol=1e-6)
        mean, var, _, info = pkg.predict_batch_multi([engine, e2], nodes, noises, tp, check=False)
        mr, vr, _ = pkg.raw_components(mean, var, info, 300, yt)
        xr, cr, itr = engine.mixture_quantile(mr, vr, w, QS, tol=1e-6)
        assert R.same_bits(xm, xr).all() and np.array_equal(cm, cr) and np.array_equal(itm, itr) and cm.all()
        assert np.abs(xm - xv).max() <= 1e-4 * max(1.0, np.abs(xv).max())
    finally:
        e2.close()


def test_poison_and_two_engines_bitwise(pkg, engine, monkeypatch):
    rng = np.random.default_rng(21)
    ts, xs = pkg.prior.synthetic_series(400, seed=5)
    nodes, noises = pkg.prior.sample_particles(rng, 24, max_depth=3)
    tp = np.concatenate([ts[:40], 1.0 + 0.01 * np.arange(60)])
    w = np.exp(pkg.dist.normalize_weights(rng.standard_normal(24))[1])
    engine.set_data(ts, xs)
    ref = engine.predict_quantile_batch(nodes, noises, tp, w, QS, tol=1e-6, check=False)
    means, vars_, _ = R.random_mixture(rng, 24, 300)
    ref_m = engine.mixture_quantile(means, vars_, w, QS, tol=1e-6)
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            e.set_data(ts, xs)
            got = e.predict_quantile_batch(nodes, noises, tp, w, QS, tol=1e-6, check=False)
            got_m = e.mixture_quantile(means, vars_, w, QS, tol=1e-6)
            for a, b in zip(got + got_m, ref + ref_m):
                assert R.same_bits(a, b).all() if a.dtype == np.float64 else np.array_equal(a, b)
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
