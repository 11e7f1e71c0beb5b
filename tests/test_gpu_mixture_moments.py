"""Mixture moments on the GPU (agp_mixture_moments / agp_predict_mixture_batch: Distributions.mean / var / cov of the MixtureModel
predict_mvn returns, and of its MvLogNormal re-wrap) against the exact restatement of tests/_mixture_moments_ref.py, within the
bounds derived there.  Every case compares the whole lower triangle.  At P = 65, m = 130 the log-normal covariance (P mpmath
evaluations per element) is restated in extended precision (R.moments_lognormal_extended, its own error added to the bound), and
that restatement is held to the mpmath one on the diagonal, the corners and a seeded sample of the triangle."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mixture_moments_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

NORMAL = dict(offset=1e6, spread=1.0, vscale=1.0)          # a common offset 10^6 times the between-particle spread
LOGN = dict(offset=2.0, spread=0.4, vscale=0.1)            # log-space components of moderate size
YTS = ((2.5, -0.7), (-0.5, 0.3))                           # y_transform = (slope, intercept); one negative slope


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def sample_pairs(rng, m, k=300):
    pr = {(i, i) for i in range(m)} | {(m - 1, 0), (0, 0), (m - 1, m - 1), (m - 1, m - 2)}
    while len(pr) < min(k + m, m * (m + 1) // 2):
        i, j = sorted(rng.integers(0, m, 2))
        pr.add((int(j), int(i)))
    return sorted(pr)


def check(got, ref, ctx, slack=0.0):
    """got = (mean, var, cov or None) of the device; ref = R.moments(...).  slack: LP_TOL-type allowance on top of the bounds."""
    mean, var, cov = got
    m = mean.shape[0]
    for name, g, r, b in (("mean", mean, ref["mean"], ref["mean_bound"]), ("var", var, ref["var"], ref["var_bound"])):
        err = np.abs(g - r)
        tol = b + slack * max(1.0, np.abs(r).max() if m else 0.0)
        print(ctx, name, "max err / bound:", float((err / np.maximum(tol, 1e-300)).max()) if m else 0.0)
        assert (err <= tol).all(), (ctx, name, int(np.argmax(err - tol)), float(err.max()), float(tol.max()))
    if cov is not None:
        assert np.array_equal(cov, cov.T), (ctx, "asymmetric")
        assert same_bits(var, np.diag(cov).copy()), (ctx, "var is not the diagonal")
        g = np.array([cov[i, j] for i, j in ref["pairs"]])
        err = np.abs(g - ref["cov"])
        tol = ref["cov_bound"] + slack * max(1.0, np.abs(ref["cov"]).max())
        print(ctx, "cov max err / bound:", float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (ctx, "cov", ref["pairs"][int(np.argmax(err - tol))], float(err.max()), float(tol.max()))


# ---- the device functions of the log-normal components ----------------------------------------------------------------------

def test_device_exp_and_expm1_bounds(engine):
    """exp_f (which = 0) and the device library's expm1 (which = 9) against mpmath over the arguments the log-normal cases produce:
    within the constants the bounds are built from."""
    import mpmath as mp
    rng = np.random.default_rng(0)
    means, vars_, covs, _ = R.random_mixture(rng, 65, 17, **LOGN)
    # (up to where exp overflows: mixmom_exp hands exp_f every argument below 709.78, past the 700 csrc/agp_math.hpp documents it to)
    arg = np.concatenate([(means + 0.5 * vars_).ravel(), rng.uniform(-3.0, 6.0, 2000), rng.uniform(-60.0, 120.0, 1000),
                          rng.uniform(700.0, 709.78, 500), [709.78]])
    c = np.concatenate([covs.ravel()[::3], rng.uniform(-0.6, 0.6, 2000), 10.0 ** rng.uniform(-12, -1, 500), rng.uniform(-40.0, 60.0, 1000),
                        [0.0]])
    e_exp = R.ulp_err(engine.debug_math(0, arg), arg, mp.exp)
    e_em1 = R.ulp_err(engine.debug_math(9, c), c, mp.expm1)
    print(f"device exp_f error {e_exp:.3f} ulp, device expm1 error {e_em1:.3f} ulp")
    assert e_exp <= R.EXP_ULP_DEV and e_em1 <= R.EXPM1_ULP_DEV


# ---- a. caller-supplied components ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("P", [1, 2, 65])
def test_shapes_against_restatement(engine, P, space):
    for m in (0, 1, 17, 130):
        for kw in ([NORMAL, dict(offset=0.0, spread=1.0, vscale=1.0)] if space == 0 and m == 17 else [NORMAL if space == 0 else LOGN]):
            rng = np.random.default_rng(1000 * P + 10 * m + space)
            means, vars_, covs, w = R.random_mixture(rng, P, max(m, 1), **kw)
            means, vars_, covs = means[:, :m], vars_[:, :m], covs[:, :m, :m]
            for with_cov in (False, True):
                got = engine.mixture_moments(means, w, vars=vars_, covs=covs if with_cov else None, space=space)
                assert got[0].shape == (m,) and got[1].shape == (m,) and (got[2] is None) == (not with_cov)
                if m == 0:
                    continue
                if space == 1 and with_cov and P * m * m > 200_000:
                    exact = R.moments(means, w, covs=covs, space=1, pairs=sample_pairs(rng, m))
                    ref = R.moments_lognormal_extended(means, w, covs)
                    at = {pr: k for k, pr in enumerate(ref["pairs"])}
                    ix = np.array([at[pr] for pr in exact["pairs"]])
                    assert (np.abs(ref["cov"][ix] - exact["cov"]) <= ref["ref_err"][ix] + R.EPS * np.abs(exact["cov"])).all()
                    assert (np.abs(ref["mean"] - exact["mean"]) <= R.EPS * np.abs(exact["mean"])).all()
                else:
                    ref = R.moments(means, w, vars=vars_, covs=covs if with_cov else None, space=space)
                check(got, ref, (P, m, space, with_cov, kw["offset"]))
            # covariances given, only mean and var asked for: the diagonals
            if m:
                a = engine.mixture_moments(means, w, covs=covs, space=space, want_cov=False)
                b = engine.mixture_moments(means, w, vars=vars_, space=space)
                assert a[2] is None and same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ---- b / c. the resident series ----------------------------------------------------------------------------------------------

def population(pkg, engine, n, tp, P=11, seed=0, noise_pred=None):
    """P sampled particles that have a predictive on the engine's series, their weights (one 0), predict_batch's own outputs."""
    rng = np.random.default_rng(seed)
    nodes, noises = pkg.prior.sample_particles(rng, 3 * P, max_depth=3)
    _, _, _, info = engine.predict_batch(nodes, noises, tp, n=n, noise_pred=noise_pred, want_cov=True, check=False)
    ok = [p for p in range(3 * P) if info[p] == 0][:P]
    assert len(ok) == P
    nodes = [nodes[p] for p in ok]; noises = noises[ok]
    w = rng.random(P) + 0.1
    w[0] = 0.0
    w /= w.sum()
    return nodes, noises, w


def raw(mean, var, cov, yt):
    a, b = yt
    iv = 1.0 / (a * a)
    return (mean - b) / a, iv * var, None if cov is None else iv * cov


@pytest.mark.parametrize("n", [0, 50, 200])
def test_fused_covariance_pass(pkg, engine, n):
    ts, xs = pkg.prior.synthetic_series(200, seed=11)
    engine.set_data(ts, xs)
    for m in (1, 33, 130):
        tp = np.linspace(0.8, 1.3, m) if m > 1 else np.array([1.05])
        for npred, yt in zip((None, 0.0), YTS):
            nodes, noises, w = population(pkg, engine, n, tp, seed=7 * n + m, noise_pred=npred)
            mean, var, cov, _ = engine.predict_batch(nodes, noises, tp, n=n, noise_pred=npred, want_cov=True)
            mr, vr, cr = raw(mean, var, cov, yt)
            for space in ((0, 1) if m == 33 else (0,)):
                got = engine.predict_mixture_batch(nodes, noises, tp, w, n=n, noise_pred=npred, y_transform=yt, space=space, want_cov=True)
                assert (got[3] == 0).all()
                ref = R.moments(mr, w, covs=cr, space=space)
                check(got[:3], ref, ("fused", n, m, npred, yt, space), slack=R.LP_TOL)


def test_marginal_pass_with_training_queries(pkg, engine):
    """out_cov = NULL: queries = the training points + future points (the alpha / diag(K^-1) shortcut of agp_predict_batch)."""
    ts, xs = pkg.prior.synthetic_series(300, seed=12)
    engine.set_data(ts, xs)
    tp = np.concatenate([ts, 1.0 + 0.01 * np.arange(1, 31)])
    nodes, noises, w = population(pkg, engine, 300, tp[-30:], seed=5)
    mean, var, _, info = engine.predict_batch(nodes, noises, tp, check=False)
    assert (info == 0).all()
    for space, yt in zip((0, 1), YTS):
        mr, vr, _ = raw(mean, var, None, yt)
        got = engine.predict_mixture_batch(nodes, noises, tp, w, y_transform=yt, space=space)
        assert got[2] is None and (got[3] == 0).all()
        check(got[:3], R.moments(mr, w, vars=vr, space=space), ("marginal", space), slack=R.LP_TOL)


# ---- d. chunking ---------------------------------------------------------------------------------------------------------------

def test_workspace_chunking_is_bitwise_invisible(pkg, engine):
    ts, xs = pkg.prior.synthetic_series(300, seed=8)
    engine.set_data(ts, xs)
    tp = np.linspace(0, 1.1, 20)
    nodes, noises, w = population(pkg, engine, 300, tp, P=13, seed=8)
    w[:4] = 0.0; w /= w.sum()          # the first chunk of 3 holds no weight: the sums begin in the second
    rng = np.random.default_rng(8)
    means, vars_, covs, wm = R.random_mixture(rng, 13, 20, **LOGN)
    passes, chunks = engine.mixture_stats()
    whole = [engine.predict_mixture_batch(nodes, noises, tp, w, y_transform=YTS[1], space=s, want_cov=True)[:3] for s in (0, 1)]
    whole_m = [engine.mixture_moments(means, wm, covs=covs, space=s) for s in (0, 1)]
    passes0, chunks0 = engine.mixture_stats()
    assert (passes0 - passes, chunks0 - chunks) == (4, 4)          # (no limit: one chunk per pass)
    try:
        engine.set_workspace_limit(3 * 10 * 128 * 128 * 8)      # room for 3 particles per chunk (nt = 3 + 1 -> 10 tiles)
        parts = [engine.predict_mixture_batch(nodes, noises, tp, w, y_transform=YTS[1], space=s, want_cov=True)[:3] for s in (0, 1)]
        engine.set_workspace_limit(3 * 20 * 20 * 8)             # 3 caller-supplied covariances per chunk
        parts_m = [engine.mixture_moments(means, wm, covs=covs, space=s) for s in (0, 1)]
    finally:
        engine.set_workspace_limit(0)
    passes1, chunks1 = engine.mixture_stats()
    # the limited passes really ran in chunks of 3: ceil(13 / 3) = 5 each, less a leading chunk that holds no weight (the pass
    # sorts the particles, so the four of weight 0 need not lead it; random_mixture leaves at most the first three without weight)
    assert passes1 - passes0 == 4 and 4 * 4 <= chunks1 - chunks0 <= 4 * 5
    for a, b in zip(whole + whole_m, parts + parts_m):
        for x, y in zip(a, b):
            assert same_bits(x, y)


# ---- e. resampled population -----------------------------------------------------------------------------------------------------

def test_copies_are_evaluated_once_and_their_weights_added(pkg, engine):
    ts, xs = pkg.prior.synthetic_series(200, seed=13)
    engine.set_data(ts, xs)
    tp = np.linspace(0.9, 1.2, 33)
    nodes, noises, w = population(pkg, engine, 200, tp, seed=13)
    rng = np.random.default_rng(13)
    pop, pn, pw = [], [], []
    for p in rng.permutation(11):
        k = int(rng.integers(1, 4))
        split = rng.random(k); split /= split.sum()
        for s in split:
            pop.append(nodes[p]); pn.append(noises[p]); pw.append(w[p] * s)
    order = rng.permutation(len(pop))
    pop = [pop[i] for i in order]; pn = np.array(pn)[order]; pw = np.array(pw)[order]
    mean, var, cov, _ = engine.predict_batch(nodes, noises, tp, want_cov=True)
    ref = R.moments(mean, w, covs=cov)
    base = engine.predict_mixture_batch(nodes, noises, tp, w, want_cov=True)
    seen0, run0 = engine.dedup_stats()
    got = engine.predict_mixture_batch(pop, pn, tp, pw, want_cov=True)
    seen1, run1 = engine.dedup_stats()
    assert (seen1 - seen0, run1 - run0) == (len(pop), 11)
    # the bounds of (a) and nothing on top: both calls reduce the covariances predict_batch returned above (the same pass on the
    # same distinct particles), and the summed weights differ from w by a rounding each, which the (P + 8) of the bounds covers
    check(got[:3], ref, "copies")
    check(base[:3], ref, "distinct")
    pairs = ref["pairs"]
    d = np.abs(np.array([got[2][i, j] - base[2][i, j] for i, j in pairs]))
    print("copies vs distinct: cov", float((d / np.maximum(ref["cov_bound"], 1e-300)).max()), "mean",
          float((np.abs(got[0] - base[0]) / ref["mean_bound"]).max()))
    assert (d <= ref["cov_bound"]).all() and (np.abs(got[0] - base[0]) <= ref["mean_bound"]).all()


# ---- f. errors and undefined mixtures ------------------------------------------------------------------------------------------------

def test_nonpd_particle_and_argument_errors(pkg, engine):
    G = pkg
    rng = np.random.default_rng(2)
    ts = np.sort(rng.random(64)); xs = rng.standard_normal(64)
    ts[10] = ts[11]
    engine.set_data(ts, xs)
    nodes = [G.SquaredExponential(0.3, 1.0), G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1)]
    noises = np.array([0.1, 0.0, 0.2])          # duplicate time, zero noise: K11 singular for the Linear particle
    with pytest.raises(O.PosDefException):
        O.gp_logpdf(nodes[1].to_tuple(), 0.0, ts, xs)
    tp = np.linspace(1.0, 1.2, 9)
    for w in (np.array([0.5, 0.25, 0.25]), np.array([0.5, 0.0, 0.5])):
        for want_cov in (False, True):
            mean, var, cov, info = engine.predict_mixture_batch(nodes, noises, tp, w, want_cov=want_cov, check=False)
            assert info[1] != 0 and info[0] == 0 and info[2] == 0
            assert np.isnan(mean).all() and np.isnan(var).all() and (cov is None or np.isnan(cov).all())
            with pytest.raises(pkg.PosDefException):
                engine.predict_mixture_batch(nodes, noises, tp, w, want_cov=want_cov)
    good = dict(nodes=nodes[:1], noises=noises[:1], ts_pred=tp, weights=np.ones(1))
    for bad in (dict(weights=np.array([0.7])), dict(space=2), dict(y_transform=(0.0, 0.0)), dict(y_transform=(1.0, np.inf))):
        with pytest.raises(pkg.AGPError):
            engine.predict_mixture_batch(**{**good, **bad})
    means, vars_, covs, w = R.random_mixture(rng, 3, 4)
    for kw in (dict(vars=vars_, want_cov=True), dict(vars=vars_, space=2), dict(vars=vars_, weights=w * 1.01), dict()):
        wk = kw.pop("weights", w)
        with pytest.raises(pkg.AGPError):
            engine.mixture_moments(means, wk, **kw)
    # a component of weight 0 contributes nothing, whatever it holds
    means2 = means.copy(); covs2 = covs.copy()
    w3 = np.array([0.0, 0.625, 0.375])
    means2[0] = np.nan; covs2[0] = np.inf
    for space in (0, 1):
        for a, b in zip(engine.mixture_moments(means, w3, covs=covs, space=space), engine.mixture_moments(means2, w3, covs=covs2, space=space)):
            assert same_bits(a, b) and np.isfinite(a).all()


# ---- g. poison mode ----------------------------------------------------------------------------------------------------------------

def test_poisoned_context_returns_the_same_bits(pkg, engine, monkeypatch):
    rng = np.random.default_rng(21)
    ts, xs = pkg.prior.synthetic_series(200, seed=5)
    engine.set_data(ts, xs)
    tp = np.concatenate([ts[:10], 1.0 + 0.01 * np.arange(23)])
    nodes, noises, w = population(pkg, engine, 200, tp, seed=21)
    means, vars_, covs, wm = R.random_mixture(rng, 9, 33, **LOGN)

    def run(e):
        out = []
        for space in (0, 1):
            out += list(e.predict_mixture_batch(nodes, noises, tp, w, y_transform=YTS[0], space=space, want_cov=True)[:3])
            out += list(e.predict_mixture_batch(nodes, noises, tp, w, y_transform=YTS[0], space=space)[:2])
            out += list(e.mixture_moments(means, wm, covs=covs, space=space))
            out += list(e.mixture_moments(means, wm, vars=vars_, space=space)[:2])
        return out

    ref = run(engine)
    monkeypatch.setenv("AGP_POISON", "1")
    e = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_POISON")
    try:
        e.set_data(ts, xs)
        got = run(e)
        assert e.poison_stats()["bytes"] > 0
    finally:
        e.close()
    for a, b in zip(got, ref):
        assert same_bits(a, b)


# ---- h. the Python MixtureModel ------------------------------------------------------------------------------------------------

def test_python_mixture_model(pkg, engine):
    rng = np.random.default_rng(31)
    ts, xs = pkg.prior.synthetic_series(200, seed=6)
    engine.set_data(ts, xs)
    tp = np.linspace(0.9, 1.2, 17)
    nodes, noises, _ = population(pkg, engine, 200, tp, P=8, seed=31)
    lw = rng.standard_normal(8)
    yt = YTS[0]
    d = pkg.predict_mvn(engine, nodes, noises, lw, tp, y_transform=yt)
    w = np.exp(pkg.dist.normalize_weights(lw)[1])
    assert same_bits(d.probs, w)
    mean, var, cov, _ = engine.predict_batch(nodes, noises, tp, want_cov=True)
    mr, vr, cr = raw(mean, var, cov, yt)
    mu = w @ mr
    dm = mr - mu
    cref = np.einsum("p,pij->ij", w, cr + dm[:, :, None] * dm[:, None, :])
    scale = max(1.0, np.abs(cref).max())
    assert np.abs(d.mean() - mu).max() <= 1e-8 * max(1.0, np.abs(mu).max())
    assert np.abs(d.var() - np.diag(cref)).max() <= 1e-8 * scale
    assert np.abs(d.cov() - cref).max() <= 1e-8 * scale and same_bits(d.var(), np.diag(d.cov()).copy())
    y = mu + 0.1 * rng.standard_normal(17)
    pr = pkg.predict_proba(engine, nodes, noises, lw, tp, y, y_transform=yt)
    t = np.log(pr["weight"]) + pr["logp"]
    assert abs(d.logpdf(y) - (t.max() + np.log(np.exp(t - t.max()).sum()))) <= 1e-12 * max(1.0, abs(t.max()))
    ln = d.lognormal()
    ref = R.moments(mr, w, covs=cr, space=1)
    check((ln.mean(), ln.var(), ln.cov()), ref, "lognormal view", slack=R.LP_TOL)
    xq, ok = d.quantile(0.5, tol=1e-6)
    xq2, ok2 = pkg.predict_quantile(engine, nodes, noises, lw, tp, 0.5, y_transform=yt, tol=1e-6)
    assert same_bits(xq, xq2) and ok == ok2
    assert same_bits(d.rand(5, seed=3), pkg.predict_rand(engine, nodes, noises, lw, tp, 5, seed=3, y_transform=yt))
    # predict_mvn_sum's components through agp_mixture_moments
    comps = [pkg.MvNormal.from_moments(mr[p], cr[p]) for p in range(8)]
    fc = pkg.MixtureModel.from_components(comps, w, engine=engine)
    assert np.abs(fc.cov() - cref).max() <= 1e-8 * scale and np.abs(fc.mean() - mu).max() <= 1e-8 * max(1.0, np.abs(mu).max())
