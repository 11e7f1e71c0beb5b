"""Batched sum-of-GPs posterior on the GPU (agp_infer_gp_sum_batch / agp_predict_sum_batch; src/api.jl:898-1034 predict_sum /
predict_mvn_sum, src/GP.jl:904-993 infer_gp_sum) against the restatement of tests/_sum_decomposition_ref.py (oracle.infer_gp_sum,
oracle.quantile), against the single-particle entry, and for bitwise invariance under batch order, copies, chunking and poison mode."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _sum_decomposition_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-8
LEAVES = ("Periodic", "Linear", "SquaredExponential", "GammaExponential", "Constant", "WhiteNoise")


def population(pkg, seed, P, leaf):
    G = pkg
    rng = np.random.default_rng(seed)
    nodes, noises = G.prior.sample_particles(rng, P, max_depth=3)
    noises = np.maximum(noises, 0.05)
    T = getattr(G, leaf)
    return nodes, noises, [list(G.split_kernel_sop(nd, T)) for nd in nodes]


def series(pkg, kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "regular":
        ts = np.linspace(0.0, 1.0, n) if n > 1 else np.full(n, 0.5)
        return ts, 0.5 * np.sin(9 * ts) + 0.1 * rng.standard_normal(n)
    if kind == "irregular":
        return np.sort(rng.random(n)), 0.4 * rng.standard_normal(n)
    ts, xs = pkg.prior.calendar_series(max(n, 2), "M", seed=seed)
    return ts[:n], xs[:n]


def close(got, ref, what):
    err = np.abs(got - ref).max() if ref.size else 0.0
    assert err <= TOL * max(1.0, np.abs(ref).max() if ref.size else 0.0), (what, err)


@pytest.mark.parametrize("kind", ["regular", "irregular", "calendar"])
@pytest.mark.parametrize("n,p", [(0, 9), (1, 5), (127, 3), (128, 17), (129, 11), (257, 40)])
def test_oracle_parity(pkg, engine, kind, n, p):
    nodes, noises, splits = population(pkg, 100 * n + p, 5, LEAVES[(n + p) % len(LEAVES)])
    ts, xs = series(pkg, kind, n, n + 1)
    engine.set_data(ts if n else np.zeros(1), xs if n else np.zeros(1))
    tp = np.linspace(-0.1, 1.2, p)
    for npred in (None, 0.0, 0.03):
        mean, var, cov, info, iF, iX = engine.infer_gp_sum_batch(splits, noises, tp, n=n, noise_pred=npred, want_cov=True)
        mean2, var2, cov2, _, _, _ = engine.infer_gp_sum_batch(splits, noises, tp, n=n, noise_pred=npred)
        assert (info == 0).all() and cov2 is None
        assert np.array_equal(mean, mean2) and np.array_equal(var, var2)
        assert iF == [slice(0, p), slice(p, 2 * p)] and iX == slice(2 * p, 3 * p)
        for k in range(len(nodes)):
            mu_o, S_o, _, _ = O.infer_gp_sum([x.to_tuple() for x in splits[k]], noises[k], ts, xs, tp, noise_pred=npred)
            ctx = (kind, n, p, npred, k)
            close(mean[k], mu_o, ("mean",) + ctx)
            close(cov[k], S_o, ("cov",) + ctx)
            close(var[k], np.diag(S_o), ("var",) + ctx)
            assert np.array_equal(np.diag(cov[k]), var[k]), ctx


def test_single_entry_parity_and_prior(pkg, engine):
    """Per particle, agp_infer_gp_sum's numbers to rounding; with n = 0, the prior (test/test_GP.jl:185,205)."""
    G = pkg
    nodes, noises, splits = population(pkg, 7, 6, "Periodic")
    ts, xs = series(pkg, "irregular", 150, 3)
    engine.set_data(ts, xs)
    tp = np.linspace(0.0, 1.25, 33)
    for npred in (None, 0.0, 0.02):
        mean, var, cov, _, _, _ = engine.infer_gp_sum_batch(splits, noises, tp, noise_pred=npred, want_cov=True)
        for k in range(len(nodes)):
            m1, c1, _, _ = engine.infer_gp_sum(splits[k], noises[k], tp, noise_pred=npred)
            close(mean[k], m1, ("single mean", npred, k))
            close(cov[k], c1, ("single cov", npred, k))
    mean, var, cov, _, _, _ = engine.infer_gp_sum_batch(splits, noises, tp, n=0, noise_pred=0.0, want_cov=True)
    for k in range(len(nodes)):
        mu_o, S_o, _, _ = O.infer_gp_sum([x.to_tuple() for x in splits[k]], noises[k], [], [], tp, noise_pred=0.0)
        assert np.array_equal(mean[k], np.zeros_like(mean[k]))
        close(cov[k], S_o, ("prior", k))
        # the components' covariances add up to the observable's (test/test_GP.jl:228-237), JITTER aside
        p = tp.shape[0]
        lat = sum(cov[k][a, b] for a in (slice(0, p), slice(p, 2 * p)) for b in (slice(0, p), slice(p, 2 * p)))
        assert np.abs(lat - cov[k][2 * p:, 2 * p:]).max() <= 1e-6 * max(1.0, np.abs(lat).max())


def test_bitwise_invariance(pkg, engine):
    """Reorder, copies (dedup counter moves), a small workspace limit: every particle keeps its bits."""
    nodes, noises, splits = population(pkg, 11, 8, "Linear")
    ts, xs = series(pkg, "regular", 200, 5)
    engine.set_data(ts, xs)
    tp = np.linspace(0.0, 1.3, 60)
    q = [0.05, 0.5, 0.95]
    base = engine.infer_gp_sum_batch(splits, noises, tp, want_cov=True)[:3]
    bsum = engine.predict_sum_batch(splits, noises, tp, q=q, y_transform=(2.0, 0.3))[:2]
    perm = np.random.default_rng(0).permutation(8)
    idx = np.concatenate([perm, [3, 3, 0, 5]])
    d0 = engine.dedup_stats()
    got = engine.infer_gp_sum_batch([splits[i] for i in idx], noises[idx], tp, want_cov=True)[:3]
    gsum = engine.predict_sum_batch([splits[i] for i in idx], noises[idx], tp, q=q, y_transform=(2.0, 0.3))[:2]
    d1 = engine.dedup_stats()
    assert d1 != d0
    for a, b in zip(base + bsum, got + gsum):
        assert np.array_equal(a[idx], b)
    engine.set_workspace_limit(1 << 20)
    try:
        small = engine.infer_gp_sum_batch(splits, noises, tp, want_cov=True)[:3]
        ssum = engine.predict_sum_batch(splits, noises, tp, q=q, y_transform=(2.0, 0.3))[:2]
    finally:
        engine.set_workspace_limit(0)
    for a, b in zip(base + bsum, small + ssum):
        assert np.array_equal(a, b)
    # one particle alone: the same bits as inside the batch
    one = engine.infer_gp_sum_batch(splits[2:3], noises[2:3], tp, want_cov=True)[:3]
    for a, b in zip(base, one):
        assert np.array_equal(a[2:3], b)


def test_predict_sum_against_restatement(pkg, engine):
    """Raw means with the F_1 intercept shift and the marginal quantiles of predict_sum against oracle.quantile on the restated
    raw components; the module-level predict_sum's columns and row order."""
    G = pkg
    nodes, noises, splits = population(pkg, 21, 6, "Periodic")
    ts, xs = series(pkg, "calendar", 144, 2)
    n_fit = 115
    engine.set_data(ts[:n_fit], xs[:n_fit])
    tp = np.concatenate([ts, ts[-1] + (ts[1] - ts[0]) * np.arange(1, 21)])
    q = [1e-6, 0.025, 0.5, 0.975]
    a, b = 0.37, -1.2
    for npred in (None, 0.0, 0.01):
        mean, x, info = engine.predict_sum_batch(splits, noises, tp, q=q, noise_pred=npred, y_transform=(a, b))
        assert (info == 0).all() and x.shape == (6, 3 * tp.shape[0], 4)
        comps, idx = R.predict_mvn_sum([[s.to_tuple() for s in sp] for sp in splits], noises, ts[:n_fit], xs[:n_fit], tp,
                                       y_transform=(a, b), noise_pred=npred)
        for k, (mr, Sr) in enumerate(comps):
            close(mean[k], mr, ("raw mean", npred, k))
            close(x[k], O.quantile(mr, Sr, q), ("quantiles", npred, k))
            assert np.array_equal(x[k][:, 2], mean[k])          # (sigma * ndtri(0.5) = 0: the median is the mean, bit for bit)
        # predict_sum without quantiles: the same means
        m0, x0, _ = engine.predict_sum_batch(splits, noises, tp, noise_pred=npred, y_transform=(a, b))
        assert np.array_equal(m0, mean) and x0.shape == (6, 3 * tp.shape[0], 0)
    lw = np.linspace(-2.0, 0.0, 6)
    cols = G.predict_sum(engine, nodes, noises, lw, tp, G.Periodic, y_transform=(a, b), quantiles=[0.1, 0.9])
    ref = R.predict_sum([[s.to_tuple() for s in sp] for sp in splits], noises, lw, ts[:n_fit], xs[:n_fit], tp, y_transform=(a, b),
                        quantiles=[0.1, 0.9])
    assert list(cols) == list(ref)
    for k in ("ds", "component", "particle"):
        assert np.array_equal(cols[k], ref[k]), k
    assert np.allclose(cols["weight"], ref["weight"], rtol=1e-14)
    for k in ("y_mean", "y_0.1", "y_0.9"):
        close(cols[k], ref[k], k)
    comps, w, idx = G.predict_mvn_sum(engine, nodes[:2], noises[:2], lw[:2], tp, G.Periodic, y_transform=(a, b))
    rc, ridx = R.predict_mvn_sum([[s.to_tuple() for s in sp] for sp in splits[:2]], noises[:2], ts[:n_fit], xs[:n_fit], tp,
                                 y_transform=(a, b))
    assert idx == ridx
    for d, (m, S) in zip(comps, rc):
        close(d.mean(), m, "mvn mean"); close(d.cov(), S, "mvn cov")


def test_non_pd_particle_only_nans_itself(pkg, engine):
    G = pkg
    nodes, noises, splits = population(pkg, 31, 5, "Linear")
    ts, xs = series(pkg, "irregular", 140, 8)
    engine.set_data(ts, xs)
    tp = np.linspace(0.0, 1.1, 13)
    bad = [G.Constant(1.0), G.Constant(0.5)]          # rank one without noise: the second pivot is exactly 0
    sp = splits[:2] + [bad] + splits[2:]
    nz = np.concatenate([noises[:2], [0.0], noises[2:]])
    mean, var, cov, info, _, _ = engine.infer_gp_sum_batch(sp, nz, tp, want_cov=True, check=False)
    assert info[2] > 0 and (np.delete(info, 2) == 0).all()
    assert np.isnan(mean[2]).all() and np.isnan(var[2]).all() and np.isnan(cov[2]).all()
    ref = engine.infer_gp_sum_batch(splits, noises, tp, want_cov=True)
    for a, b in zip((mean, var, cov), ref[:3]):
        assert np.array_equal(np.delete(a, 2, axis=0), b)
    m2, x2, info2 = engine.predict_sum_batch(sp, nz, tp, q=[0.5], check=False)
    assert info2[2] == info[2] and np.isnan(m2[2]).all() and np.isnan(x2[2]).all() and np.isfinite(np.delete(x2, 2, axis=0)).all()
    with pytest.raises(pkg.PosDefException):
        engine.infer_gp_sum_batch(sp, nz, tp)
    # a raw row that fails: a noise_pred that drives the observable variance negative -> info = n + j (first X row)
    m3, x3, info3 = engine.predict_sum_batch(splits[:2], noises[:2], tp, q=[0.5], noise_pred=-1e6, check=False)
    n = ts.shape[0]
    assert (info3 == n + 2 * tp.shape[0] + 1).all() and np.isnan(x3).all()


def test_program_limits_and_argument_errors(pkg, engine):
    G = pkg
    ts, xs = series(pkg, "irregular", 50, 1)
    engine.set_data(ts, xs)
    tp = np.linspace(0.0, 1.0, 5)
    ok = [G.SquaredExponential(0.3, 1.0), G.Periodic(0.5, 0.3, 1.0)]
    big = G.Linear(0.1) + G.Periodic(0.2, 0.3)
    for _ in range(5):
        big = big * big
    long_split = list(G.split_kernel_sop(big, G.Periodic))
    assert sum(len(G.unroll(x)) for x in long_split) > 255
    with pytest.raises(pkg.AGPError, match="particle 2"):
        engine.infer_gp_sum_batch([ok, ok, long_split], [0.1] * 3, tp)
    with pytest.raises(pkg.AGPError, match="particle 1"):
        engine.predict_sum_batch([ok, long_split], [0.1] * 2, tp)
    with pytest.raises(pkg.AGPError, match=r"\(0, 1\)"):
        engine.predict_sum_batch([ok], [0.1], tp, q=[0.5, 1.0])
    with pytest.raises(pkg.AGPError, match=r"\(0, 1\)"):
        engine.predict_sum_batch([ok], [0.1], tp, q=[0.0])
    for yt in ((0.0, 0.0), (np.inf, 0.0), (1.0, np.nan)):
        with pytest.raises(pkg.AGPError, match="y_transform"):
            engine.predict_sum_batch([ok], [0.1], tp, q=[0.5], y_transform=yt)
    with pytest.raises(pkg.AGPError, match="n exceeds"):
        engine.infer_gp_sum_batch([ok], [0.1], tp, n=51)
    with pytest.raises(pkg.AGPError, match="M must be"):
        engine.infer_gp_sum_batch([[G.Constant(1.0)] * 201], [0.1], tp)
    with pytest.raises(pkg.AGPError, match="P must be"):
        engine.infer_gp_sum_batch([], np.zeros(0), tp)
    mean, var, cov, info, _, _ = engine.infer_gp_sum_batch([ok], [0.1], np.zeros(0), want_cov=True)
    assert mean.shape == (1, 0) and cov.shape == (1, 0, 0)


def test_poison_mode_bitwise(pkg, monkeypatch):
    """AGP_POISON=1: every value buffer the entries read is NaN until written; clean and poisoned engines bitwise equal."""
    out = []
    nodes, noises, splits = population(pkg, 41, 6, "SquaredExponential")
    ts, xs = series(pkg, "irregular", 145, 3)
    tp = np.linspace(0.5, 1.3, 37)
    for poison in ("1", "0"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        try:
            e.set_data(ts, xs)
            f0 = e.poison_stats()["fills"]
            r = engine_results(e, splits + splits[:2], np.concatenate([noises, noises[:2]]), tp)
            if poison == "1":
                assert e.poison_stats()["fills"] > f0
            out.append(r)
        finally:
            e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)
        assert np.isfinite(a).all()


def engine_results(e, splits, noises, tp):
    m, v, c, _, _, _ = e.infer_gp_sum_batch(splits, noises, tp, want_cov=True, noise_pred=0.01)
    mr, x, _ = e.predict_sum_batch(splits, noises, tp, q=[0.1, 0.9], y_transform=(1.7, 0.2))
    return m, v, c, mr, x
