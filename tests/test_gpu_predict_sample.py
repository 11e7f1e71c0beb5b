"""Posterior predictive samples on the GPU (agp_predict_sample_batch; rand(predict_mvn(model, ds), N), src/api.jl:497-522): the algebra
given (component, z) against oracle.predict_mvn, the seeded draws against the restatement of tests/_pred_sample_ref.py, bitwise
invariance of a sample under S, order, copies and chunking, the mixture's moments, failures, argument errors and poison mode."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _pred_sample_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

NS = [0, 1, 127, 128, 129, 257, 1000]
MS = [1, 17, 128, 129, 300]
QUERY_KINDS = ("future", "interleaved", "training")


def fixture_kernels(G):
    base = [G.WhiteNoise(1), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
            G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1)]      # test/test_GP.jl:24-33
    return base + [base[2] + base[5], base[3] * base[4], G.ChangePoint(base[2], base[5], 0.5, 0.05),
                   G.ChangePoint(base[3] + base[4], base[2] * base[5], 0.3, 0.2)]


def queries(kind, ts, n, m, rng):
    if kind == "training" and n > 0:
        return ts[rng.integers(0, n, m)].copy()
    if kind == "interleaved":
        return rng.random(m)
    return 1.0 + 0.3 * np.arange(1, m + 1) / max(m, 1)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def raw_oracle(node, noise, ts, xs, tp, npred, a, b):
    mu, cv = O.predict_mvn(node.to_tuple(), float(noise), ts, xs, tp, noise_pred=npred)
    return (mu - b) / a, cv / (a * a)


def uniform_w(P):
    return np.full(P, 1.0 / P)


def test_algebra_given_component_and_z(pkg, engine):
    """z = I on a series with xs = 0 (raw mean exactly 0) gives the columns of L / |a|; z = 0 the raw mean; random z mu + chol(cov) z."""
    G = pkg
    nodes = fixture_kernels(G)
    P = len(nodes)
    noises = np.full(P, 0.2)
    rng = np.random.default_rng(17)
    ts_all = np.sort(rng.random(max(NS))); xs_all = 0.5 * rng.standard_normal(max(NS))
    c = 0
    n_zero_checked = 0
    for n in NS:
        ts, xs = ts_all[:n], xs_all[:n]
        for m in MS:
            for kind in QUERY_KINDS:
                c += 1
                tp = queries(kind, ts, n, m, rng)
                slope = (1.7, -2.5, 0.4, -0.8)[c % 4]
                npred = [None, 0.05 + 0.1 * rng.random(P)][c % 2]
                npp = lambda p: None if npred is None else float(npred[p])      # noqa: E731
                check = [(c + k) % P for k in range(3)]
                # L from z = I_m: S = m P samples, component p for the p-th block of m
                engine.set_data(ts, np.zeros(n))
                comp = np.repeat(np.arange(P, dtype=np.int32), m)
                x, cout, info = engine.predict_sample_batch(nodes, noises, tp, uniform_w(P), m * P, n=n, noise_pred=npred,
                                                            y_transform=(slope, 0.0), component=comp, z=np.tile(np.eye(m), P))
                assert np.array_equal(cout, comp) and (info == 0).all()
                for p in check:
                    L = x[:, p * m:(p + 1) * m]
                    assert (np.triu(L, 1) == 0).all() and (np.diag(L) > 0).all(), (n, m, kind, p)
                    _, cr = raw_oracle(nodes[p], noises[p], ts, np.zeros(n), tp, npp(p), slope, 0.0)
                    err = np.linalg.norm(L @ L.T - cr)
                    assert err <= 1e-10 * np.linalg.norm(cr), (n, m, kind, p, err)
                if kind != "training" and m <= 17:
                    # noise_pred = 0: the backward error holds wherever the factor exists
                    for p in check:
                        x1, _, i1 = engine.predict_sample_batch([nodes[p]], noises[p:p + 1], tp, [1.0], m, n=n, noise_pred=0.0,
                                                                y_transform=(slope, 0.0), component=np.zeros(m, np.int32), z=np.eye(m),
                                                                check=False)
                        if i1[0] != 0:
                            assert np.isnan(x1).all()
                            continue
                        _, cr = raw_oracle(nodes[p], noises[p], ts, np.zeros(n), tp, 0.0, slope, 0.0)
                        assert (np.triu(x1, 1) == 0).all()
                        assert np.linalg.norm(x1 @ x1.T - cr) <= 1e-10 * np.linalg.norm(cr), (n, m, kind, p, "noise_pred 0")
                        n_zero_checked += 1
                # raw mean (z = 0) and random z on the real series
                engine.set_data(ts, xs)
                b = 0.3
                comp = np.arange(P, dtype=np.int32)
                x0, _, _ = engine.predict_sample_batch(nodes, noises, tp, uniform_w(P), P, n=n, noise_pred=npred, y_transform=(slope, b),
                                                       component=comp, z=np.zeros((m, P)))
                Z = rng.standard_normal((m, 2 * P))
                xr, _, _ = engine.predict_sample_batch(nodes, noises, tp, uniform_w(P), 2 * P, n=n, noise_pred=npred,
                                                       y_transform=(slope, b), component=np.tile(comp, 2), z=Z)
                for p in check:
                    mr, cr = raw_oracle(nodes[p], noises[p], ts, xs, tp, npp(p), slope, b)
                    assert np.abs(x0[:, p] - mr).max() <= 1e-8 * max(1.0, np.abs(mr).max()), (n, m, kind, p)
                    Lo = np.linalg.cholesky(cr)
                    for s in (p, p + P):
                        want = mr + Lo @ Z[:, s]
                        scale = np.abs(mr) + np.abs(Lo) @ np.abs(Z[:, s])
                        assert (np.abs(xr[:, s] - want) <= 1e-8 * scale).all(), (n, m, kind, p, s)
    assert n_zero_checked >= 10


def population(pkg):
    G = pkg
    nodes = [G.SquaredExponential(0.3, 1.0), G.Periodic(0.4, 0.2, 1.0) + G.Linear(0.2), G.Constant(0.5) * G.SquaredExponential(0.1, 1.0),
             G.GammaExponential(0.2, 0.8, 1.5), G.SquaredExponential(0.05, 0.7) + G.WhiteNoise(0.1)]
    noises = np.array([0.1, 0.2, 0.15, 0.1, 0.3])
    return nodes, noises


def test_seeded_draws_against_restatement(pkg, engine):
    rng = np.random.default_rng(3)
    n, m, S, seed = 129, 17, 1000, 987654321
    ts = np.sort(rng.random(n)); xs = 0.5 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    nodes, noises = population(pkg)
    w = np.array([0.1, 0.0, 0.25, 0.4, 0.25])
    tp = np.concatenate([ts[:5], 1.0 + 0.02 * np.arange(m - 5)])
    yt = (-1.3, 0.4)
    x, comp, info = engine.predict_sample_batch(nodes, noises, tp, w, S, seed=seed, noise_pred=0.05, y_transform=yt)
    assert (info == 0).all()
    assert np.array_equal(comp, R.components(seed, w, S))
    assert 1 not in comp
    zr = R.normals(seed, m, range(S))
    x2, _, _ = engine.predict_sample_batch(nodes, noises, tp, w, S, noise_pred=0.05, y_transform=yt, component=comp, z=zr)
    for p in set(comp.tolist()):
        mr, cr = raw_oracle(nodes[p], noises[p], ts, xs, tp, 0.05, *yt)
        La = np.abs(np.linalg.cholesky(cr))
        sel = np.nonzero(comp == p)[0]
        scale = np.abs(mr)[:, None] + La @ np.abs(zr[:, sel])
        assert (np.abs(x[:, sel] - x2[:, sel]) <= 1e-12 * scale).all(), p
        # and the draws are the predictive's: mu + chol(cov) z
        assert (np.abs(x[:, sel] - (mr[:, None] + np.linalg.cholesky(cr) @ zr[:, sel])) <= 1e-8 * scale).all(), p
    xa, ca, _ = engine.predict_sample_batch(nodes, noises, tp, w, S, seed=seed, noise_pred=0.05, y_transform=yt)
    assert same(xa, x) and np.array_equal(ca, comp)
    x10, c10, _ = engine.predict_sample_batch(nodes, noises, tp, w, 10, seed=seed, noise_pred=0.05, y_transform=yt)
    assert same(x10, x[:, :10]) and np.array_equal(c10, comp[:10])
    xo, _, _ = engine.predict_sample_batch(nodes, noises, tp, w, S, seed=seed + 1, noise_pred=0.05, y_transform=yt)
    assert not np.array_equal(xo, x)


def test_bitwise_invariance_order_copies_chunking(pkg, engine):
    rng = np.random.default_rng(8)
    n, m, S, seed = 300, 140, 400, 5
    ts = np.sort(rng.random(n)); xs = 0.5 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    nodes, noises = population(pkg)
    P = len(nodes)
    tp = np.concatenate([rng.random(m // 2), 1.0 + 0.01 * np.arange(m - m // 2)])
    w = uniform_w(P)
    comp = rng.integers(0, P, S).astype(np.int32)
    x, _, _ = engine.predict_sample_batch(nodes, noises, tp, w, S, seed=seed, component=comp, noise_pred=0.1)
    perm = rng.permutation(P)
    inv = np.argsort(perm)
    xp, _, _ = engine.predict_sample_batch([nodes[i] for i in perm], noises[perm], tp, w, S, seed=seed, component=inv[comp].astype(np.int32),
                                           noise_pred=0.1)
    assert same(xp, x)
    # copies: [A, A, B, ...]; samples of A drawn to either copy read the shared factor
    dn = [nodes[0]] + nodes; dz = np.concatenate([noises[:1], noises])
    dcomp = (comp + 1).astype(np.int32)
    dcomp[(comp == 0) & (np.arange(S) % 2 == 0)] = 0
    d0 = engine.dedup_stats()
    xd, _, _ = engine.predict_sample_batch(dn, dz, tp, uniform_w(P + 1), S, seed=seed, component=dcomp, noise_pred=0.1)
    d1 = engine.dedup_stats()
    assert same(xd, x)
    assert d1[0] - d0[0] == P + 1 and d1[1] - d0[1] == P
    # one particle per chunk
    nt = -(-n // 128) - (-m // 128)
    engine.set_workspace_limit(nt * (nt + 1) // 2 * 128 * 128 * 8)
    try:
        xc, _, _ = engine.predict_sample_batch(nodes, noises, tp, w, S, seed=seed, component=comp, noise_pred=0.1)
    finally:
        engine.set_workspace_limit(0)
    assert same(xc, x)
    # one sample alone
    x1, _, _ = engine.predict_sample_batch(nodes, noises, tp, w, 1, seed=seed, component=comp[:1], noise_pred=0.1)
    assert same(x1, x[:, :1])
    assert np.isfinite(x).all()


def mixture_moments(mus, covs, w):
    mean = sum(wp * mp for wp, mp in zip(w, mus))
    second = sum(wp * (cp + np.outer(mp, mp)) for wp, mp, cp in zip(w, mus, covs))
    return mean, second - np.outer(mean, mean)


def check_moments(x, mean, cov, ctx):
    S = x.shape[1]
    xm = x.mean(axis=1)
    assert (np.abs(xm - mean) <= 5 * np.sqrt(np.diag(cov) / S)).all(), (ctx, xm, mean)
    d = x - mean[:, None]
    m = x.shape[0]
    for i in range(m):
        for j in range(i + 1):
            prod = d[i] * d[j]
            assert abs(prod.mean() - cov[i, j]) <= 5 * prod.std() / np.sqrt(S), (ctx, i, j, prod.mean(), cov[i, j])


def test_mixture_distribution(pkg, engine):
    G = pkg
    rng = np.random.default_rng(12)
    n, S = 60, 200_000
    ts = np.sort(rng.random(n)); xs = np.sin(6 * ts) + 0.1 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    nodes = [G.SquaredExponential(0.2, 1.0), G.SquaredExponential(0.05, 0.5) + G.Linear(0.3), G.Periodic(0.3, 0.4, 1.0)]
    noises = np.array([0.05, 0.1, 0.2])
    w = np.array([0.3, 0.0, 0.7])
    tp = np.array([0.5, 1.05, 1.3])
    yt = (2.0, -0.5)
    x, comp, info = engine.predict_sample_batch(nodes, noises, tp, w, S, seed=42, y_transform=yt)
    assert (info == 0).all() and 1 not in comp
    f = (comp == 0).mean()
    assert abs(f - 0.3) <= 5 * math.sqrt(0.21 / S)
    mus, covs = zip(*[raw_oracle(nodes[p], noises[p], ts, xs, tp, None, *yt) for p in range(3)])
    mean, cov = mixture_moments(mus, covs, w)
    check_moments(x, mean, cov, "mixture")
    # the prior (n = 0): K + noise I, the tutorials' synthetic data; MvNormal.rand is that route
    d = pkg.MvNormal(nodes[0], 0.05, [], [], tp, engine=engine)
    xp = d.rand(S, seed=7)
    check_moments(xp, np.zeros(3), O.compute_cov_matrix_vectorized(nodes[0].to_tuple(), 0.05, tp), "prior")
    v = d.rand()
    assert v.shape == (3,) and np.isfinite(v).all()


def test_predict_rand_route(pkg, engine):
    rng = np.random.default_rng(1)
    n = 100
    ts = np.sort(rng.random(n)); xs = 0.5 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    nodes, noises = population(pkg)
    lw = np.log(np.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    tp = 1.0 + 0.01 * np.arange(20)
    x = pkg.predict_rand(engine, nodes, noises, lw, tp, 50, seed=3, y_transform=(1.5, 0.2), noise_pred=0.05)
    w = np.exp(pkg.dist.normalize_weights(lw)[1])
    x2, _, _ = engine.predict_sample_batch(nodes, noises, tp, w, 50, seed=3, y_transform=(1.5, 0.2), noise_pred=0.05)
    assert x.shape == (20, 50) and same(x, x2)
    v = pkg.predict_rand(engine, nodes, noises, lw, tp, seed=3, y_transform=(1.5, 0.2), noise_pred=0.05)
    assert v.shape == (20,) and same(v, x2[:, 0])
    e, c, i = engine.predict_sample_batch(nodes, noises, tp, w, 0)
    assert e.shape == (20, 0)
    e, c, i = engine.predict_sample_batch(nodes, noises, np.zeros(0), w, 5)
    assert e.shape == (0, 5)


def failing_population(pkg):
    G = pkg
    rng = np.random.default_rng(6)
    n, m = 150, 40
    ts = np.sort(rng.random(n)); xs = 0.5 * rng.standard_normal(n)
    good = [G.SquaredExponential(0.3, 1.0), G.Periodic(0.4, 0.2, 1.0) + G.Linear(0.2), G.Constant(0.5) * G.SquaredExponential(0.1, 1.0)]
    # (test_gpu_predict_logpdf.py::test_failures_are_isolated: SE(0.001, 1) at two queries t = 5 with noise_pred = 0: minor 2 vanishes)
    tp = np.concatenate([[5.0, 5.0], 1.0 + 0.01 * np.arange(m - 2)])
    nodes = [good[0], G.SquaredExponential(0.3, 1.0), good[1], good[2], G.SquaredExponential(0.001, 1.0)]
    return ts, xs, tp, nodes, n


def test_failures(pkg, engine):
    ts, xs, tp, nodes, n = failing_population(pkg)
    engine.set_data(ts, xs)
    w = uniform_w(5)
    for noises, npred, bad, want in ((np.array([0.1, -5.0, 0.1, 0.1, 0.1]), np.full(5, 0.05), 1, None),
                                     (np.full(5, 0.1), np.array([0.05, 0.05, 0.05, 0.05, 0.0]), 4, n + 2)):
        x, comp, info = engine.predict_sample_batch(nodes, noises, tp, w, 30, seed=1, noise_pred=npred, check=False)
        if want is None:
            assert 1 <= info[bad] <= n
        else:
            assert info[bad] == want
        assert (np.delete(info, bad) == 0).all()
        assert np.isnan(x).all() and x.shape == (len(tp), 30)
        with pytest.raises(pkg.PosDefException):
            engine.predict_sample_batch(nodes, noises, tp, w, 30, seed=1, noise_pred=npred)
        with pytest.raises(pkg.PosDefException):
            pkg.predict_rand(engine, nodes, noises, np.zeros(5), tp, 30, noise_pred=float(npred[bad]))


def test_argument_errors(pkg, engine):
    G = pkg
    engine.set_data(np.linspace(0, 1, 50), np.zeros(50))
    k = [G.SquaredExponential(0.3, 1.0), G.Linear(0.2)]
    tp = np.linspace(1, 2, 5); nz = [0.1, 0.1]
    w = np.array([0.5, 0.5])
    call = engine.predict_sample_batch
    assert call(k, nz, tp, w, 4)[0].shape == (5, 4)
    for kw, msg in ((dict(weights=np.array([0.5, 0.6])), "sum to 1"), (dict(weights=np.array([1.5, -0.5])), ">= 0"),
                    (dict(y_transform=(0.0, 0.0)), "slope"), (dict(y_transform=(np.inf, 0.0)), "slope"),
                    (dict(y_transform=(1.0, np.nan)), "intercept"),
                    (dict(component=np.array([0, 2, 1, 0])), "range"), (dict(component=np.array([0, -1, 1, 0])), "range"),
                    (dict(weights=np.array([1.0, 0.0]), component=np.array([0, 1, 0, 0])), "weight 0"),
                    (dict(n_samples=-1), "negative"), (dict(n=51), "n exceeds")):
        args = dict(weights=w, n_samples=4)
        args.update(kw)
        if "component" in kw:
            args["component"] = kw["component"].astype(np.int32)
        with pytest.raises(pkg.AGPError, match=msg):
            call(k, nz, tp, args.pop("weights"), args.pop("n_samples"), **args)
    with pytest.raises(pkg.AGPError, match="too large"):
        call(k, nz, np.linspace(1, 2, 1 << 16), w, 1 << 15)


def test_poison_mode_matches_clean(pkg, monkeypatch):
    rng = np.random.default_rng(13)
    engs = []
    for poison in ("1", "0"):
        monkeypatch.setenv("AGP_POISON", poison)
        engs.append(pkg.GPEngine(0))
        monkeypatch.delenv("AGP_POISON")
    ez, ec = engs
    try:
        ts, xs = pkg.prior.synthetic_series(400, seed=12, shuffle=True)
        nodes, noises = pkg.prior.sample_particles(rng, 12, max_depth=4)
        P = len(nodes)
        w = rng.random(P); w[3] = 0.0; w /= w.sum()
        for n, m, slope in ((0, 17, 1.0), (1, 1, -2.0), (129, 127, 0.5), (257, 129, -1.0), (300, 100, 1.3)):
            tp = np.concatenate([ts[n:n + m // 2], 1.0 + 0.01 * np.arange(m - m // 2)])
            Z = rng.standard_normal((m, 40))
            comp = np.nonzero(w > 0)[0][rng.integers(0, P - 1, 40)].astype(np.int32)
            res = []
            for e in (ez, ec):
                e.set_data(ts[:max(n, 1)], xs[:max(n, 1)])
                r1 = e.predict_sample_batch(nodes, noises, tp, w, 300, seed=9, n=n, noise_pred=0.5 * noises + 0.1,
                                            y_transform=(slope, 0.2), check=False)
                r2 = e.predict_sample_batch(nodes, noises, tp, w, 40, n=n, noise_pred=0.5 * noises + 0.1, y_transform=(slope, 0.2),
                                            component=comp, z=Z, check=False)
                nt = -(-n // 128) - (-m // 128)
                e.set_workspace_limit(nt * (nt + 1) // 2 * 128 * 128 * 8)
                try:
                    r3 = e.predict_sample_batch(nodes, noises, tp, w, 300, seed=9, n=n, noise_pred=0.5 * noises + 0.1,
                                                y_transform=(slope, 0.2), check=False)
                finally:
                    e.set_workspace_limit(0)
                res.append((r1, r2, r3))
            for (xz, cz, iz), (xc, cc, ic) in zip(*res):
                assert same(xz, xc) and np.array_equal(cz, cc) and np.array_equal(iz, ic), (n, m)
                assert (ic != 0).any() or np.isfinite(xz).all(), (n, m)
            assert same(res[1][0][0], res[1][2][0])
        assert ez.poison_stats()["bytes"] > 0
        # a failing particle: NaN everywhere on both engines
        ts2, xs2, tp2, nodes2, n2 = failing_population(pkg)
        outs = []
        for e in (ez, ec):
            e.set_data(ts2, xs2)
            outs.append(e.predict_sample_batch(nodes2, np.array([0.1, -5.0, 0.1, 0.1, 0.1]), tp2, uniform_w(5), 20, noise_pred=0.05,
                                               check=False))
        assert np.array_equal(outs[0][2], outs[1][2]) and np.isnan(outs[0][0]).all() and np.isnan(outs[1][0]).all()
    finally:
        ez.close(); ec.close()
