"""GPU tests of agp_predict_sample_series_batch (sample paths and joint forecasts of many short series in one fused launch;
k_series_predict_sample and k_series_sample_fill, csrc/agp_series_kernel.hpp).

Reference: oracle.predict_mvn (the reference's op order, LU solves) + np.linalg.cholesky.  Bounds, the resident sample tests' own:
|x - ref| <= 1e-8 max(1, max|ref|) per sample, out_mean to 1e-8 max(1, max|ref|), ||cov - ref||_F <= 1e-10 ||ref||_F, cov == cov.T
bitwise.  The inputs (synthetic series on [0, 1], noises of 0.1 .. 0.2 on kernels of unit scale) keep every Sigma* well inside the
range where two CPU routes — the oracle's LU route and a LAPACK Cholesky of the joint matrix read out as the kernel reads it — agree
within those bounds: cpu_routes_agree() asserts it for every particle of the algebra case, without a GPU, and reports the worst
ratio of their difference to each bound (measured: 2.1e-6 of the sample bound, 1.1e-6 of the mean bound, 1.9e-4 of the covariance
bound).  No particle is skipped: the reference factors every particle (np.linalg.cholesky raises otherwise) unless the test is
about failure."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

import _pred_sample_ref as PS
import _series_sample_ref as R
import test_gpu_series as TS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
bits = TS.bits
TOL_X, TOL_COV = 1e-8, 1e-10

# (training points, query points): both ends of the cap, the prior, splits 0, 1, 15 of a block ...
SHAPES = ((0, 1), (0, 17), (1, 1), (15, 1), (16, 16), (17, 15), (31, 33), (100, 76), (175, 1), (1, 175), (160, 16))
# ... whose joint lengths end in 1, 2, 4 or 11 blocks of 16: here 3, 5, 6, 7, 8, 9 and 10
MORE_SHAPES = ((20, 20), (60, 15), (50, 40), (97, 10), (100, 25), (130, 9), (3, 150))
R_VALUES = (1, 16, 17, 33)


def stack_depth(pkg, node):
    """evaluation-stack depth of the encoded (postfix) program: the value kernels take the depth-8 instantiation above 4"""
    sp = depth = 0
    for o in pkg.encode(node)[0]:
        sp += -1 if int(o) >= 6 else 1                     # opcodes 6, 7, 8: Plus, Times, ChangePoint (include/autogp_hip.h)
        depth = max(depth, sp)
    return depth


def kernels(G):
    se = G.SquaredExponential(0.47, 0.9)
    pl = G.Periodic(0.96, 0.21, 0.8) * G.Linear(0.1, 1.3, 0.7)
    leafs = [G.SquaredExponential(0.3, 0.5), G.Linear(0.2, 0.4, 0.6), G.Periodic(0.5, 0.3, 0.7), G.Constant(0.4),
             G.GammaExponential(0.42, 0.58, 1.2)]
    chain = leafs[4]
    for k in (3, 2, 1, 0):                                # right-nested: the evaluation stack grows by one per ChangePoint
        chain = G.ChangePoint(leafs[k], chain, 0.2 + 0.15 * k, 0.05)
    wide = TS.full_tree(G, 3) + TS.full_tree(G, 2, 1)
    assert wide.size() == 23
    return [se, pl, chain, wide]


def build_case(shapes, seed0=900):
    """one series per shape (a prefix of a shuffled synthetic series; queries inside and beyond it, one of them on a training time),
    the four kernels on each, slopes of both signs"""
    import __graft_entry__ as g
    G = g.load_package()
    ks = kernels(G)
    assert stack_depth(G, ks[2]) > 4 >= stack_depth(G, ks[0])
    series, queries, nodes, noises, sidx, yts = [], [], [], [], [], []
    for s, (n, m) in enumerate(shapes):
        ts, xs = G.prior.synthetic_series(256, seed=seed0 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        rng = np.random.default_rng(seed0 + 50 + s)
        tq = np.sort(rng.random(m) * 1.3 - 0.1)
        if n and m > 1:
            tq[m // 2] = ts[0]
        queries.append(tq)
        nodes += ks; noises += [0.1, 0.15, 0.2, 0.12]; sidx += [s] * 4
        yts.append((2.0, 0.3) if s % 2 == 0 else (-0.5, -1.25))
    return series, queries, nodes, np.array(noises), np.array(sidx, dtype=np.int32), np.array(yts)


@functools.lru_cache(maxsize=None)
def algebra_case():
    """The shared case and its CPU reference (computed once, never modified): per particle (mu*, Sigma*, chol(Sigma*))"""
    case = build_case(SHAPES + MORE_SHAPES)
    series, queries, nodes, noises, sidx, yts = case
    assert {(n + m + 15) // 16 for n, m in SHAPES + MORE_SHAPES} == set(range(1, 12))
    ref = []
    for p, nd in enumerate(nodes):
        s = int(sidx[p])
        mu, Sg = O.predict_mvn(nd.to_tuple(), float(noises[p]), *series[s], queries[s])
        Lc = np.linalg.cholesky(Sg)                        # (raises where the reference has no predictive: none is skipped)
        for a in (mu, Sg, Lc):
            a.setflags(write=False)
        ref.append((mu, Sg, Lc))
    return case, ref


def cpu_routes_agree():
    """the oracle's LU route against a LAPACK Cholesky of the joint matrix read out as the kernel reads it, in units of each bound"""
    (series, queries, nodes, noises, sidx, yts), ref = algebra_case()
    worst = np.zeros(3)
    rng = np.random.default_rng(1)
    for p, nd in enumerate(nodes):
        s = int(sidx[p])
        (ts, xs), tq = series[s], queries[s]
        n, m = len(ts), len(tq)
        K = O.compute_cov_matrix_vectorized(nd.to_tuple(), 0.0, np.concatenate([ts, tq])) + float(noises[p]) * np.eye(n + m)
        L = np.linalg.cholesky(K)
        mu2 = L[n:, :n] @ np.linalg.solve(L[:n, :n], xs) if n else np.zeros(m)
        S2 = L[n:, n:] @ L[n:, n:].T
        mu, Sg, Lc = ref[p]
        z = rng.standard_normal((m, 4))
        xa, xb = mu[:, None] + Lc @ z, mu2[:, None] + L[n:, n:] @ z
        worst = np.maximum(worst, [np.abs(xa - xb).max() / (TOL_X * max(1.0, np.abs(xa).max())),
                                   np.abs(mu - mu2).max() / (TOL_X * max(1.0, np.abs(mu).max())),
                                   np.linalg.norm(Sg - S2) / (TOL_COV * np.linalg.norm(Sg))])
    return worst


def raw(mu, Lc, z, yt):
    a, b = yt
    return (mu[:, None] + np.sign(a) * (Lc @ z) - b) / a


def weights_of(sidx, skip=None):
    """uniform over the particles of each series, those in `skip` at 0"""
    sidx = np.asarray(sidx)
    live = np.ones(len(sidx), dtype=bool)
    if skip is not None:
        live[list(skip)] = False
    return np.array([live[p] / (live & (sidx == sidx[p])).sum() for p in range(len(sidx))])


def obits(r):
    """every floating-point output of a call as one int64 vector"""
    parts = [bits(np.ascontiguousarray(x)).ravel() for x in r.x]
    if r.mean is not None:
        parts += [bits(a).ravel() for a in r.mean] + [bits(np.ascontiguousarray(c)).ravel() for c in r.cov]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def test_algebra_with_caller_component_and_z(pkg, engine):
    (series, queries, nodes, noises, sidx, yts), ref = algebra_case()
    cpu = cpu_routes_agree()
    print("[series-sample] CPU routes, worst difference in units of the bounds (x, mean, cov):", cpu)
    assert (cpu < 0.01).all(), cpu
    S, P = len(series), len(nodes)
    plist = [np.flatnonzero(sidx == s) for s in range(S)]
    rng = np.random.default_rng(3)
    worst = np.zeros(3)
    for Rn in R_VALUES:
        # particle s % 4 of series s has no sample; the others take them in turn
        comp = np.array([[plist[s][(s + 1 + j % 3) % 4] for j in range(Rn)] for s in range(S)], dtype=np.int32)
        z = [rng.standard_normal((len(q), Rn)) for q in queries]
        r = engine.predict_sample_series_batch(series, queries, nodes, noises, sidx, weights_of(sidx), Rn, y_transforms=yts,
                                               component=comp, z=z, want_moments=True)
        assert (r.info == 0).all() and np.array_equal(r.component, comp)
        for s in range(S):
            assert r.x[s].shape == (len(queries[s]), Rn)
            assert not (comp[s] == plist[s][s % 4]).any()
            for j in range(Rn):
                mu, Sg, Lc = ref[comp[s, j]]
                want = raw(mu, Lc, z[s][:, j:j + 1], yts[s])[:, 0]
                err = np.abs(r.x[s][:, j] - want).max() / max(1.0, np.abs(want).max())
                worst[0] = max(worst[0], err)
                assert err <= TOL_X, (Rn, s, j, err)
        for p in range(P):
            mu, Sg, Lc = ref[p]
            a, b = yts[sidx[p]]
            want = (mu - b) / a
            e1 = np.abs(r.mean[p] - want).max() / max(1.0, np.abs(want).max())
            e2 = np.linalg.norm(r.cov[p] - Sg / a ** 2) / np.linalg.norm(Sg / a ** 2)
            worst[1:] = np.maximum(worst[1:], [e1, e2])
            assert e1 <= TOL_X and e2 <= TOL_COV, (Rn, p, e1, e2)
            assert np.array_equal(bits(np.ascontiguousarray(r.cov[p])), bits(np.ascontiguousarray(r.cov[p].T)))
    print("[series-sample] algebra: worst x, mean (relative to max(1, max|ref|)), cov (relative Frobenius):", worst)


@pytest.fixture(scope="module")
def seeded(engine):
    """three series of the algebra case drawn under their own seeds, one particle of each at weight 0"""
    (series, queries, nodes, noises, sidx, yts), ref = algebra_case()
    sel_s = [SHAPES.index((17, 15)), SHAPES.index((31, 33)), SHAPES.index((0, 17))]
    sel_p = np.concatenate([np.flatnonzero(sidx == s) for s in sel_s])
    sub = ([series[s] for s in sel_s], [queries[s] for s in sel_s], [nodes[p] for p in sel_p], noises[sel_p],
           np.repeat(np.arange(3, dtype=np.int32), 4), yts[sel_s])
    w = np.tile([0.5, 0.0, 0.125, 0.375], 3)
    seeds = np.array([7, 2 ** 63 + 11, 0], dtype=np.uint64)
    Rn = 20
    r = engine.predict_sample_series_batch(*sub[:5], w, Rn, seeds=seeds, y_transforms=sub[5], want_moments=True)
    return sub, [ref[p] for p in sel_p], w, seeds, Rn, r


def test_seeded_draws(seeded):
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    for s in range(3):
        comp = PS.components(int(seeds[s]), w[4 * s:4 * s + 4], Rn) + 4 * s
        assert np.array_equal(r.component[s], comp)
        z = PS.normals(int(seeds[s]), len(queries[s]), range(Rn))
        for j in range(Rn):
            mu, Sg, Lc = ref[comp[j]]
            want = raw(mu, Lc, z[:, j:j + 1], yts[s])[:, 0]
            assert np.abs(r.x[s][:, j] - want).max() <= TOL_X * max(1.0, np.abs(want).max()), (s, j)


def test_cross_route(engine, seeded):
    """per series, agp_set_data + agp_predict_sample_batch(seed = seeds[s]): identical components, x within the bound; the
    components' means and variances against agp_predict_series_batch"""
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    for s in range(3):
        sel = slice(4 * s, 4 * s + 4)
        engine.set_data(*series[s])
        x, comp, info = engine.predict_sample_batch(nodes[sel], noises[sel], queries[s], w[sel], Rn, seed=int(seeds[s]),
                                                    y_transform=tuple(yts[s]))
        assert (info == 0).all() and np.array_equal(comp + 4 * s, r.component[s])
        assert (np.abs(x - r.x[s]).max(axis=0) <= TOL_X * np.maximum(1.0, np.abs(x).max(axis=0))).all(), s
    means, vars_, info = engine.predict_series_batch(series, queries, nodes, noises, sidx)
    for p in range(12):
        a, b = yts[sidx[p]]
        want_m, want_v = (means[p] - b) / a, vars_[p] / a ** 2
        assert np.abs(r.mean[p] - want_m).max() <= TOL_X * max(1.0, np.abs(want_m).max())
        assert np.abs(np.diag(r.cov[p]) - want_v).max() <= TOL_X * max(1.0, np.abs(want_v).max())


def test_bitwise_independence(engine, seeded):
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    call = lambda ss, pp, si, R_=Rn, mom=True: engine.predict_sample_series_batch(
        [series[s] for s in ss], [queries[s] for s in ss], [nodes[p] for p in pp], noises[pp], si, w[pp], R_,
        seeds=seeds[ss], y_transforms=yts[ss], want_moments=mom)
    allp = np.arange(12)
    # the series in reverse order (the particles of a series keep their order: the inverse CDF of the components runs over them)
    back = np.array([8, 9, 10, 11, 4, 5, 6, 7, 0, 1, 2, 3])
    rev = call([2, 1, 0], back, np.repeat(np.arange(3, dtype=np.int32), 4))
    for s in range(3):
        assert np.array_equal(bits(rev.x[2 - s]), bits(r.x[s]))
        assert np.array_equal(back[rev.component[2 - s]], r.component[s])
    for k, p in enumerate(back):
        assert np.array_equal(bits(rev.mean[k]), bits(r.mean[p])) and np.array_equal(bits(rev.cov[k]), bits(r.cov[p]))
    # each series alone
    for s in range(3):
        one = call([s], allp[4 * s:4 * s + 4], np.zeros(4, dtype=np.int32))
        assert np.array_equal(bits(one.x[0]), bits(r.x[s])) and np.array_equal(one.component[0] + 4 * s, r.component[s])
    # particles interleaved across the series (ascending order inside each series kept: the draws depend on it)
    perm = np.array([0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11])
    mix = call([0, 1, 2], perm, sidx[perm].copy())
    inv = np.argsort(perm)
    for s in range(3):
        assert np.array_equal(bits(mix.x[s]), bits(r.x[s])) and np.array_equal(perm[mix.component[s]], r.component[s])
    for p in range(12):
        assert np.array_equal(bits(mix.cov[inv[p]]), bits(r.cov[p]))
    # R = 5 against R = 40: the first five columns; moments requested or not
    few, many = call([0, 1, 2], allp, sidx, 5, False), call([0, 1, 2], allp, sidx, 40, True)
    assert few.mean is None
    for s in range(3):
        assert np.array_equal(bits(few.x[s]), bits(many.x[s][:, :5])) and np.array_equal(bits(r.x[s]), bits(many.x[s][:, :Rn]))
    assert np.array_equal(obits(many)[sum(x.size for x in many.x):], obits(r)[sum(x.size for x in r.x):])
    # the held-out entry factors the same joint matrices: its info words on the same input
    held = [np.zeros(len(q)) for q in queries]
    sc = engine.predict_logpdf_series_batch(series, queries, held, nodes, noises, sidx, check=False)
    assert np.array_equal(sc.info, r.info)


def test_failures(pkg, engine, seeded):
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    G = pkg
    # series 3: a repeated query time with noise_pred = 0 -> leading minor k of the predictive covariance fails (k = 4: 0-based 3)
    ts3, xs3 = series[0]
    q3 = np.array([0.11, 0.52, 0.93, 0.52, 0.7])
    n3 = len(ts3)
    # series 4: K11 itself fails (tests/_series_cases.changepoint_particle's construction on 40 points)
    ts4 = np.linspace(0.0, 1.0, 40)
    bad11 = G.ChangePoint(G.WhiteNoise(1.0), G.Constant(1e-3), ts4[9] - 0.5 / 39, 1e-4)
    for w_bad in (0.5, 0.0):
        ser = list(series) + [(ts3, xs3), (ts4, np.zeros(40))]
        qs = list(queries) + [q3, np.array([0.3, 1.1])]
        nd = list(nodes) + [G.SquaredExponential(0.5, 0.8), G.SquaredExponential(0.47, 0.9), G.Constant(0.5), bad11]
        nz = np.concatenate([noises, [0.1, 0.1, 0.1, -0.5]])
        si = np.concatenate([sidx, [3, 3, 4, 4]]).astype(np.int32)
        ww = np.concatenate([w, [1.0 - w_bad, w_bad, 1.0 - w_bad, w_bad]])
        npred = np.concatenate([noises, [0.1, 0.0, 0.1, 0.1]])
        yy = np.vstack([yts, [(1.0, 0.0), (3.0, 1.0)]])
        sd = np.concatenate([seeds, np.array([5, 6], dtype=np.uint64)])
        f = engine.predict_sample_series_batch(ser, qs, nd, nz, si, ww, Rn, seeds=sd, y_transforms=yy, noise_pred=npred,
                                               want_moments=True, check=False)
        assert f.info[:12].tolist() == [0] * 12 and f.info[12:].tolist() == [0, n3 + 4, 0, 10], f.info
        assert np.isnan(f.x[3]).all() and np.isnan(f.x[4]).all() and f.x[3].shape == (5, Rn)
        assert np.isnan(f.mean[13]).all() and np.isnan(f.cov[13]).all() and np.isnan(f.mean[15]).all() and np.isnan(f.cov[15]).all()
        assert np.isfinite(f.mean[12]).all() and np.isfinite(f.cov[12]).all() and np.isfinite(f.cov[14]).all()
        # the neighbours: bit-identical to the run without the failing series (noise_pred == noise there)
        for s in range(3):
            assert np.array_equal(bits(f.x[s]), bits(r.x[s])) and np.array_equal(f.component[s], r.component[s])
        for p in range(12):
            assert np.array_equal(bits(f.mean[p]), bits(r.mean[p])) and np.array_equal(bits(f.cov[p]), bits(r.cov[p]))
        with pytest.raises(pkg.PosDefException):
            engine.predict_sample_series_batch(ser, qs, nd, nz, si, ww, Rn, seeds=sd, y_transforms=yy, noise_pred=npred)


def test_mixture_distribution(pkg, engine):
    """R = 4096 draws of one 3-particle series, m = 3: sample mean and covariance within 5 standard errors of the mixture's moments
    (agp_mixture_moments of the returned components).  The draws are a function of the seed alone, so the outcome is fixed: the
    reference route — the same components and normals through tests/_pred_sample_ref.py and NumPy — passes at this seed (checked
    here before the device's samples are), and the device's samples lie within the sample bound of that route's."""
    G = pkg
    ts, xs = G.prior.synthetic_series(256, seed=31, shuffle=True)
    series, queries = [(ts[:40].copy(), xs[:40].copy())], [np.array([0.2, 0.6, 1.05])]
    nodes = [G.SquaredExponential(0.47, 0.9), G.Periodic(0.96, 0.21, 0.8) * G.Linear(0.1, 1.3, 0.7), G.Linear(0.3, 0.2, 0.5)]
    noises, w, seed, Rn = np.array([0.1, 0.2, 0.15]), np.array([0.5, 0.2, 0.3]), 2026, 4096
    r = engine.predict_sample_series_batch(series, queries, nodes, noises, [0, 0, 0], w, Rn, seeds=[seed], y_transforms=[(2.0, 0.5)],
                                           want_moments=True)
    mean, var, cov = engine.mixture_moments(np.stack(r.mean), w, covs=np.stack(r.cov))
    comp = PS.components(seed, w, Rn)
    z = PS.normals(seed, 3, range(Rn))
    assert np.array_equal(r.component[0], comp)
    cpu = np.stack([r.mean[c] + np.linalg.cholesky(r.cov[c]) @ z[:, j] for j, c in enumerate(comp)], axis=1)
    assert (np.abs(cpu - r.x[0]).max(axis=0) <= TOL_X * np.maximum(1.0, np.abs(cpu).max(axis=0))).all()
    for name, x in (("reference route", cpu), ("device", r.x[0])):
        d = x - mean[:, None]
        se_mean = np.sqrt(var / Rn)
        assert (np.abs(x.mean(axis=1) - mean) <= 5 * se_mean).all(), name
        prod = d[:, None, :] * d[None, :, :]                 # (3, 3, R): the sample covariance is the mean of these products
        se_cov = prod.std(axis=2, ddof=1) / np.sqrt(Rn)
        assert (np.abs(prod.mean(axis=2) - cov) <= 5 * se_cov).all(), name


def test_python_routes(pkg, engine, seeded):
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    lw = np.log(np.maximum(w, 1e-300))
    lw[w == 0] = -np.inf
    xs = pkg.predict_rand_series(engine, series, queries, nodes, noises, sidx, lw, Rn, seeds, y_transforms=yts)
    assert [x.shape for x in xs] == [(len(q), Rn) for q in queries]
    for s in range(3):
        assert np.array_equal(bits(xs[s]), bits(r.x[s]))     # (the softmax of log(w) over a series gives w back: dyadic weights)
    mv = pkg.predict_mvn_series(engine, series, queries, nodes, noises, sidx, lw, y_transforms=yts)
    assert len(mv) == 3
    for s, d in enumerate(mv):
        sel = np.arange(4 * s, 4 * s + 4)
        m = len(queries[s])
        mus = np.stack([r.mean[p] for p in sel]); covs = np.stack([r.cov[p] for p in sel])
        mean = w[sel] @ mus
        dev = mus - mean
        cov = np.einsum("p,pij->ij", w[sel], covs) + np.einsum("p,pi,pj->ij", w[sel], dev, dev)
        assert d.mean().shape == (m,) and d.cov().shape == (m, m) and d.var().shape == (m,)
        assert np.abs(d.mean() - mean).max() <= 1e-12 * max(1.0, np.abs(mean).max())
        assert np.linalg.norm(d.cov() - cov) <= 1e-12 * np.linalg.norm(cov)
        assert np.abs(d.var() - np.diag(cov)).max() <= 1e-12 * np.abs(cov).max()
        assert np.array_equal(bits(d.rand(Rn, seed=int(seeds[s]))), bits(r.x[s]))
        y = r.x[s][:, 0]
        assert np.isfinite(d.logpdf(y))
        q, ok = d.quantile(0.5)
        assert q.shape == (m,) and ok
    # built from moments alone there is no series behind the object: the base class's refusal, not an AttributeError
    bare = pkg.SeriesMixtureModel.from_components(mv[0]._components, mv[0].probs, engine=engine)
    assert np.array_equal(bits(bare.mean()), bits(mv[0].mean()))
    for call in (lambda: bare.rand(2), lambda: bare.logpdf(r.x[0][:, 0]), lambda: bare.quantile(0.5)):
        with pytest.raises(NotImplementedError):
            call()


def raw_call(pkg, engine, a, R_, Rp, fill):
    """agp_predict_sample_series_batch itself on the arguments a (a dict), outputs sized for Rp samples per series and pre-filled
    with `fill`: (rc, message, {name: flat output})"""
    E = sys.modules[pkg.__name__ + ".engine"]
    packed = pkg.series_call_args(a["series"], a["nodes"], a["noises"], a["sidx"])
    qpack = pkg.pack_queries(a["queries"], len(a["series"]), None, len(a["nodes"]))
    S, P = len(a["series"]), len(a["nodes"])
    m_p = [len(a["queries"][s]) for s in a["sidx"]]
    o = {"x": np.full(Rp * int(qpack[0][-1]) + 1, float(fill)), "component": np.full(S * Rp + 1, fill, dtype=np.int32),
         "mean": np.full(sum(m_p) + 1, float(fill)), "cov": np.full(sum(k * k for k in m_p) + 1, float(fill)),
         "info": np.full(P, fill, dtype=np.int32), "out_off": np.full(P + 1, fill, dtype=np.int64),
         "cov_off": np.full(P + 1, fill, dtype=np.int64)}
    yt = np.asarray(a["yts"], dtype=np.float64)
    sl, ic = np.ascontiguousarray(yt[:, 0]), np.ascontiguousarray(yt[:, 1])
    i64 = C.POINTER(C.c_int64)
    zz = None if a["z"] is None else np.ascontiguousarray(a["z"], dtype=np.float64)
    cc = None if a["component"] is None else np.ascontiguousarray(a["component"], dtype=np.int32)
    sd = np.ascontiguousarray(a["seeds"], dtype=np.uint64)
    ww = np.ascontiguousarray(a["w"], dtype=np.float64)
    rc = engine._lib.agp_predict_sample_series_batch(
        engine._ctx, *E._series_ctypes(packed, qpack), E._dp(sl), E._dp(ic), E._dp(ww), R_, sd.ctypes.data_as(C.POINTER(C.c_uint64)),
        E._ip(cc), E._dp(zz), E._dp(o["x"]), E._ip(o["component"]), E._dp(o["mean"]), o["out_off"].ctypes.data_as(i64), E._dp(o["cov"]),
        o["cov_off"].ctypes.data_as(i64), E._ip(o["info"]))
    return rc, engine._lib.agp_last_error(engine._ctx).decode(), o


def test_flat_layout(pkg, engine, seeded):
    """the C entry's own flat outputs, particles interleaved across the series: out_off, cov_off and the places of every sample,
    mean and covariance are tests/_series_sample_ref.layout's; one element past each output stays untouched"""
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    perm = np.array([0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11])
    a = dict(series=series, queries=queries, nodes=[nodes[p] for p in perm], noises=noises[perm], sidx=sidx[perm], w=w[perm],
             seeds=seeds, yts=yts, component=None, z=None)
    rc, msg, o = raw_call(pkg, engine, a, Rn, Rn, -7)
    assert rc == 0, msg
    m_s = [len(q) for q in queries]
    x_off, out_off, cov_off = R.layout(m_s, sidx[perm], Rn)
    assert np.array_equal(o["out_off"], out_off) and np.array_equal(o["cov_off"], cov_off) and (o["info"] == 0).all()
    for s in range(3):
        for j in range(Rn):
            at = x_off[s] + j * m_s[s]
            assert np.array_equal(bits(o["x"][at:at + m_s[s]]), bits(np.ascontiguousarray(r.x[s][:, j])))
        assert np.array_equal(perm[o["component"][s * Rn:(s + 1) * Rn]], r.component[s])
    for k, p in enumerate(perm):
        assert np.array_equal(bits(o["mean"][out_off[k]:out_off[k + 1]]), bits(r.mean[p]))
        assert np.array_equal(bits(o["cov"][cov_off[k]:cov_off[k + 1]]), bits(np.ascontiguousarray(r.cov[p]).ravel()))   # (symmetric)
    assert o["x"][x_off[-1]] == -7 and o["mean"][out_off[-1]] == -7 and o["cov"][cov_off[-1]] == -7 and o["component"][3 * Rn] == -7


def test_argument_errors(pkg, engine, seeded):
    (series, queries, nodes, noises, sidx, yts), ref, w, seeds, Rn, r = seeded
    m_s = [len(q) for q in queries]
    Q = sum(m_s)

    def attempt(match, R_=4, **kw):
        a = dict(series=series, queries=queries, nodes=nodes, noises=noises, sidx=sidx, w=w, seeds=seeds, yts=yts, component=None, z=None)
        a.update(kw)
        # (the sentinels are sized for the valid calls' four samples, whatever R_ is: a rejected call writes nothing)
        rc, msg, o = raw_call(pkg, engine, a, R_, 4, -7)
        assert rc != 0 and match in msg, (match, rc, msg)
        for name, out in o.items():                                            # nothing is written
            assert (out == -7).all(), (match, name)
        return msg

    attempt("negative number of samples", R_=-1)
    attempt("too large", R_=2 ** 31 // Q + 1, component=np.zeros(1, dtype=np.int32), z=np.zeros(1))
    c_ok = np.repeat(np.array([[0], [4], [8]], dtype=np.int32), 4, axis=1)
    c = c_ok.copy(); c[1, 2] = 3
    assert "series 1" in attempt("is not a particle of the series", component=c)
    c = c_ok.copy(); c[2, 0] = 9
    assert "series 2" in attempt("has weight 0", component=c)
    z = np.zeros(4 * Q); z[4 * m_s[0] + 5] = np.inf
    assert "series 1" in attempt("is not finite", z=z)
    y = np.array(yts); y[1, 1] = np.nan
    assert "series 1" in attempt("finite intercept", yts=y)
    y = np.array(yts); y[2, 0] = 0.0
    assert "series 2" in attempt("non-zero slope", yts=y)
    wb = w.copy(); wb[4] = 0.6
    assert "series 1" in attempt("sum to 1", w=wb)
    # a series without particles
    assert "series 3" in attempt("no particles", series=list(series) + [series[0]], queries=list(queries) + [np.zeros(0)],
                                 seeds=np.arange(4), yts=np.vstack([yts, [(1.0, 0.0)]]))
    # the cap on the joint points: 144 training points + 36 queries
    ts, xs = pkg.prior.synthetic_series(256, seed=1, shuffle=True)
    msg = attempt("more than AGP_SERIES_MAX_N", series=[series[0], (ts[:144], xs[:144]), series[2]],
                  queries=[queries[0], np.linspace(1.0, 1.2, 36), queries[2]])
    assert "series 1" in msg and "144" in msg and "36" in msg
