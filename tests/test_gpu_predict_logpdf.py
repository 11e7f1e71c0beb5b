"""Predictive log-density of held-out values on the GPU (agp_predict_logpdf_batch; src/api.jl:686-699 predict_proba,
test/experiment_hmc.jl:125) against the reference restatement of tests/_pred_logpdf_ref.py: |lp - ref| <= 1e-8 S per particle,
S the sum of the magnitudes of the terms the log-density is made of; up to n + m = 300 an mpmath / 80-bit arbiter decides misses."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _pred_logpdf_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-8
NS = [0, 1, 2, 127, 128, 129, 257, 1000]
MS = [0, 1, 17, 127, 128, 129, 300]
QUERY_KINDS = ("future", "interleaved", "training", "shuffled")


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
    tp = 1.0 + 0.3 * np.arange(1, m + 1) / max(m, 1)
    if kind == "shuffled":
        tp = np.concatenate([rng.random(m // 2), tp[: m - m // 2]]); rng.shuffle(tp)
    return tp


def check_batch(lp, info, nodes, noises, ts, xs, tp, y, npred=None, mt=None, mp_=None, ctx=None, sub=None):
    for p in (range(len(nodes)) if sub is None else sub):
        assert info[p] == 0, (ctx, p, info[p])
        npp = None if npred is None else float(np.broadcast_to(npred, (len(nodes),))[p])
        R.assert_close(float(lp[p]), nodes[p].to_tuple(), float(noises[p]), ts, xs, tp, y, tol=TOL, ctx=(ctx, p),
                       noise_pred=npp, mean_train=mt, mean_pred=mp_)


def test_shapes_query_sets_fixture_kernels(pkg, engine):
    G = pkg
    nodes = fixture_kernels(G)
    P = len(nodes)
    noises = np.full(P, 0.2)
    rng = np.random.default_rng(11)
    ts_all = np.sort(rng.random(max(NS))); xs_all = 0.5 * rng.standard_normal(max(NS))
    engine.set_data(ts_all, xs_all)
    c = 0
    for n in NS:
        ts, xs = ts_all[:n], xs_all[:n]
        for m in MS:
            for kind in QUERY_KINDS:
                c += 1
                tp = queries(kind, ts, n, m, rng)
                y = 0.5 * rng.standard_normal(m)
                npred = [None, 0.3 * noises, 0.05 + 0.1 * rng.random(P)][c % 3]
                lp, info = engine.predict_logpdf_batch(nodes, noises, tp, y, n=n, noise_pred=npred)
                if m == 0:
                    assert (lp == 0.0).all() and (info == 0).all()
                    continue
                check_batch(lp, info, nodes, noises, ts, xs, tp, y, npred=npred, ctx=(n, m, kind))


def test_prior_populations_and_mean_functions(pkg, engine):
    rng = np.random.default_rng(5)
    ts, xs = pkg.prior.synthetic_series(1000, seed=3, shuffle=True)
    engine.set_data(ts, xs)
    for depth, n, m in ((3, 257, 129), (6, 1000, 129), (6, 129, 300)):
        nodes, noises = pkg.prior.sample_particles(rng, 24, max_depth=depth, min_depth=min(depth, 3))
        assert any("ChangePoint" in repr(k) for k in nodes)
        tp = np.concatenate([ts[: m // 3], 1.0 + 0.01 * np.arange(m - m // 3)])
        y = 0.4 * rng.standard_normal(m)
        for npred, mean in ((None, False), (0.3 * noises, True), (0.02 + 0.1 * rng.random(24), True)):
            mt = 0.2 * ts[:n] - 0.1 if mean else None
            mp_ = 0.2 * tp - 0.1 if mean else None
            lp, info = engine.predict_logpdf_batch(nodes, noises, tp, y, n=n, noise_pred=npred, mean_train=mt, mean_pred=mp_, check=False)
            ok = [p for p in range(24) if info[p] == 0]
            assert len(ok) >= 20
            check_batch(lp, info, nodes, noises, ts[:n], xs[:n], tp, y, npred=npred, mt=mt, mp_=mp_, ctx=(depth, n, m), sub=ok)


def test_large_case(pkg, engine):
    rng = np.random.default_rng(9)
    ts, xs = pkg.prior.synthetic_series(4096, seed=8)
    n = m = 2048
    engine.set_data(ts[:n], xs[:n])
    nodes, noises = pkg.prior.sample_particles(rng, 64, max_depth=4)
    tp, y = ts[n:], xs[n:]
    lp, info = engine.predict_logpdf_batch(nodes, noises, tp, y, check=False)
    ok = [p for p in range(64) if info[p] == 0]
    assert len(ok) >= 56
    sub = sorted(ok, key=lambda p: -noises[p])[:4]          # (no arbiter at this size: the fp64 reference's best-conditioned cases)
    check_batch(lp, info, nodes, noises, ts[:n], xs[:n], tp, y, ctx="2048", sub=sub)


def lag_pred_passes(eng):
    k = C.c_int64()
    eng._check(eng._lib.agp_get_lag_predict_stats(eng._ctx, C.byref(k)))
    return k.value


def test_lattice_and_general_paths_agree(pkg, engine, monkeypatch):
    """Queries on the series' lattice take the rank-table evaluators; the same points with rank tables off (AGP_LAG_RANK=0) and with
    every regular-grid path off (AGP_LAG=0) give the same log-density to the tolerance; off-lattice queries match the reference too."""
    rng = np.random.default_rng(4)
    n, m = 300, 140
    h = 1.0 / 511
    ts = np.arange(n) * h; xs = 0.5 * rng.standard_normal(n)
    nodes, noises = pkg.prior.sample_particles(rng, 32, max_depth=3)
    nodes += fixture_kernels(pkg); noises = np.concatenate([noises, np.full(10, 0.2)])
    tp = np.concatenate([ts[rng.integers(0, n, 40)], (n + np.arange(m - 40)) * h]); rng.shuffle(tp)
    y = 0.4 * rng.standard_normal(m)
    engine.set_data(ts, xs)
    k0 = lag_pred_passes(engine)
    lp, info = engine.predict_logpdf_batch(nodes, noises, tp, y, check=False)
    assert lag_pred_passes(engine) == k0 + 1, "lattice queries should take the rank-table path"
    tp_off = tp + 0.37 * h
    lp_off, i_off = engine.predict_logpdf_batch(nodes, noises, tp_off, y, check=False)
    assert lag_pred_passes(engine) == k0 + 1
    others = []
    for env in ({"AGP_LAG_RANK": "0"}, {"AGP_LAG": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = pkg.GPEngine(0)
        for k in env:
            monkeypatch.delenv(k)
        try:
            e.set_data(ts, xs)
            others.append(e.predict_logpdf_batch(nodes, noises, tp, y, check=False))
            assert lag_pred_passes(e) == 0
        finally:
            e.close()
    ok = [p for p in range(len(nodes)) if info[p] == 0]
    assert len(ok) >= len(nodes) - 2
    for lo, io in others:
        assert np.array_equal(io, info)
        for p in ok:
            _, S = R.reference(nodes[p].to_tuple(), float(noises[p]), ts, xs, tp, y)
            assert abs(lp[p] - lo[p]) <= TOL * S, p
    check_batch(lp, info, nodes, noises, ts, xs, tp, y, ctx="lattice", sub=ok)
    check_batch(lp_off, i_off, nodes, noises, ts, xs, tp_off, y, ctx="off-lattice", sub=[p for p in ok if i_off[p] == 0])


def test_agrees_with_value_sweep_and_host_route(pkg, engine):
    """logpdf(joint) - logpdf(prefix) from agp_logpdf (relative 1e-7), and the host route: predict_batch(want_cov=True) + an
    m x m Cholesky (what tests/test_gpu_parity.py::test_predictive_likelihood_identity_on_gpu does)."""
    G = pkg
    ts, xs = pkg.prior.synthetic_series(500, seed=77, shuffle=True)
    n_obs = 380
    for k in [G.SquaredExponential(0.2, 1.0), G.Linear(0.5) + G.Periodic(0.3, 0.25, 1.0), G.ChangePoint(G.Linear(0.5), G.Linear(1.5), 0.5, 0.001)]:
        engine.set_data(ts, xs)
        lj = engine.logpdf(k, 0.1)
        lo = engine.logpdf(k, 0.1, n=n_obs)
        lp, info = engine.predict_logpdf_batch([k], [0.1], ts[n_obs:], xs[n_obs:], n=n_obs)
        assert abs((lj - lo) - lp[0]) <= 1e-7 * max(1.0, abs(lp[0])), (k, lj - lo, lp[0])
        mean, var, cov, _ = engine.predict_batch([k], [0.1], ts[n_obs:], n=n_obs, want_cov=True)
        host = O.mvnormal_logpdf(xs[n_obs:], cov[0], mean[0])
        _, S = R.reference(k.to_tuple(), 0.1, ts[:n_obs], xs[:n_obs], ts[n_obs:], xs[n_obs:])
        assert abs(host - lp[0]) <= TOL * S
        # the public wrappers
        d = G.MvNormal(k, 0.1, ts[:n_obs], xs[:n_obs], ts[n_obs:], engine=engine)
        assert d.logpdf(xs[n_obs:]) == lp[0]


def test_predict_proba(pkg, engine):
    rng = np.random.default_rng(2)
    ts, xs = pkg.prior.synthetic_series(200, seed=1)
    a, b = 0.7, -0.2                       # scaled = a raw + b
    engine.set_data(ts[:150], xs[:150])
    nodes, noises = pkg.prior.sample_particles(rng, 6, max_depth=3)
    lw = rng.standard_normal(6)
    y_raw = (xs[150:] - b) / a
    out = pkg.predict_proba(engine, nodes, noises, lw, ts[150:], y_raw, y_transform=(a, b))
    assert list(out["particle"]) == list(range(1, 7))
    assert np.allclose(out["weight"], O.particle_weights(lw)) and abs(out["weight"].sum() - 1) < 1e-12
    for p in range(6):
        mu, cov = R.predictive(nodes[p].to_tuple(), float(noises[p]), ts[:150], xs[:150], ts[150:])
        direct = O.mvnormal_logpdf(y_raw, cov / a ** 2, (mu - b) / a)
        _, S = R.reference(nodes[p].to_tuple(), float(noises[p]), ts[:150], xs[:150], ts[150:], xs[150:])
        assert abs(out["logp"][p] - direct) <= TOL * S
    e = pkg.predict_proba(engine, nodes, noises, lw, ts[150:150], y_raw[:0], y_transform=(a, b))
    assert (e["logp"] == 0.0).all()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_bitwise_invariance(pkg, engine):
    """The result of a particle does not depend on the batch around it, the workspace chunking, copies or the caller order."""
    rng = np.random.default_rng(21)
    ts, xs = pkg.prior.synthetic_series(700, seed=5, shuffle=True)
    n, m = 520, 180
    engine.set_data(ts[:n], xs[:n])
    tp, y = ts[n:], xs[n:]
    nodes, noises = pkg.prior.sample_particles(rng, 300, max_depth=4)
    npred = 0.5 * noises
    lp, info = engine.predict_logpdf_batch(nodes, noises, tp, y, noise_pred=npred, check=False)
    for p in (0, 7, 150, 299):
        l1, i1 = engine.predict_logpdf_batch([nodes[p]], noises[p:p + 1], tp, y, noise_pred=npred[p:p + 1], check=False)
        assert same(l1, lp[p:p + 1]) and i1[0] == info[p], p
    perm = rng.permutation(300)
    lq, iq = engine.predict_logpdf_batch([nodes[i] for i in perm], noises[perm], tp, y, noise_pred=npred[perm], check=False)
    assert same(lq, lp[perm]) and np.array_equal(iq, info[perm])
    # resampled population: copies of a few survivors
    pick = rng.integers(0, 12, 200)
    d0 = engine.dedup_stats()
    lr, ir = engine.predict_logpdf_batch([nodes[i] for i in pick], noises[pick], tp, y, noise_pred=npred[pick], check=False)
    assert same(lr, lp[pick]) and np.array_equal(ir, info[pick])
    # chunked workspace: a few particles' matrices per chunk
    nt = -(-n // 128) - (-m // 128)
    engine.set_workspace_limit(3 * nt * (nt + 1) // 2 * 128 * 128 * 8)
    try:
        lc, ic = engine.predict_logpdf_batch(nodes[:40], noises[:40], tp, y, noise_pred=npred[:40], check=False)
    finally:
        engine.set_workspace_limit(0)
    assert same(lc, lp[:40]) and np.array_equal(ic, info[:40])
    assert np.isfinite(lp[info == 0]).all()
    del d0


def test_failures_are_isolated(pkg, engine):
    G = pkg
    rng = np.random.default_rng(6)
    n, m = 150, 40
    ts = np.sort(rng.random(n)); xs = 0.5 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    good = [G.SquaredExponential(0.3, 1.0), G.Periodic(0.4, 0.2, 1.0) + G.Linear(0.2), G.Constant(0.5) * G.SquaredExponential(0.1, 1.0)]
    # the first two queries share a time far from the data: for SE(0.001, 1) there K21 = 0 and, with noise_pred = 0, Sigma*'s leading
    # 2 x 2 block is [1 1; 1 1] — minor 2 vanishes exactly
    tp = np.concatenate([[5.0, 5.0], 1.0 + 0.01 * np.arange(m - 2)])
    y = 0.3 * rng.standard_normal(m)
    ref, _ = engine.predict_logpdf_batch(good, [0.1] * 3, tp, y, noise_pred=[0.05] * 3)
    # non-PD K11: a negative noise far larger than the kernel
    nodes = [good[0], G.SquaredExponential(0.3, 1.0), good[1], good[2], G.SquaredExponential(0.001, 1.0)]
    noises = np.array([0.1, -5.0, 0.1, 0.1, 0.1])
    npred = np.array([0.05, 0.05, 0.05, 0.05, 0.0])
    lp, info = engine.predict_logpdf_batch(nodes, noises, tp, y, noise_pred=npred, check=False)
    assert 1 <= info[1] <= n and math.isnan(lp[1])
    assert info[4] == n + 2 and math.isnan(lp[4])
    assert info[[0, 2, 3]].tolist() == [0, 0, 0]
    assert same(lp[[0, 2, 3]], ref)
    with pytest.raises(pkg.PosDefException):
        engine.predict_logpdf_batch(nodes, noises, tp, y, noise_pred=npred)


def test_argument_errors(pkg, engine):
    G = pkg
    engine.set_data(np.linspace(0, 1, 50), np.zeros(50))
    k = [G.SquaredExponential(0.3, 1.0)]
    lib, ctx = engine._lib, engine._ctx
    op_off, ops, prm_off, prm = G.encode_batch(k)
    tp = np.linspace(1, 2, 5); y = np.zeros(5); nz = np.array([0.1]); out = np.empty(1); info = np.zeros(1, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))       # noqa: E731
    u8 = ops.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(n, ts, yy, m):
        return lib.agp_predict_logpdf_batch(ctx, n, ts, yy, m, 1, ip(op_off), u8, ip(prm_off), dp(prm), dp(nz), None, None, None,
                                            dp(out), ip(info))
    assert call(50, dp(tp), dp(y), 5) == 0
    assert call(50, dp(tp), dp(y), -1) < 0
    assert call(51, dp(tp), dp(y), 5) < 0
    assert call(50, dp(tp), None, 5) < 0
    assert call(50, None, None, 0) == 0 and out[0] == 0.0
    with pytest.raises(pkg.AGPError):
        engine.predict_logpdf_batch(k, [0.1], tp, y, n=51)


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
        nodes, noises = pkg.prior.sample_particles(rng, 20, max_depth=4)
        nodes = nodes + [pkg.SquaredExponential(0.3, 1.0)]; noises = np.concatenate([noises, [-5.0]])      # one non-PD particle first
        for n, m in ((0, 17), (1, 1), (129, 127), (257, 129), (300, 100)):
            tp = np.concatenate([ts[n:n + m // 2], 1.0 + 0.01 * np.arange(m - m // 2)])
            y = 0.3 * rng.standard_normal(m)
            res = []
            for e in (ez, ec):
                e.set_data(ts[:max(n, 1)], xs[:max(n, 1)])
                res.append(e.predict_logpdf_batch(nodes, noises, tp, y, n=n, noise_pred=0.5 * noises + 0.1, check=False))
            (lz, iz), (lc, ic) = res
            assert same(lz, lc) and np.array_equal(iz, ic), (n, m)
            assert np.isfinite(lz[iz == 0]).all()
        assert ez.poison_stats()["bytes"] > 0
        check_batch(lc, ic, nodes, noises, ts[:300], xs[:300], tp, y, npred=0.5 * noises + 0.1, ctx="poison",
                    sub=[p for p in range(len(nodes)) if ic[p] == 0][:5])
    finally:
        ez.close(); ec.close()
