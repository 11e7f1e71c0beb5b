"""GPU tests of agp_predict_quantile_series_batch (forecast bands of many short series in one call: agp_predict_series_batch, then the
ragged pack / search / moments kernels of csrc/agp_series_quantile_kernel.hpp on the same stream).
Bitwise: per series, x / converged / iters equal mixture_quantile(raw_components(predict_series_batch(...))) on the series' stacked
block, mean / var equal mixture_moments(..., space=0) on it, logpdf / info equal predict_series_batch's — every series, every point.
Against the oracle (independent of the engine's search): |F_oracle(x) - q| < tol + 1e-7 by mpmath at every point (check_fused's
criterion in tests/test_gpu_predict_quantile.py; 1e-7 is the project's allowance for the predictive's own error), and the moments
within 1e-8 max(1, max|ref|) per series of tests/_mixture_moments_ref.py on the oracle's components (_series_predict_ref.close, the
family's tolerance)."""
import ctypes as C

import numpy as np
import pytest

import _mixture_moments_ref as MM
import _mixture_quantile_ref as MQ
import _series_cases as SC
import _series_predict_ref as P
import _series_quantile_ref as R
import test_gpu_series as TS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
bits = TS.bits
TOLS = (1e-5, 1e-10)


def sbits(band, s):
    """every output of series s as one int64 vector: x, converged, iters, mean, var"""
    parts = [bits(band.x[s]).ravel(), band.converged[s].astype(np.int64).ravel(), band.iters[s].astype(np.int64).ravel()]
    if band.mean is not None:
        parts += [bits(band.mean[s]), bits(band.var[s])]
    return np.concatenate(parts)


def call(engine, c, tol=1e-5, q=None, **kw):
    kw.setdefault("want_moments", True); kw.setdefault("want_logpdf", True); kw.setdefault("check", False)
    return engine.predict_quantile_series_batch(c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"], c["weights"],
                                                c["q"] if q is None else q, y_transforms=c["yt"], tol=tol, **kw)


def subcase(c, keep):
    """the case restricted to the series `keep`, in that order"""
    keep = list(keep)
    sel = np.concatenate([np.flatnonzero(c["sidx"] == s) for s in keep]) if keep else np.zeros(0, dtype=np.int64)
    new = {s: k for k, s in enumerate(keep)}
    return dict(series=[c["series"][s] for s in keep], queries=[c["queries"][s] for s in keep], nodes=[c["nodes"][i] for i in sel],
                noises=c["noises"][sel], sidx=np.array([new[int(c["sidx"][i])] for i in sel], dtype=np.int32),
                weights=c["weights"][sel], yt=c["yt"][keep], q=c["q"])


def check_two_step(pkg, engine, c, name):
    """the new call against predict_series_batch -> raw_components -> mixture_quantile / mixture_moments, series by series"""
    S = len(c["series"])
    means, vars_, lp, info = engine.predict_series_batch(c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"],
                                                         want_logpdf=True, check=False)
    assert (info == 0).all(), (name, info)
    bands = {tol: call(engine, c, tol) for tol in TOLS}
    n_pts = 0
    for s in range(S):
        sel = np.flatnonzero(c["sidx"] == s)
        assert len(sel) > 0
        bm, bv = np.stack([means[i] for i in sel]), np.stack([vars_[i] for i in sel])
        mr, vr, inf = pkg.raw_components(bm, bv, info[sel], len(c["series"][s][0]), tuple(c["yt"][s]))
        assert (inf == 0).all()
        w = c["weights"][sel]
        for tol in TOLS:
            b = bands[tol]
            x, conv, it = engine.mixture_quantile(mr, vr, w, c["q"], tol=tol)
            assert b.x[s].shape == x.shape == (len(c["queries"][s]), len(c["q"])), (name, s)
            assert np.array_equal(bits(b.x[s]), bits(x)), (name, s, tol)
            assert np.array_equal(b.converged[s], conv) and np.array_equal(b.iters[s], it), (name, s, tol)
            assert conv.all(), (name, s, tol)
        mean, var, _ = engine.mixture_moments(mr, w, vars=vr, space=0)
        for b in bands.values():
            assert np.array_equal(bits(b.mean[s]), bits(mean)) and np.array_equal(bits(b.var[s]), bits(var)), (name, s)
        n_pts += x.size
    for b in bands.values():
        assert np.array_equal(bits(b.logpdf), bits(lp)) and np.array_equal(b.info, info), name
    print(f"[series-quantile] {name}: {S} series, {n_pts} (query, quantile) points bitwise equal to the two-step route at tol {TOLS}")


@pytest.fixture(scope="module")
def band(engine):
    c = R.band_case()
    res = call(engine, c)
    return c, res


def test_bitwise_band_case(pkg, engine):
    c = R.band_case()
    check_two_step(pkg, engine, c, "band")
    b = call(engine, c)
    assert b.x[1].shape == (0, 3) and b.mean[1].shape == (0,) and b.converged[1].shape == (0, 3)      # the series without queries


def test_bitwise_band_case_shuffled_particles(pkg, engine, band):
    c, res = band
    perm = np.random.default_rng(11).permutation(len(c["nodes"]))
    assert (np.diff(np.flatnonzero(c["sidx"][perm] == 8)) > 1).any()      # a series' particles are interleaved with other series'
    cs = dict(c, nodes=[c["nodes"][i] for i in perm], noises=c["noises"][perm], sidx=c["sidx"][perm], weights=c["weights"][perm])
    check_two_step(pkg, engine, cs, "band, shuffled particles")


def wide_case(pkg):
    """three 17-point series, five queries each, 1, 65 and 130 particles: the lane stride and the padding boundaries"""
    rng = np.random.default_rng(20261019)
    series, queries, nodes, noises, sidx, weights = [], [], [], [], [], []
    for s, Ps in enumerate((1, 65, 130)):
        ts, xs = pkg.prior.synthetic_series(256, seed=400 + s, shuffle=True)
        series.append((ts[:17].copy(), xs[:17].copy()))
        queries.append(P.queries_for(ts, ts[:17], 5))
        nd, nz = pkg.prior.sample_particles(rng, Ps, max_depth=3)
        w = rng.random(Ps)
        if Ps > 2:
            w[[0, Ps // 2]] = 0.0
        nodes += nd; noises += list(nz); sidx += [s] * Ps; weights += list(w / w.sum())
    return dict(series=series, queries=queries, nodes=nodes, noises=np.array(noises), sidx=np.array(sidx, dtype=np.int32),
                weights=np.array(weights), yt=np.array([[1.7, -0.3], [0.25, 3.0], [-2.0, 0.5]]), q=np.array(R.QS))


def test_bitwise_wide_case(pkg, engine):
    check_two_step(pkg, engine, wide_case(pkg), "wide")


def test_against_oracle(engine, band):
    c, res = band
    tol = 1e-5
    assert (res.info == 0).all()
    worst = worst_m = worst_v = 0.0
    for s in range(len(c["series"])):
        w = c["weights"][c["sidx"] == s]
        assert res.converged[s].all(), s
        M, Sd = MQ.components(c["raw_mean"][s], c["raw_var"][s])
        for i in range(len(c["queries"][s])):
            for k, qk in enumerate(c["q"]):
                F = MQ.mp_cdf(res.x[s][i, k], M[i], Sd[i], w)
                worst = max(worst, float(abs(F - qk)))
                assert abs(F - qk) < tol + 1e-7, (s, i, k, float(F), qk)
        ref = MM.moments(c["raw_mean"][s], w, vars=c["raw_var"][s], space=0)
        assert P.close(res.mean[s], ref["mean"]) and P.close(res.var[s], ref["var"]), s
        if ref["mean"].size:
            worst_m = max(worst_m, np.abs(res.mean[s] - ref["mean"]).max() / max(1.0, np.abs(ref["mean"]).max()))
            worst_v = max(worst_v, np.abs(res.var[s] - ref["var"]).max() / max(1.0, np.abs(ref["var"]).max()))
    print(f"[series-quantile] oracle: worst |F(x) - q| {worst:.3e} (bound {tol + 1e-7:.3e}); moments |d| / max(1, max|ref|): mean "
          f"{worst_m:.3e}, variance {worst_v:.3e} (bound 1e-8)")


def test_batch_independence_bitwise(pkg, engine, band, monkeypatch):
    c, res = band
    S = len(c["series"])
    for s in range(S):                                           # each series alone
        one = call(engine, subcase(c, [s]))
        assert np.array_equal(sbits(one, 0), sbits(res, s)), s
        assert np.array_equal(bits(one.logpdf), bits(res.logpdf[c["sidx"] == s]))
    order = np.random.default_rng(5).permutation(S)              # the series list permuted
    pr = call(engine, subcase(c, order))
    for k, s in enumerate(order):
        assert np.array_equal(sbits(pr, k), sbits(res, s)), s
    for k, qk in enumerate(c["q"]):                              # nq = 1 against column k of nq = 3
        one = call(engine, c, q=float(qk))
        for s in range(S):
            assert one.x[s].shape == (len(c["queries"][s]),)
            assert np.array_equal(bits(one.x[s]), bits(res.x[s][:, k])) and np.array_equal(one.iters[s], res.iters[s][:, k])
            assert np.array_equal(one.converged[s], res.converged[s][:, k])
            assert np.array_equal(bits(one.mean[s]), bits(res.mean[s])) and np.array_equal(bits(one.var[s]), bits(res.var[s]))
    again = call(engine, c)                                      # a second call
    for s in range(S):
        assert np.array_equal(sbits(again, s), sbits(res, s))
    mom = call(engine, c, q=[])                                  # nq = 0: the moments alone
    for s in range(S):
        assert mom.x[s].shape == (len(c["queries"][s]), 0)
        assert np.array_equal(bits(mom.mean[s]), bits(res.mean[s])) and np.array_equal(bits(mom.var[s]), bits(res.var[s]))
    for poison in ("0", "1"):                                    # a poisoned engine (tests/test_gpu_predict_quantile.py builds it so)
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = call(e, c)
            for s in range(S):
                assert np.array_equal(sbits(got, s), sbits(res, s)), (poison, s)
            assert np.array_equal(bits(got.logpdf), bits(res.logpdf)) and np.array_equal(got.info, res.info)
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()


def test_particle_without_predictive(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(40, seed=2)
    q = np.linspace(1.0, 1.5, 19)
    bad = G.Constant(1.0)
    good, good2 = G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.3, 0.9) + G.Linear(0.2, 0.3, 0.4)
    first = SC.first_bad_minor(O.compute_cov_matrix_vectorized(bad.to_tuple(), -0.5, ts))
    assert first == 2
    # series 0: two good particles; series 1: a particle with a non-positive pivot between two good ones; series 2: one good particle;
    # series 3: queries but no particle
    series = [(ts, xs), (ts[:30], xs[:30]), (ts[:17], xs[:17]), (ts[:5], xs[:5])]
    queries = [q, q[:7], q[:3], q[:4]]
    nodes = [good, good2, good, bad, good2, good2]
    noises = np.array([0.1, 0.2, 0.1, -0.5, 0.2, 0.2])
    sidx = np.array([0, 0, 1, 1, 1, 2], dtype=np.int32)
    yt = np.array([[1.7, -0.3], [0.5, 0.1], [1.0, 0.0], [2.0, 1.0]])
    for w_bad in (0.25, 0.0):                                    # the series is undefined whatever the bad particle's weight
        w = np.array([0.5, 0.5, 0.5, w_bad, 0.5 - w_bad, 1.0])
        c = dict(series=series, queries=queries, nodes=nodes, noises=noises, sidx=sidx, weights=w, yt=yt, q=np.array(R.QS))
        res = call(engine, c)
        _, _, lp, info = engine.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, check=False)
        assert info.tolist() == [0, 0, 0, first, 0, 0] and np.array_equal(res.info, info)
        assert np.array_equal(bits(res.logpdf), bits(lp))
        for s in (1, 3):
            assert res.x[s].shape == (len(queries[s]), 3) and np.isnan(res.x[s]).all(), s
            assert not res.converged[s].any() and (res.iters[s] == 0).all(), s
            assert np.isnan(res.mean[s]).all() and np.isnan(res.var[s]).all(), s
        for s in (0, 2):                                         # every other series: the bits of a call without the bad series
            alone = call(engine, subcase(c, [s]))
            assert alone.converged[0].all() and np.array_equal(sbits(alone, 0), sbits(res, s)), s
        with pytest.raises(G.PosDefException) as ei:
            call(engine, c, check=True)
        assert ei.value.particle == 3 and ei.value.info == first
    # raw_components' rule: a predictive that exists (info 0) with a negative raw variance reports n_s + i + 1 for the first such query
    npred = np.array([0.1, 0.2, 0.1, 0.2, 0.2, 0.2])
    c = dict(series=series, queries=queries, nodes=[good, good2, good, good2, good2, good2], noises=np.abs(noises), sidx=sidx,
             weights=np.array([0.5, 0.5, 0.5, 0.25, 0.25, 1.0]), yt=yt, q=np.array(R.QS))
    means, vars_, info = engine.predict_series_batch(c["series"], queries, c["nodes"], c["noises"], sidx, noise_pred=npred, check=False)
    assert (info == 0).all()
    npred[4] = 0.2 - np.sort(vars_[4])[1]                        # particle 4 (series 1): its smallest variance pushed below 0
    means, vars_, info = engine.predict_series_batch(c["series"], queries, c["nodes"], c["noises"], sidx, noise_pred=npred, check=False)
    want = [pkg.raw_components(np.stack([means[i]]), np.stack([vars_[i]]), info[i:i + 1], len(series[sidx[i]][0]), tuple(yt[sidx[i]]))[2][0]
            for i in range(6)]
    assert want[4] > 30 and [w_ for i, w_ in enumerate(want) if i != 4] == [0] * 5
    res = call(engine, c, noise_pred=npred)
    assert res.info.tolist() == want
    assert np.isnan(res.x[1]).all() and not res.converged[1].any() and np.isnan(res.mean[1]).all()
    assert res.converged[0].all() and res.converged[2].all()
    with pytest.raises(G.PosDefException) as ei:
        call(engine, c, noise_pred=npred, check=True)
    assert ei.value.particle == 4 and ei.value.info == want[4]
    # no particle at all: every series is a series without particles
    none = engine.predict_quantile_series_batch(series, queries, [], np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0), R.QS,
                                                want_moments=True, want_logpdf=True)
    assert none.info.size == 0 and none.logpdf.size == 0
    for s in range(4):
        assert none.x[s].shape == (len(queries[s]), 3) and np.isnan(none.x[s]).all() and not none.converged[s].any()
        assert (none.iters[s] == 0).all() and np.isnan(none.mean[s]).all() and np.isnan(none.var[s]).all()


def test_stateless(pkg, band):
    c, res = band
    S = len(c["series"])
    eng = pkg.GPEngine(0)
    try:
        r0 = call(eng, c)                                        # a fresh engine on which set_data was never called
        assert all(np.array_equal(sbits(r0, s), sbits(res, s)) for s in range(S))
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        tq = np.linspace(1.0, 1.2, 7)
        pred0 = eng.predict_batch(rn, rz, tq, check=False)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max,
                    eng.predict_reuse_stats())
        before = snapshot()
        r1 = call(eng, c)
        assert all(np.array_equal(sbits(r1, s), sbits(res, s)) for s in range(S))
        assert snapshot() == before
        pred1 = eng.predict_batch(rn, rz, tq, check=False)
        assert np.array_equal(bits(pred1[0]), bits(pred0[0])) and np.array_equal(bits(pred1[1]), bits(pred0[1]))
    finally:
        eng.close()


SENTINEL = 7.25


def raw_call(engine, pkg, c, null=(), q_off=None, q=None, weights=None, yt=None):
    """the C entry itself on sentinel-filled outputs: (rc, msg, x, conv, iters, mean, var, logpdf, info)"""
    op_off, ops, prm_off, prm = c["programs"] if "programs" in c else pkg.encode_batch(c["nodes"])
    series, queries = c["series"], c["queries"]
    P = len(c["noises"]); S = len(series)
    pt_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(t) for t, _ in series])]), dtype=np.int64)
    if q_off is None:
        q_off = np.concatenate([[0], np.cumsum([len(v) for v in queries])])
    q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    sidx = np.ascontiguousarray(c["sidx"], dtype=np.int32)
    ts = np.ascontiguousarray(np.concatenate([t for t, _ in series] + [np.zeros(1)]))
    xs = np.ascontiguousarray(np.concatenate([x for _, x in series] + [np.zeros(1)]))
    tq = np.ascontiguousarray(np.concatenate(list(queries) + [np.zeros(1)]))
    noises = np.ascontiguousarray(c["noises"], dtype=np.float64)
    w = np.ascontiguousarray(c["weights"] if weights is None else weights, dtype=np.float64)
    yt = np.asarray(c["yt"] if yt is None else yt, dtype=np.float64)
    slope, icpt = np.ascontiguousarray(yt[:, 0]), np.ascontiguousarray(yt[:, 1])
    qa = np.ascontiguousarray(c["q"] if q is None else q, dtype=np.float64)
    nq = len(qa); Q = sum(len(v) for v in queries)
    x = np.full(nq * Q + 16, SENTINEL); mean = np.full(Q + 16, SENTINEL); var = np.full(Q + 16, SENTINEL); lp = np.full(P + 1, SENTINEL)
    conv = np.full(nq * Q + 16, 7, dtype=np.int32); iters = np.full(nq * Q + 16, 7, dtype=np.int32); info = np.full(P + 1, 7, dtype=np.int32)
    dp, ip, lp_ = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    arg = lambda name, a, t: None if name in null else a.ctypes.data_as(t)
    rc = engine._lib.agp_predict_quantile_series_batch(
        engine._ctx, S, pt_off.ctypes.data_as(lp_), ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), arg("q_off", q_off, lp_),
        arg("ts_pred", tq, dp), P, sidx.ctypes.data_as(ip), op_off.ctypes.data_as(ip), ops.ctypes.data_as(C.POINTER(C.c_uint8)),
        prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp), None, arg("weights", w, dp), slope.ctypes.data_as(dp),
        icpt.ctypes.data_as(dp), arg("q", qa, dp), nq, 1e-5, 10**6, arg("out_x", x, dp), conv.ctypes.data_as(ip), iters.ctypes.data_as(ip),
        mean.ctypes.data_as(dp), var.ctypes.data_as(dp), lp.ctypes.data_as(dp), info.ctypes.data_as(ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), x, conv, iters, mean, var, lp, info


def test_argument_errors_leave_outputs_untouched(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(G.SERIES_MAX_N + 1, seed=4)
    q = np.linspace(1.0, 1.3, 9)
    good = G.SquaredExponential(0.3, 0.8)
    c = dict(series=[(ts[:20], xs[:20]), (ts[:9], xs[:9])], queries=[q, q[:4]], nodes=[good, good, good], noises=np.array([0.1, 0.2, 0.1]),
             sidx=np.array([0, 0, 1], dtype=np.int32), weights=np.array([0.25, 0.75, 1.0]), yt=np.array([[1.0, 0.0], [2.0, 0.5]]),
             q=np.array(R.QS))

    def untouched(out):
        rc, msg, x, conv, iters, mean, var, lp, info = out
        return ((x == SENTINEL).all() and (mean == SENTINEL).all() and (var == SENTINEL).all() and (lp == SENTINEL).all()
                and (conv == 7).all() and (iters == 7).all() and (info == 7).all())

    def valid():
        out = raw_call(engine, pkg, c)
        ref = call(engine, c)
        assert out[0] == 0 and (out[8][:3] == 0).all()
        assert np.array_equal(bits(out[2][:27]), bits(ref.x[0].T.ravel())) and np.array_equal(bits(out[2][27:39]), bits(ref.x[1].T.ravel()))
        assert (out[2][39:] == SENTINEL).all() and (out[5][13:] == SENTINEL).all() and (out[3][39:] == 7).all()      # nothing behind the last block
        assert np.array_equal(bits(out[5][:13]), bits(np.concatenate(ref.mean)))

    valid()
    out = raw_call(engine, pkg, c, weights=[0.25, 0.75, 0.9])                         # the weights of series 1 sum to 0.9
    assert out[0] == -1 and "series 1" in out[1] and "sum to 1" in out[1] and untouched(out)
    out = raw_call(engine, pkg, c, weights=[1.25, -0.25, 1.0])                        # a negative weight
    assert out[0] == -1 and "series 0" in out[1] and ">= 0" in out[1] and untouched(out)
    for qq in ([0.5, 1.0], [0.0], [np.nan], [-0.1, 0.5]):                             # q outside (0, 1)
        out = raw_call(engine, pkg, c, q=qq)
        assert out[0] == -1 and "(0, 1)" in out[1] and untouched(out), qq
    out = raw_call(engine, pkg, c, yt=[[1.0, 0.0], [0.0, 0.5]])                       # a zero slope
    assert out[0] == -1 and "series 1" in out[1] and "slope" in out[1] and untouched(out)
    out = raw_call(engine, pkg, c, null=("out_x",))                                   # a null out_x with nq > 0
    assert out[0] == -1 and "out_x" in out[1] and untouched(out)
    out = raw_call(engine, pkg, c, null=("weights",))
    assert out[0] == -1 and "weights" in out[1] and untouched(out)
    valid()
    # agp_predict_series_batch's own errors, with its messages: a decreasing q_off, a series longer than the cap, a null ts_pred
    out = raw_call(engine, pkg, c, q_off=[0, 9, 5])
    assert out[0] == -1 and "series 1" in out[1] and "q_off decreases" in out[1] and untouched(out)
    long_case = dict(c, series=[(ts[:20], xs[:20]), (ts, xs)])
    out = raw_call(engine, pkg, long_case)
    assert out[0] == -1 and "series 1" in out[1] and str(G.SERIES_MAX_N + 1) in out[1] and untouched(out)
    out = raw_call(engine, pkg, c, null=("ts_pred",))
    assert out[0] == -1 and "null pointer" in out[1] and untouched(out)
    with pytest.raises(G.AGPError, match=r"particle 2.*series index 5"):
        engine.predict_quantile_series_batch(c["series"], c["queries"], c["nodes"], c["noises"], [0, 0, 5], c["weights"], c["q"])
    with pytest.raises(ValueError):
        engine.predict_quantile_series_batch(c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"], c["weights"][:2], c["q"])
    with pytest.raises(ValueError):
        engine.predict_quantile_series_batch(c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"], c["weights"], c["q"],
                                             y_transforms=[(1.0, 0.0)])
    valid()


def test_module_level_predict_quantile_series(pkg, engine, band):
    c, res = band
    rng = np.random.default_rng(12)
    lw = 2.0 * rng.standard_normal(len(c["nodes"]))
    _, w = pkg.pack_series_mixture(c["sidx"], len(c["series"]), log_weights=lw)
    ref = engine.predict_quantile_series_batch(c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"], w, c["q"],
                                               y_transforms=c["yt"], tol=1e-6)
    out = pkg.predict_quantile_series(engine, c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"], lw, c["q"],
                                      y_transforms=c["yt"], tol=1e-6)
    assert len(out) == len(c["series"])
    for s, (x, ok) in enumerate(out):
        assert np.array_equal(bits(x), bits(ref.x[s])) and ok.shape == (3,)
        assert np.array_equal(ok, ref.converged[s].all(axis=0)) and ok.all()
        if x.size:
            assert (x[:, 0] < x[:, 1]).all() and (x[:, 1] < x[:, 2]).all()
    one = pkg.predict_quantile_series(engine, c["series"], c["queries"], c["nodes"], c["noises"], c["sidx"], lw, 0.5, y_transforms=c["yt"],
                                      tol=1e-6)
    for s, (x, ok) in enumerate(one):
        assert isinstance(ok, bool) and ok and np.array_equal(bits(x), bits(ref.x[s][:, 1]))
