"""GPU tests of agp_predict_long_series_batch and agp_predict_quantile_long_series_batch (forecasts and bands of series of up to 512
points; k_long_series_predict, csrc/agp_long_series_kernel.hpp): parity with oracle.predict_mvn on ragged input under both routings,
every final block count, every leaf and combinator, agreement with the resident-series path, bitwise independence of the batch, the
workspace split and the other query times, noise_pred, bad pivots at chosen points, refusals through the raw entry, statelessness,
concurrent callers, and the band against the two-step route (bitwise) and the resident path.
Tolerance of every comparison with a reference: |d| <= 1e-8 max(1, max|ref|) per particle block, for the mean and the variance each
(_series_predict_ref.close, the family's).  On the ragged case every one of the 64 references is finite, the smallest variance is
0.0095, and the oracle's route and an independent Cholesky route differ by at most 5.5e-14 (mean) and 8.5e-14 (variance) in that
norm: five orders of margin, and no particle is skipped anywhere unless the test is about failure."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import _long_series_cases as LC
import _long_series_predict_ref as LP
import _series_predict_ref as SP
import test_gpu_long_series as TL
import test_gpu_series_predict as TP
from oracle import oracle as O
from conftest import to_tuple

pytestmark = pytest.mark.gpu
bits = TL.bits
close = SP.close
pbits, take, check_against_oracle = TP.pbits, TP.take, TP.check_against_oracle
SENTINEL = 7.25
WS_512 = 8 * 256 * LP.long_series_pred_ws_blocks(32)      # bytes of one 512-point workgroup's workspace


def forecast(engine, series, queries, nodes, noises, sidx, **kw):
    kw.setdefault("want_logpdf", True); kw.setdefault("check", False)
    return engine.predict_long_series_batch(series, queries, nodes, noises, sidx, **kw)


@pytest.fixture(scope="module")
def ragged(engine):
    """tests/_long_series_predict_ref.ragged_case() through the entry under both routings, once"""
    series, queries, nodes, noises, sidx, ref_mean, ref_var, ref_lp = LP.ragged_case()
    res = {flag: forecast(engine, series, queries, nodes, noises, sidx, all_long=flag) for flag in (False, True)}
    for r in res.values():
        for a in (*r[0], *r[1], r[2], r[3]):
            a.setflags(write=False)
    return series, queries, nodes, noises, sidx, (ref_mean, ref_var), res


def raw_call(engine, series, queries, sidx, programs, noises, flags=0, pt_off=None, q_off=None, null=(), want_lp=True):
    """the C entry itself with sentinel-filled outputs one block longer than needed: (out_off, rc, mean, var, msg, info, logpdf)"""
    op_off, ops, prm_off, prm = programs
    P = len(noises)
    if pt_off is None:
        pt_off = np.concatenate([[0], np.cumsum([len(t) for t, _ in series])])
    if q_off is None:
        q_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    sidx = np.ascontiguousarray(sidx, dtype=np.int32)
    ts = np.ascontiguousarray(np.concatenate([t for t, _ in series] + [np.zeros(1)]), dtype=np.float64)
    xs = np.ascontiguousarray(np.concatenate([x for _, x in series] + [np.zeros(1)]), dtype=np.float64)
    tq = np.ascontiguousarray(np.concatenate(list(queries) + [np.zeros(1)]), dtype=np.float64)
    noises = np.ascontiguousarray(noises, dtype=np.float64)
    total = int(sum(len(queries[s]) for s in sidx if 0 <= s < len(queries)))
    mean = np.full(total + 16, SENTINEL); var = np.full(total + 16, SENTINEL)
    off = np.full(P + 1, -1, dtype=np.int64); info = np.full(max(P, 1), 7, dtype=np.int32); lp = np.full(max(P, 1), SENTINEL)
    dp, ip, lp_ = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    arg = lambda name, a, t: None if name in null else a.ctypes.data_as(t)
    rc = engine._lib.agp_predict_long_series_batch(
        engine._ctx, len(pt_off) - 1, arg("pt_off", pt_off, lp_), arg("ts", ts, dp), arg("xs", xs, dp), arg("q_off", q_off, lp_),
        arg("ts_pred", tq, dp), P, arg("series", sidx, ip), arg("op_off", op_off, ip), arg("ops", ops, C.POINTER(C.c_uint8)),
        arg("prm_off", prm_off, ip), arg("prm", prm, dp), arg("noise", noises, dp), None, arg("out_mean", mean, dp),
        arg("out_var", var, dp), arg("out_off", off, lp_), lp.ctypes.data_as(dp) if want_lp else None, arg("out_info", info, ip), flags)
    msg = engine._lib.agp_last_error(engine._ctx)
    return off, rc, mean, var, (msg.decode() if msg else ""), info, lp


def untouched(off, mean, var, info, lp):
    return (mean == SENTINEL).all() and (var == SENTINEL).all() and (off == -1).all() and (info == 7).all() and (lp == SENTINEL).all()


def test_ragged_parity_both_routings(pkg, engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    assert [len(t) for t, _ in series] == TL.LENS and [len(q) for q in queries] == list(LP.RAGGED_M) and len(nodes) == 64
    m_of = np.array([len(queries[s]) for s in sidx])
    for flag in (False, True):
        means, vars_, lp, info = res[flag]
        check_against_oracle(f"ragged, all_long={flag}", res[flag], series, queries, nodes, noises, sidx, refs=refs)
        # the layout through the raw entry: out_off is the prefix sum of the particles' query counts, nothing behind the last block
        off, rc, raw_mean, raw_var, msg, raw_info, raw_lp = raw_call(engine, series, queries, sidx, pkg.encode_batch(nodes), noises,
                                                                     flags=int(flag))
        assert rc == 0, msg
        assert off.tolist() == np.concatenate([[0], np.cumsum(m_of)]).tolist()
        assert np.array_equal(bits(raw_mean[:off[-1]]), np.concatenate([bits(x) for x in means]))
        assert np.array_equal(bits(raw_var[:off[-1]]), np.concatenate([bits(x) for x in vars_]))
        assert (raw_mean[off[-1]:] == SENTINEL).all() and (raw_var[off[-1]:] == SENTINEL).all()
        assert np.array_equal(bits(raw_lp), bits(lp)) and (raw_info == 0).all()
        # the empty series: the prior predictive
        for i in np.flatnonzero(sidx == 0):
            K22 = O.eval_cov(nodes[i].to_tuple(), queries[0])
            assert (means[i] == 0.0).all() and lp[i] == 0.0 and close(vars_[i], np.diag(K22) + noises[i])
        # the series without queries: nothing written, value and info set
        for i in np.flatnonzero(sidx == 1):
            assert means[i].size == 0 and off[i] == off[i + 1] and np.isfinite(lp[i])
        # out_logpdf is the long value entry's under the same flag, bit for bit
        lv, iv = engine.logpdf_long_series_batch(series, nodes, noises, sidx, all_long=flag, check=False)
        assert np.array_equal(bits(lv), bits(lp)) and np.array_equal(iv, info), flag
    # default routing: up to the short cap the launch is predict_series_batch's, and so are the bits
    short = np.flatnonzero(np.array([len(series[s][0]) for s in sidx]) <= pkg.SERIES_MAX_N)
    n_short = int(sidx[short].max()) + 1
    assert len(short) == 4 * n_short == 32
    rs = engine.predict_series_batch(series[:n_short], queries[:n_short], [nodes[i] for i in short], noises[short], sidx[short],
                                     want_logpdf=True, check=False)
    assert np.array_equal(pbits(rs), pbits(take(res[False], short)))
    # ... and under all_long the empty series still is
    empty = np.flatnonzero(sidx == 0)
    assert np.array_equal(pbits(take(res[True], empty)), pbits(take(res[False], empty)))


def test_every_block_count(pkg, engine):
    """all_long: one series per final block count 1 .. 32, full and ragged, two particles each, 17 queries (two query blocks, the
    second with one real row).  n <= 256: exact_particles — the covariance is exact in float64"""
    rng = np.random.default_rng(20261022)
    series, queries, nodes, noises, sidx = [], [], [], [], []
    for s, n in enumerate(TL.BLOCK_LENS):
        if n <= 256:
            ts, particles = LC.exact_particles(pkg, n)
            xs = 0.5 * rng.standard_normal(n)
            nd, nz = [q[0] for q in particles], [q[1] for q in particles]
            q = SP.queries_for(np.arange(512) / 512.0, ts, 17)
        else:
            ts_full, xs_full = pkg.prior.synthetic_series(512, seed=400 + s, shuffle=True)
            ts, xs = ts_full[:n].copy(), xs_full[:n].copy()
            nd, nz = pkg.prior.sample_particles(rng, 2, max_depth=3)
            q = SP.queries_for(ts_full, ts, 17)
        series.append((ts, xs)); queries.append(q)
        nodes += list(nd); noises += list(nz); sidx += [s, s]
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    assert len(nodes) == 50
    res = forecast(engine, series, queries, nodes, noises, sidx, all_long=True)
    check_against_oracle("every block count", res, series, queries, nodes, noises, sidx)


def test_every_leaf_and_combinator(pkg, engine, golden):
    G = pkg
    cases = [c for c in golden["cases"] if "logpdf" in c and len(c["ts"]) <= G.LONG_SERIES_MAX_N]
    assert len(cases) >= 20
    series = [(np.array(c["ts"]), np.array(c["xs"])) for c in cases]
    nodes = [G.from_tuple(to_tuple(c["tree"])) for c in cases]
    noises = np.array([c["noise"] for c in cases])
    queries = []
    for ts, _ in series:                                         # 17 queries: before, inside (one ON a training time) and past the series
        lo, hi = ts.min(), ts.max()
        q = np.linspace(lo - 0.1 * (hi - lo + 1.0), hi + 0.3 * (hi - lo + 1.0), 17)
        q[3] = ts[len(ts) // 2]
        queries.append(q)
    sidx = np.arange(len(cases), dtype=np.int32)
    res = forecast(engine, series, queries, nodes, noises, sidx, all_long=True)
    check_against_oracle("golden, all_long", res, series, queries, nodes, noises, sidx)

    # hand-written trees at 300 points, a repeated training time, queries on training times and on both sides of both locations
    rng = np.random.default_rng(5)
    ts = rng.random(300); ts[241] = ts[7]
    xs = 0.5 * rng.standard_normal(300)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = TL.full_tree(G, 4)                                    # 31 nodes, evaluation stack of depth 5: the D = 8 instantiation
    assert deep.size() == 31
    q = np.array([0.05, 0.29, 0.31, 0.45, 0.59, 0.61, 0.95, ts[7], ts[7], ts[0], 1.2, -0.2, 0.3, 0.6, 0.5, 0.7, 0.1])
    assert q.size == 17 and (q < 0.3).any() and ((q > 0.3) & (q < 0.6)).any() and (q > 0.6).any()
    nodes = [nested, deep, G.GammaExponential(0.42, 0.58, 3.2), G.Constant(0.5) * G.WhiteNoise(0.3)]
    noises = np.array([0.1, 0.2, 0.05, 0.3])
    sidx = np.zeros(4, dtype=np.int32)
    res = forecast(engine, [(ts, xs)], [q], nodes, noises, sidx)
    check_against_oracle("hand-written trees at 300 points", res, [(ts, xs)], [q], nodes, noises, sidx)
    # a chain of ten ChangePoints at the cap
    N = G.LONG_SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N, seed=4)
    q = np.linspace(-0.1, 1.3, 17); q[5] = ts[11]
    chain = TL.cp_chain(G, 10)
    res = forecast(engine, [(ts, xs)], [q], [chain], np.array([0.1]), [0])
    check_against_oracle("ten ChangePoints at 512 points", res, [(ts, xs)], [q], [chain], [0.1], [0])


def test_agrees_with_resident_series_path(engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    means, vars_, lp, info = res[False]
    worst = 0.0
    for n in (177, 257, 442, 512):
        s = TL.LENS.index(n)
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        out = engine.predict_batch([nodes[i] for i in sel], noises[sel], queries[s], check=False)
        mean_r, var_r, info_r = out[0], out[1], out[-1]
        assert (np.asarray(info_r) == 0).all()
        for k, i in enumerate(sel):
            worst = max(worst, np.abs(means[i] - mean_r[k]).max() / max(1.0, np.abs(mean_r[k]).max()),
                        np.abs(vars_[i] - var_r[k]).max() / max(1.0, np.abs(var_r[k]).max()))
            assert close(means[i], mean_r[k]) and close(vars_[i], var_r[k]), (n, i)
    print("long forecast against set_data + predict_batch: worst |d| / max(1, max|ref|)", worst)


def test_batch_independence_bitwise(pkg, engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    P = len(nodes)
    rev = np.arange(P)[::-1]
    lens = np.array([len(series[s][0]) for s in sidx])
    for flag in (False, True):
        call = functools.partial(forecast, engine, all_long=flag)
        assert np.array_equal(pbits(call(series, queries, nodes, noises, sidx)), pbits(res[flag])), flag      # the call repeated
        r_rev = call(series, queries, [nodes[i] for i in rev], noises[rev], sidx[rev])
        assert np.array_equal(pbits(r_rev), pbits(take(res[flag], rev))), flag
        for s in range(len(series)):                             # one series per call
            sel = np.flatnonzero(sidx == s)
            one = call([series[s]], [queries[s]], [nodes[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32))
            assert np.array_equal(pbits(one), pbits(take(res[flag], sel))), (flag, s)
        if not flag:
            for p in np.flatnonzero(lens > pkg.SERIES_MAX_N):    # each long particle alone
                one = call([series[sidx[p]]], [queries[sidx[p]]], [nodes[p]], noises[p:p + 1], [0])
                assert np.array_equal(pbits(one), pbits(take(res[flag], [p]))), p
        # a workspace limit that admits two but not three 512-point workgroups per launch
        limit = 4 << 20
        assert 2 * WS_512 <= limit < 3 * WS_512
        engine.set_workspace_limit(limit)
        try:
            split = call(series, queries, nodes, noises, sidx)
        finally:
            engine.set_workspace_limit(0)
        assert np.array_equal(pbits(split), pbits(res[flag])), flag


def test_query_independence_bitwise(engine, ragged):
    """a query's bits depend on its own time and the particle's inputs: a subset, a reversal and a duplication of the query times of
    two long series (193 points with 529 queries — five rounds —, 512 with 257) give each surviving query its bits"""
    series, queries, nodes, noises, sidx, refs, res = ragged
    means, vars_, _, _ = res[False]
    rng = np.random.default_rng(7)
    for s in (TL.LENS.index(193), TL.LENS.index(512)):
        sel = np.flatnonzero(sidx == s)
        m = len(queries[s])
        picks = {"subset": np.sort(rng.choice(m, size=m // 3, replace=False)), "reversal": np.arange(m)[::-1],
                 "duplication": np.concatenate([np.arange(m), np.arange(m)]), "one": np.array([m - 1])}
        for name, idx in picks.items():
            r = forecast(engine, [series[s]], [queries[s][idx]], [nodes[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32))
            for k, i in enumerate(sel):
                assert np.array_equal(bits(r[0][k]), bits(means[i][idx])) and np.array_equal(bits(r[1][k]), bits(vars_[i][idx])), (s, name)


def test_noise_pred(engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    means, vars_, lp, info = res[False]
    explicit = forecast(engine, series, queries, nodes, noises, sidx, noise_pred=noises.copy())
    assert np.array_equal(pbits(explicit), pbits(res[False]))
    other = noises + 0.375
    shifted = forecast(engine, series, queries, nodes, noises, sidx, noise_pred=other)
    zero = forecast(engine, series, queries, nodes, noises, sidx, noise_pred=np.zeros(len(nodes)))
    for i in range(len(nodes)):
        assert np.array_equal(bits(shifted[0][i]), bits(means[i]))
        base = zero[1][i]      # var = (k** - sum) + noise_pred: the variances are roundings of base + noise_pred
        for got, npred in ((vars_[i], noises[i]), (shifted[1][i], other[i])):
            want = base + npred
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), i


BAD_POINTS = (0, 16, 176, 177, 496, 511)


def bad_pivot_case(G):
    ts = TL.cp_ts()
    xs = np.random.default_rng(31).standard_normal(ts.size)
    nodes = [TL.changepoint_particle(G, k) for k in BAD_POINTS]
    at = 3                                                       # the good particle sits between the failing ones
    nodes.insert(at, G.SquaredExponential(0.3, 0.8))
    noises = np.full(len(nodes), TL.CP_NOISE); noises[at] = 0.1
    q = np.linspace(-0.1, 1.2, 19); q[4] = ts[100]
    return ts, xs, q, nodes, noises, at


def test_bad_pivots_at_chosen_points(pkg, engine):
    ts, xs, q, nodes, noises, at = bad_pivot_case(pkg)
    res = forecast(engine, [(ts, xs)], [q], nodes, noises, np.zeros(len(nodes), dtype=np.int32))
    means, vars_, lp, info = res
    assert np.delete(info, at).tolist() == [k + 1 for k in BAD_POINTS], info
    for i in range(len(nodes)):
        assert means[i].shape == (19,)
        if i != at:
            assert np.isnan(means[i]).all() and np.isnan(vars_[i]).all() and np.isnan(lp[i])
    alone = forecast(engine, [(ts, xs)], [q], [nodes[at]], noises[at:at + 1], [0])
    assert info[at] == 0 and np.array_equal(pbits(alone), pbits(take(res, [at])))
    check_against_oracle("beside failed particles", take(res, [at]), [(ts, xs)], [q], [nodes[at]], [0.1], [0])
    with pytest.raises(pkg.PosDefException) as ei:
        engine.predict_long_series_batch([(ts, xs)], [q], nodes[at:at + 2], noises[at:at + 2], [0, 0], check=True)
    assert ei.value.particle == 1 and ei.value.info == BAD_POINTS[at] + 1


def test_refusals_leave_outputs_untouched(pkg, engine):
    G = pkg
    N = G.LONG_SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    q = np.linspace(1.0, 1.3, 9)
    good = G.SquaredExponential(0.3, 0.8)
    progs = G.encode_batch([good, good])
    s200, s9 = (ts[:200], xs[:200]), (ts[:9], xs[:9])
    mu, cov = O.predict_mvn(good.to_tuple(), 0.1, *s200, q)

    def valid():
        means, vars_, lp, info = forecast(engine, [s200], [q], [good], np.array([0.1]), [0])
        assert info[0] == 0 and close(means[0], mu) and close(vars_[0], np.diag(cov))

    # 513 points
    off, rc, mean, var, msg, info, lp = raw_call(engine, [s9, (ts, xs)], [q, q], [0, 1], progs, [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and str(N + 1) in msg and "AGP_LONG_SERIES_MAX_N" in msg and untouched(off, mean, var, info, lp), msg
    with pytest.raises(ValueError, match="series 0"):
        engine.predict_long_series_batch([(ts, xs)], [q], [good], [0.1], [0])
    # unknown flag bits
    for flags in (2, 1 | 4, 0x80000000):
        off, rc, mean, var, msg, info, lp = raw_call(engine, [s200, s9], [q, q], [0, 1], progs, [0.1, 0.1], flags=flags)
        assert rc == -1 and "flag" in msg and untouched(off, mean, var, info, lp), (flags, msg)
    valid()
    # each null pointer
    for name in ("pt_off", "ts", "xs", "series", "op_off", "ops", "prm_off", "prm", "noise", "out_info", "q_off", "ts_pred", "out_mean",
                 "out_var", "out_off"):
        off, rc, mean, var, msg, info, lp = raw_call(engine, [s200, s9], [q, q], [0, 1], progs, [0.1, 0.1], null=(name,))
        assert rc == -1 and "null pointer" in msg and untouched(off, mean, var, info, lp), (name, msg)
    valid()
    # bad q_off
    off, rc, mean, var, msg, info, lp = raw_call(engine, [s200, s9], [q, q], [0, 1], progs, [0.1, 0.1], q_off=[1, 9, 18])
    assert rc == -1 and "q_off[0]" in msg and untouched(off, mean, var, info, lp)
    off, rc, mean, var, msg, info, lp = raw_call(engine, [s200, s9], [q, q], [0, 1], progs, [0.1, 0.1], q_off=[0, 9, 5])
    assert rc == -1 and "series 1" in msg and "q_off decreases" in msg and untouched(off, mean, var, info, lp)
    valid()
    # LDS, counted from the kernel's own map: the longest ChangePoint chain that fits at the cap predicts, one more is refused
    k_fit = max(k for k in range(1, 60) if LP.cp_chain_fits(k, N))
    assert k_fit >= 10
    sN = (ts[:N], xs[:N])
    fits, too_many = TL.cp_chain(G, k_fit), TL.cp_chain(G, k_fit + 1)
    res = forecast(engine, [sN], [q], [fits], np.array([0.1]), [0])
    check_against_oracle(f"{k_fit} ChangePoints at 512 points", res, [sN], [q], [fits], [0.1], [0])
    off, rc, mean, var, msg, info, lp = raw_call(engine, [sN], [q], [0, 0], G.encode_batch([good, too_many]), [0.1, 0.1])
    assert rc == -3 and "particle 1" in msg and "LDS" in msg and untouched(off, mean, var, info, lp), msg
    # P == 0 touches nothing
    off, rc, mean, var, msg, info, lp = raw_call(engine, [s200], [q], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert rc == 0 and untouched(off, mean, var, info, lp)
    # out_logpdf may be null
    off, rc, mean, var, msg, info, lp = raw_call(engine, [s200], [q], [0], G.encode_batch([good]), [0.1], want_lp=False)
    assert rc == 0 and info[0] == 0 and (lp == SENTINEL).all() and close(mean[:9], mu)
    valid()


def test_stateless(pkg, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    eng = pkg.GPEngine(0)
    try:
        r0 = forecast(eng, series, queries, nodes, noises, sidx)      # a fresh engine on which set_data was never called
        assert np.array_equal(pbits(r0), pbits(res[False]))
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        tq = np.linspace(1.0, 1.2, 7)
        pred0 = eng.predict_batch(rn, rz, tq, check=False)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max,
                    eng.predict_reuse_stats())
        before = snapshot()
        r1 = forecast(eng, series, queries, nodes, noises, sidx, all_long=True)
        assert np.array_equal(pbits(r1), pbits(res[True]))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        pred1 = eng.predict_batch(rn, rz, tq, check=False)
        assert np.array_equal(bits(pred1[0]), bits(pred0[0])) and np.array_equal(bits(pred1[1]), bits(pred0[1]))
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)       # the store still holds its factors: a longer prefix extends them
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_concurrent_callers(engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    out = [None] * 4

    def work(i):
        out[i] = forecast(engine, series, queries, nodes, noises, sidx, all_long=bool(i % 2))

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i, o in enumerate(out):
        assert o is not None and np.array_equal(pbits(o), pbits(res[bool(i % 2)])), i


# ---- the band ----
QS = np.array([0.025, 0.5, 0.975])


def band_inputs():
    series, queries, nodes, noises, sidx, *_ = LP.ragged_case()
    rng = np.random.default_rng(20261023)
    w = rng.random(len(nodes)) + 0.1
    for s in range(len(series)):
        sel = sidx == s
        w[sel] /= w[sel].sum()
    yt = np.column_stack([0.5 + rng.random(len(series)), rng.standard_normal(len(series))])
    return series, queries, nodes, noises, sidx, w, yt


def sbits(band, s):
    return np.concatenate([bits(band.x[s]).ravel(), band.converged[s].astype(np.int64).ravel(), band.iters[s].astype(np.int64).ravel(),
                           bits(band.mean[s]), bits(band.var[s])])


def test_band_bitwise_against_the_two_step_route(pkg, engine, ragged):
    series, queries, nodes, noises, sidx, w, yt = band_inputs()
    for flag in (False, True):
        means, vars_, lp, info = ragged[6][flag]
        band = engine.predict_quantile_long_series_batch(series, queries, nodes, noises, sidx, w, QS, y_transforms=yt, want_moments=True,
                                                         want_logpdf=True, all_long=flag, check=False)
        assert np.array_equal(bits(band.logpdf), bits(lp)) and (band.info == 0).all()
        for s in range(len(series)):
            sel = np.flatnonzero(sidx == s)
            m = len(queries[s])
            assert band.x[s].shape == (m, 3) and band.mean[s].shape == (m,)
            if m == 0:
                continue
            bm, bv = np.stack([means[i] for i in sel]), np.stack([vars_[i] for i in sel])
            mr, vr, inf = pkg.raw_components(bm, bv, info[sel], len(series[s][0]), tuple(yt[s]))
            assert (inf == 0).all()
            x, conv, it = engine.mixture_quantile(mr, vr, w[sel], QS)
            mean, var, _ = engine.mixture_moments(mr, w[sel], vars=vr, space=0)
            assert np.array_equal(bits(band.x[s]), bits(x)) and np.array_equal(band.converged[s], conv) and conv.all(), (flag, s)
            assert np.array_equal(band.iters[s], it), (flag, s)
            assert np.array_equal(bits(band.mean[s]), bits(mean)) and np.array_equal(bits(band.var[s]), bits(var)), (flag, s)
    # the module-level wrapper takes the same route
    lw = np.log(w)
    out = pkg.predict_quantile_series(engine, series, queries, nodes, noises, sidx, lw, QS, y_transforms=yt, max_n=pkg.LONG_SERIES_MAX_N)
    assert len(out) == len(series) and out[14][0].shape == (36, 3) and out[14][1].all()


def test_band_agrees_with_resident_path(engine, ragged):
    series, queries, nodes, noises, sidx, w, yt = band_inputs()
    s = TL.LENS.index(442)
    sel = np.flatnonzero(sidx == s)
    tol = 1e-10      # (both searches to well inside the comparison's bound)
    band = engine.predict_quantile_long_series_batch([series[s]], [queries[s]], [nodes[i] for i in sel], noises[sel],
                                                     np.zeros(len(sel), dtype=np.int32), w[sel], QS, tol=tol, check=False)
    engine.set_data(*series[s])
    x_r, conv_r, _, info_r = engine.predict_quantile_batch([nodes[i] for i in sel], noises[sel], queries[s], w[sel], QS, tol=tol, check=False)
    assert (np.asarray(info_r) == 0).all() and band.converged[0].all() and np.asarray(conv_r).all()
    d = np.abs(band.x[0] - x_r).max() / max(1.0, np.abs(x_r).max())
    print("band at 442 points against predict_quantile_batch: |d| / max(1, max|ref|)", d)
    assert np.isfinite(x_r).all() and d <= 1e-8


def test_band_with_a_failed_particle(pkg, engine):
    ts, xs, q, nodes, noises, at = bad_pivot_case(pkg)
    ts2, xs2 = pkg.prior.synthetic_series(200, seed=11)
    good = nodes[at]
    # series 0 holds a failed particle beside the good one; series 1 and 2 (200 and 512 points) hold good ones only
    nds = [good, nodes[0], good, good, good]
    nz = np.array([0.1, TL.CP_NOISE, 0.1, 0.2, 0.1])
    sidx = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    w = np.array([0.5, 0.5, 0.25, 0.75, 1.0])
    family = [(ts, xs), (ts2, xs2), (ts, xs)]
    band = engine.predict_quantile_long_series_batch(family, [q, q, q], nds, nz, sidx, w, QS, want_moments=True, check=False)
    assert band.info.tolist() == [0, BAD_POINTS[0] + 1, 0, 0, 0]
    assert np.isnan(band.x[0]).all() and np.isnan(band.mean[0]).all() and not band.converged[0].any()
    rest = engine.predict_quantile_long_series_batch(family[1:], [q, q], nds[2:], nz[2:], sidx[2:] - 1, w[2:], QS, want_moments=True, check=False)
    for s in (1, 2):
        assert np.isfinite(band.x[s]).all() and np.array_equal(sbits(band, s), sbits(rest, s - 1)), s
