"""GPU tests of agp_predict_series_batch (forecasts of many short series in one fused launch; k_series_predict,
csrc/agp_series_kernel.hpp): parity with oracle.predict_mvn on ragged input with ragged query sets, every leaf and combinator, every
block count, agreement with the resident-series path, batch independence (bitwise), statelessness, non-PD reporting, argument errors,
concurrent callers and chaining into mixture_quantile.
Tolerance of every comparison with a reference: |d| <= 1e-8 max(1, max|ref|) per particle, for the mean and the variance each (the
project's LP_TOL as tests/test_gpu_parity.py applies it to predict_batch).  On the ragged case the oracle's LU route and an
independent Cholesky route differ by at most 3.2e-14 (mean) and 2.1e-15 (variance) in that norm and the smallest variance is 0.021:
five orders of margin, no cancellation case.  No particle is skipped anywhere: info == 0 and a finite reference for every particle,
unless the test is about failure."""
import ctypes as C
import threading

import numpy as np
import pytest

import _series_cases as S
import _series_predict_ref as R
import test_gpu_series as TS
from oracle import oracle as O
from conftest import to_tuple

pytestmark = pytest.mark.gpu
bits = TS.bits
close = R.close


def pbits(res):
    """every output of a call as one int64 vector: means, variances (bit patterns), [logpdf], info"""
    means, vars_, *rest = res
    parts = [bits(x) for x in means] + [bits(x) for x in vars_]
    if len(rest) == 2:
        parts.append(bits(rest[0]))
    parts.append(np.asarray(rest[-1], dtype=np.int64))
    return np.concatenate(parts)


def take(res, sel):
    means, vars_, *rest = res
    return ([means[i] for i in sel], [vars_[i] for i in sel], *[r[np.asarray(sel)] for r in rest])


def check_against_oracle(name, res, series, queries, nodes, noises, sidx, refs=None, noise_pred=None):
    means, vars_, *_, info = res
    assert (np.asarray(info) == 0).all(), (name, info)
    worst_m = worst_v = 0.0
    fails = []
    for i, nd in enumerate(nodes):
        s = int(sidx[i])
        if refs is not None:
            mu, var = refs[0][i], refs[1][i]
        else:
            npred = None if noise_pred is None else float(noise_pred[i])
            mu, cov = O.predict_mvn(nd.to_tuple(), float(noises[i]), *series[s], queries[s], noise_pred=npred)
            var = np.diag(cov)
        assert np.isfinite(mu).all() and np.isfinite(var).all(), (name, i)
        assert means[i].shape == mu.shape and vars_[i].shape == var.shape, (name, i)
        if mu.size:
            worst_m = max(worst_m, np.abs(means[i] - mu).max() / max(1.0, np.abs(mu).max()))
            worst_v = max(worst_v, np.abs(vars_[i] - var).max() / max(1.0, np.abs(var).max()))
        if not (close(means[i], mu) and close(vars_[i], var)):
            fails.append(f"{name} particle {i} (series {s}, {nd.to_tuple()})")
    print(f"[series-predict] {name}: worst |d| / max(1, max|ref|): mean {worst_m:.3e}, variance {worst_v:.3e} over {len(nodes)} particles")
    assert not fails, "\n".join(fails)


@pytest.fixture(scope="module")
def ragged(engine):
    """tests/_series_predict_ref.ragged_case() through the entry, once, with the training log-likelihood"""
    series, queries, nodes, noises, sidx, ref_mean, ref_var = R.ragged_case()
    res = engine.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, check=False)
    for a in (*res[0], *res[1], res[2], res[3]):
        a.setflags(write=False)
    return series, queries, nodes, noises, sidx, (ref_mean, ref_var), res


def test_ragged_parity(pkg, engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    means, vars_, lp, info = res
    assert [len(t) for t, _ in series] == [0, 1, 2, 15, 16, 17, 33, 126, 144, pkg.SERIES_MAX_N]
    assert [len(q) for q in queries] == [5, 0, 1, 15, 16, 17, 33, 12, 36, 65] and len(nodes) == 60
    assert (info == 0).all()
    check_against_oracle("ragged", res, series, queries, nodes, noises, sidx, refs=refs)
    # the layout: out_off is the prefix sum of the particles' query counts, and the views are cut from one particle-major array
    m_of = np.array([len(queries[s]) for s in sidx])
    off, _, raw_mean, raw_var, _, _ = raw_call(engine, series, queries, sidx, pkg.encode_batch(nodes), noises)
    assert off.tolist() == np.concatenate([[0], np.cumsum(m_of)]).tolist()
    assert np.array_equal(bits(raw_mean[:off[-1]]), np.concatenate([bits(x) for x in means]))
    assert np.array_equal(bits(raw_var[:off[-1]]), np.concatenate([bits(x) for x in vars_]))
    assert (raw_mean[off[-1]:] == SENTINEL).all() and (raw_var[off[-1]:] == SENTINEL).all()      # nothing behind the last block
    # the empty series: the prior predictive
    for i in np.flatnonzero(sidx == 0):
        K22 = O.eval_cov(nodes[i].to_tuple(), queries[0])
        assert (means[i] == 0.0).all() and lp[i] == 0.0
        assert close(vars_[i], np.diag(K22) + noises[i])
    # the series without queries: nothing written (its particles' blocks are empty, their neighbours' blocks adjacent), value and info set
    for i in np.flatnonzero(sidx == 1):
        assert means[i].size == 0 and vars_[i].size == 0 and off[i] == off[i + 1] and np.isfinite(lp[i])


def test_evaluator_coverage(pkg, engine, golden):
    G = pkg
    cases = [c for c in golden["cases"] if "logpdf" in c and len(c["ts"]) <= G.SERIES_MAX_N]
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
    res = engine.predict_series_batch(series, queries, nodes, noises, sidx)      # ONE ragged call, each case its own series
    check_against_oracle("golden", res, series, queries, nodes, noises, sidx)

    # hand-written trees on a series with a repeated training time
    rng = np.random.default_rng(5)
    ts = rng.random(70); ts[41] = ts[7]
    xs = 0.5 * rng.standard_normal(70)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = TS.full_tree(G, 4)                                    # 31 nodes, evaluation stack of depth 5: the D = 8 instantiation
    assert deep.size() == 31
    q = np.array([0.05, 0.29, 0.31, 0.45, 0.59, 0.61, 0.95, ts[7], ts[7], ts[0], 1.2, -0.2, 0.3, 0.6, 0.5, 0.7, 0.1])
    assert q.size == 17 and (q < 0.3).any() and ((q > 0.3) & (q < 0.6)).any() and (q > 0.6).any()      # both sides of both locations
    nodes = [nested, deep, G.GammaExponential(0.42, 0.58, 3.2), G.Constant(0.5) * G.WhiteNoise(0.3)]
    noises = np.array([0.1, 0.2, 0.05, 0.3])
    sidx = np.zeros(4, dtype=np.int32)
    res = engine.predict_series_batch([(ts, xs)], [q], nodes, noises, sidx)
    check_against_oracle("hand-written", res, [(ts, xs)], [q], nodes, noises, sidx)
    # a chain of 8 ChangePoints at the cap
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N, seed=4)
    q = np.linspace(-0.1, 1.3, 17); q[5] = ts[11]
    chain = TS.cp_chain(G, 8)
    res = engine.predict_series_batch([(ts, xs)], [q], [chain], [0.1], [0])
    check_against_oracle("ChangePoint chain at the cap", res, [(ts, xs)], [q], [chain], [0.1], [0])


def block_count_case(pkg):
    lens = (49, 80, 81, 97, 112, 145, 161)
    rng = np.random.default_rng(20261019)
    series, queries, nodes, noises, sidx = [], [], [], [], []
    for s, n in enumerate(lens):
        ts, xs = pkg.prior.synthetic_series(256, seed=200 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        queries.append(R.queries_for(ts, ts[:n], 17))
        nd, nz = pkg.prior.sample_particles(rng, 6, max_depth=3)
        nodes += nd; noises += list(nz); sidx += [s] * 6
    return series, queries, nodes, np.array(noises), np.array(sidx, dtype=np.int32)


def test_parity_at_the_remaining_block_counts(pkg, engine):
    """the lengths of the ragged case end in 1, 2, 3, 8, 9 or 11 blocks of 16: here every other final block count, full and ragged"""
    series, queries, nodes, noises, sidx = block_count_case(pkg)
    assert len(nodes) == 42
    res = engine.predict_series_batch(series, queries, nodes, noises, sidx, check=False)
    check_against_oracle("block counts", res, series, queries, nodes, noises, sidx)


def test_agrees_with_resident_series_path(engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    means, vars_, lp, info = res
    for s in (5, 7, 8):                                          # 17, 126 and 144 points
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        out = engine.predict_batch([nodes[i] for i in sel], noises[sel], queries[s], check=False)
        mean_r, var_r, info_r = out[0], out[1], out[-1]
        assert (np.asarray(info_r) == 0).all()
        for k, i in enumerate(sel):
            assert close(means[i], mean_r[k]) and close(vars_[i], var_r[k]), (s, i)
    # the training log-likelihood is the value entry's, bit for bit
    lp_v, info_v = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)
    assert np.array_equal(bits(lp_v), bits(lp)) and np.array_equal(info_v, info)
    # noise_pred = noise given explicitly: the default's bits; another noise_pred shifts the variance by exactly the difference
    explicit = engine.predict_series_batch(series, queries, nodes, noises, sidx, noise_pred=noises.copy(), want_logpdf=True, check=False)
    assert np.array_equal(pbits(explicit), pbits(res))
    other = noises + 0.375
    shifted = engine.predict_series_batch(series, queries, nodes, noises, sidx, noise_pred=other, check=False)
    zero = engine.predict_series_batch(series, queries, nodes, noises, sidx, noise_pred=np.zeros(len(nodes)), check=False)
    for i in range(len(nodes)):
        assert np.array_equal(bits(shifted[0][i]), bits(means[i]))
        # var = (k** - sum) + noise_pred: the two variances are roundings of base + noise and base + other
        base = zero[1][i]
        for got, npred in ((vars_[i], noises[i]), (shifted[1][i], other[i])):
            want = base + npred
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), i


def test_batch_independence_bitwise(engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    P = len(nodes)
    rev = np.arange(P)[::-1]
    r_rev = engine.predict_series_batch(series, queries, [nodes[i] for i in rev], noises[rev], sidx[rev], want_logpdf=True, check=False)
    assert np.array_equal(pbits(r_rev), pbits(take(res, rev)))
    for s in range(len(series)):                                 # one series at a time
        sel = np.flatnonzero(sidx == s)
        one = engine.predict_series_batch([series[s]], [queries[s]], [nodes[i] for i in sel], noises[sel],
                                          np.zeros(len(sel), dtype=np.int32), want_logpdf=True, check=False)
        assert np.array_equal(pbits(one), pbits(take(res, sel))), s
    for p in range(P):                                           # each particle alone
        one = engine.predict_series_batch([series[sidx[p]]], [queries[sidx[p]]], [nodes[p]], noises[p:p + 1], [0], want_logpdf=True,
                                          check=False)
        assert np.array_equal(pbits(one), pbits(take(res, [p]))), p


def test_stateless(pkg, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    eng = pkg.GPEngine(0)
    try:
        # a fresh engine on which set_data was never called
        r0 = eng.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, check=False)
        assert np.array_equal(pbits(r0), pbits(res))
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)      # (with copies: dedup counts them)
        tq = np.linspace(1.0, 1.2, 7)
        pred0 = eng.predict_batch(rn, rz, tq, check=False)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max,
                    eng.predict_reuse_stats())
        before = snapshot()
        r1 = eng.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, check=False)
        assert np.array_equal(pbits(r1), pbits(res))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        pred1 = eng.predict_batch(rn, rz, tq, check=False)
        assert np.array_equal(bits(pred1[0]), bits(pred0[0])) and np.array_equal(bits(pred1[1]), bits(pred0[1]))
        # the store still holds its factors: a longer prefix extends them
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_concurrent_callers(engine, ragged):
    series, queries, nodes, noises, sidx, refs, res = ragged
    out = [None] * 4

    def work(i):
        out[i] = engine.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, check=False)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for o in out:
        assert o is not None and np.array_equal(pbits(o), pbits(res))


def test_non_positive_definite(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(40, seed=2)
    q = np.linspace(1.0, 1.5, 19)
    bad = G.Constant(1.0)
    good, good2 = G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.3, 0.9) + G.Linear(0.2, 0.3, 0.4)
    first = S.first_bad_minor(O.compute_cov_matrix_vectorized(bad.to_tuple(), -0.5, ts))
    assert first == 2
    res = engine.predict_series_batch([(ts, xs)], [q], [good, bad, good2], [0.1, -0.5, 0.2], [0, 0, 0], want_logpdf=True, check=False)
    means, vars_, lp, info = res
    assert info.tolist() == [0, first, 0]
    assert means[1].shape == (19,) and np.isnan(means[1]).all() and np.isnan(vars_[1]).all() and np.isnan(lp[1])
    for i, (nd, nz) in ((0, (good, 0.1)), (2, (good2, 0.2))):
        alone = engine.predict_series_batch([(ts, xs)], [q], [nd], [nz], [0], want_logpdf=True, check=False)
        assert alone[3][0] == 0 and np.array_equal(pbits(alone), pbits(take(res, [i])))
    check_against_oracle("beside a failed particle", take(res, [0, 2]), [(ts, xs)], [q], [good, good2], [0.1, 0.2], [0, 0])
    with pytest.raises(G.PosDefException) as ei:
        engine.predict_series_batch([(ts, xs), (ts, xs)], [q, q], [good, bad], [0.1, -0.5], [0, 1], check=True)
    assert ei.value.particle == 1 and ei.value.info == first


SENTINEL = 7.25


def raw_call(engine, series, queries, sidx, programs, noises, pt_off=None, q_off=None, null=()):
    """the C entry itself with sentinel-filled outputs one block longer than needed: (out_off, rc, mean, var, msg, info)"""
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
    off = np.full(P + 1, -1, dtype=np.int64); info = np.full(P, 7, dtype=np.int32)
    dp, ip, lp_ = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    arg = lambda name, a, t: None if name in null else a.ctypes.data_as(t)
    rc = engine._lib.agp_predict_series_batch(engine._ctx, len(pt_off) - 1, pt_off.ctypes.data_as(lp_), ts.ctypes.data_as(dp),
                                              xs.ctypes.data_as(dp), arg("q_off", q_off, lp_), arg("ts_pred", tq, dp), P,
                                              sidx.ctypes.data_as(ip), op_off.ctypes.data_as(ip), ops.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp), None,
                                              arg("out_mean", mean, dp), arg("out_var", var, dp), arg("out_off", off, lp_), None,
                                              info.ctypes.data_as(ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return off, rc, mean, var, (msg.decode() if msg else ""), info


def test_errors_name_the_culprit(pkg, engine):
    G = pkg
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    q = np.linspace(1.0, 1.3, 9)
    good = G.SquaredExponential(0.3, 0.8)
    progs = G.encode_batch([good, good])
    s20, s9 = (ts[:20], xs[:20]), (ts[:9], xs[:9])
    mu20, cov20 = O.predict_mvn(good.to_tuple(), 0.1, *s20, q)

    def valid():
        means, vars_, info = engine.predict_series_batch([s20], [q], [good], [0.1], [0])
        assert info[0] == 0 and close(means[0], mu20) and close(vars_[0], np.diag(cov20))

    def untouched(mean, var, off):
        return (mean == SENTINEL).all() and (var == SENTINEL).all() and (off == -1).all()

    off, rc, mean, var, msg, _ = raw_call(engine, [s20, s9], [q, q], [0, 1], progs, [0.1, 0.1], q_off=[1, 9, 18])
    assert rc == -1 and "q_off[0]" in msg and untouched(mean, var, off)
    valid()
    off, rc, mean, var, msg, _ = raw_call(engine, [s20, s9], [q, q], [0, 1], progs, [0.1, 0.1], q_off=[0, 9, 5])
    assert rc == -1 and "series 1" in msg and "q_off decreases" in msg and untouched(mean, var, off)
    valid()
    for name in ("q_off", "ts_pred", "out_mean", "out_var", "out_off"):
        off, rc, mean, var, msg, _ = raw_call(engine, [s20, s9], [q, q], [0, 1], progs, [0.1, 0.1], null=(name,))
        assert rc == -1 and "null pointer" in msg, name
    valid()
    with pytest.raises(G.AGPError, match=r"particle 1.*series index 3"):
        engine.predict_series_batch([s20, s9], [q, q], [good, good], [0.1, 0.1], [0, 3])
    valid()
    with pytest.raises(G.AGPError, match=r"particle 0.*series index -1"):
        engine.predict_series_batch([s20], [q], [good], [0.1], [-1])
    long_series = [(ts[:5], xs[:5]), (ts, xs)]
    off, rc, mean, var, msg, _ = raw_call(engine, long_series, [q, q], [0, 1], progs, [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and str(N + 1) in msg and untouched(mean, var, off)
    off, rc, mean, var, msg, _ = raw_call(engine, [s20, s9], [q, q], [0, 1], progs, [0.1, 0.1], pt_off=[0, 30, 20])
    assert rc == -1 and "series 1" in msg and "pt_off decreases" in msg
    with pytest.raises(ValueError, match="series 0"):
        engine.predict_series_batch([(ts, xs)], [q], [good], [0.1], [0])
    valid()
    # a malformed program: particle 1 is a lone '+'
    op_off, ops, prm_off, prm = G.encode_batch([good])
    bad_prog = (np.array([0, ops.size, ops.size + 1], dtype=np.int32), np.concatenate([ops, np.array([6], dtype=np.uint8)]),
                np.array([0, prm.size, prm.size], dtype=np.int32), prm)
    off, rc, mean, var, msg, _ = raw_call(engine, [s20], [q], [0, 0], bad_prog, [0.1, 0.1])
    assert rc == -3 and "particle 1" in msg and "underflow" in msg and untouched(mean, var, off)
    valid()
    # per-point tables beyond the LDS budget at the cap, counted from the kernel's own map: the longest chain of ChangePoints that
    # fits predicts, one more is refused — and fits a 100-point series
    k_fit = max(k for k in range(1, 40) if R.cp_chain_fits(k, N))
    fits, too_many = TS.cp_chain(G, k_fit), TS.cp_chain(G, k_fit + 1)
    sN, s100 = (ts[:N], xs[:N]), (ts[:100], xs[:100])
    res = engine.predict_series_batch([sN], [q], [fits], [0.1], [0])
    check_against_oracle("ChangePoint chain at the cap", res, [sN], [q], [fits], [0.1], [0])
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*LDS"):
        engine.predict_series_batch([sN], [q], [good, too_many], [0.1, 0.1], [0, 0])
    res = engine.predict_series_batch([s100], [q], [too_many], [0.1], [0])
    check_against_oracle("ChangePoint chain at 100 points", res, [s100], [q], [too_many], [0.1], [0])
    # P == 0 touches nothing
    off, rc, mean, var, msg, _ = raw_call(engine, [s20], [q], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert rc == 0 and untouched(mean, var, off)
    valid()


def test_chains_into_mixture_quantile(engine, ragged):
    """the (P_s, m_s) block of one series' adjacent particles goes to mixture_quantile as it is"""
    series, queries, nodes, noises, sidx, refs, res = ragged
    means, vars_, lp, info = res
    s = 8                                                        # 144 points, 36 queries
    sel = np.flatnonzero(sidx == s)
    assert len(sel) == 6 and (np.diff(sel) == 1).all()
    w = np.array([0.3, 0.1, 0.2, 0.15, 0.05, 0.2])
    qs = np.array([0.025, 0.5, 0.975])
    bm, bv = np.stack([means[i] for i in sel]), np.stack([vars_[i] for i in sel])
    assert bm.shape == (6, 36)
    tol = 1e-10      # (both searches to well inside the comparison's bound: the default 1e-5 is the searches' own, not the routes')
    x, conv, _ = engine.mixture_quantile(bm, bv, w, qs, tol=tol)
    engine.set_data(*series[s])
    x_r, conv_r, _, info_r = engine.predict_quantile_batch([nodes[i] for i in sel], noises[sel], queries[s], w, qs, tol=tol, check=False)
    assert (np.asarray(info_r) == 0).all() and np.asarray(conv).all() and np.asarray(conv_r).all()
    assert np.isfinite(x_r).all() and np.abs(x - x_r).max() <= 1e-8 * max(1.0, np.abs(x_r).max())
