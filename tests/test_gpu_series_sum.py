"""GPU tests of agp_predict_sum_series_batch (decompositions of many short series in one fused launch; k_series_predict_sum,
csrc/agp_series_kernel.hpp): parity with oracle.infer_gp_sum on ragged input at the sizes where the coded-row map can go wrong, the
exact properties 1e-8 is too loose to see, other component counts, every leaf and combinator, agreement with the resident route,
batch independence (bitwise), statelessness, concurrent callers, non-PD and row-level reporting, argument errors and chaining into
mixture_quantile.
Tolerance of every comparison with a reference: |d| <= 1e-8 max(1, max|ref|) per particle block, for the means, the variances and
the quantiles each (tests/_series_predict_ref.close, the family's own).  On the ragged case the NumPy restatement of the kernel's
algorithm (tests/_series_sum_ref.py, LAPACK's factor) and the oracle differ by at most 5.1e-14 in that norm: five orders of margin.
The smallest variance there is the jitter 1e-8 itself, on the rows of Constant(0) sentinel components: exact by construction (see
test_exact_pins), not a cancellation.  No particle is skipped anywhere."""
import ctypes as C
import threading

import numpy as np
import pytest

import _series_cases as S
import _series_sum_ref as R
import test_gpu_series as TS
from oracle import oracle as O
from conftest import to_tuple

pytestmark = pytest.mark.gpu
bits = TS.bits
close = R.close
EPS = np.finfo(np.float64).eps


def sbits(r):
    """every output of a call as one int64 vector: means, variances, quantiles (bit patterns), [logpdf], info"""
    parts = [bits(a) for a in r.mean] + [bits(a) for a in r.var] + [bits(np.ascontiguousarray(a)).ravel() for a in r.x]
    if r.logpdf is not None:
        parts.append(bits(r.logpdf))
    parts.append(np.asarray(r.info, dtype=np.int64))
    return np.concatenate(parts)


def take(r, sel):
    sel = list(sel)
    return type(r)([r.mean[i] for i in sel], [r.var[i] for i in sel], [r.x[i] for i in sel],
                   None if r.logpdf is None else r.logpdf[np.asarray(sel)], r.info[np.asarray(sel)])


def run(engine, series, queries, splits, noises, sidx, yts=None, q=R.Q, **kw):
    return engine.predict_sum_series_batch(series, queries, splits, noises, sidx, q=q, y_transforms=yts, want_var=True, want_logpdf=True,
                                           check=False, **kw)


def check_against_oracle(name, r, series, queries, splits, noises, sidx, yts=None, refs=None, noise_pred=None, q=R.Q):
    assert (np.asarray(r.info) == 0).all(), (name, r.info)
    worst = [0.0, 0.0, 0.0]
    fails = []
    for i, sp in enumerate(splits):
        s = int(sidx[i])
        if refs is not None:
            ref = (refs[0][i], refs[1][i], refs[2][i])
        else:
            yt = (1.0, 0.0) if yts is None else yts[s]
            npred = None if noise_pred is None else float(noise_pred[i])
            ref = R.oracle_rows([c.to_tuple() for c in sp], float(noises[i]), *series[s], queries[s], noise_pred=npred, y_transform=yt, q=q)
        got = (r.mean[i], r.var[i], r.x[i])
        for k in range(3):
            assert np.isfinite(ref[k]).all() and got[k].shape == ref[k].shape, (name, i, k)
            if ref[k].size:
                worst[k] = max(worst[k], np.abs(got[k] - ref[k]).max() / (1e-8 * max(1.0, np.abs(ref[k]).max())))
        if not all(close(got[k], ref[k]) for k in range(3)):
            fails.append(f"{name} particle {i} (series {s}, {[c.to_tuple() for c in sp]})")
    print(f"[series-sum] {name}: worst |d| / (1e-8 max(1, max|ref|)): mean {worst[0]:.3e}, variance {worst[1]:.3e}, quantiles {worst[2]:.3e} "
          f"over {len(splits)} particles")
    assert not fails, "\n".join(fails)


@pytest.fixture(scope="module")
def ragged(engine):
    """tests/_series_sum_ref.ragged_case() through the entry, once"""
    series, queries, splits, noises, sidx, yts, ref_mean, ref_var, ref_x = R.ragged_case()
    r = run(engine, series, queries, splits, noises, sidx, yts)
    for a in (*r.mean, *r.var, *r.x, r.logpdf, r.info):
        a.setflags(write=False)
    return series, queries, splits, noises, sidx, yts, (ref_mean, ref_var, ref_x), r


SENTINEL = 7.25


def raw_call(engine, G, series, queries, sidx, splits, noises, M=None, programs=None, pt_off=None, q_off=None, null=(), q=R.Q, nq=None,
             slope=None, icpt=None, noise_pred=None):
    """the C entry itself with sentinel-filled outputs one block longer than needed: (rc, msg, out_off, mean, var, x, lp, info)"""
    M = (len(splits[0]) if len(splits) else 2) if M is None else M
    op_off, ops, prm_off, prm = programs if programs is not None else G.encode_batch([c for sp in splits for c in sp])
    P = len(noises)
    S_ = len(series)
    if pt_off is None:
        pt_off = np.concatenate([[0], np.cumsum([len(t) for t, _ in series])])
    if q_off is None:
        q_off = np.concatenate([[0], np.cumsum([len(v) for v in queries])])
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.int64)
    sidx = np.ascontiguousarray(sidx, dtype=np.int32)
    ts = np.ascontiguousarray(np.concatenate([t for t, _ in series] + [np.zeros(1)]), dtype=np.float64)
    xs = np.ascontiguousarray(np.concatenate([x for _, x in series] + [np.zeros(1)]), dtype=np.float64)
    tq = np.ascontiguousarray(np.concatenate(list(queries) + [np.zeros(1)]), dtype=np.float64)
    noises = np.ascontiguousarray(noises, dtype=np.float64)
    qa = np.ascontiguousarray(q, dtype=np.float64)
    nq = len(qa) if nq is None else nq
    rows = (max(M, 0) + 1) * int(sum(len(queries[s]) for s in sidx if 0 <= s < len(queries)))
    mean = np.full(rows + 16, SENTINEL); var = np.full(rows + 16, SENTINEL); x = np.full((rows + 16) * max(1, len(qa)), SENTINEL)
    lp = np.full(max(1, P), SENTINEL)
    off = np.full(P + 1, -1, dtype=np.int64); info = np.full(max(1, P), 7, dtype=np.int32)
    dp, ip, lp_ = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    opt = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    slope, icpt, noise_pred = opt(slope), opt(icpt), opt(noise_pred)
    arg = lambda name, a, t: None if (name in null or a is None) else a.ctypes.data_as(t)
    rc = engine._lib.agp_predict_sum_series_batch(
        engine._ctx, S_, pt_off.ctypes.data_as(lp_), ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), arg("q_off", q_off, lp_),
        arg("ts_pred", tq, dp), P, M, sidx.ctypes.data_as(ip), arg("op_off", op_off, ip), ops.ctypes.data_as(C.POINTER(C.c_uint8)),
        prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp), arg("noise_pred", noise_pred, dp),
        arg("slope", slope, dp), arg("icpt", icpt, dp), arg("q", qa, dp), nq, arg("out_mean", mean, dp), arg("out_var", var, dp),
        arg("out_x", x, dp), arg("out_off", off, lp_), arg("out_logpdf", lp, dp), arg("out_info", info, ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), off, mean, var, x, lp, info


def test_ragged_parity(pkg, engine, ragged):
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    assert [len(t) for t, _ in series] == [0, 1, 15, 16, 17, 33, 126, 144, pkg.SERIES_MAX_N]
    assert [len(v) for v in queries] == [5, 0, 1, 6, 16, 22, 11, 12, 36] and len(splits) == 42
    assert (r.info == 0).all()
    check_against_oracle("ragged", r, series, queries, splits, noises, sidx, refs=refs)
    # the layout: out_off is (M + 1) times the prefix sum of the particles' query counts; the views are cut from particle-major arrays
    m_of = np.array([len(queries[s]) for s in sidx])
    rc, msg, off, mean, var, x, lp, info = raw_call(engine, pkg, series, queries, sidx, splits, noises, slope=yts[:, 0], icpt=yts[:, 1])
    assert rc == 0, msg
    assert off.tolist() == np.concatenate([[0], 3 * np.cumsum(m_of)]).tolist()
    n_out = int(off[-1])
    assert np.array_equal(bits(mean[:n_out]), np.concatenate([bits(a) for a in r.mean]))
    assert np.array_equal(bits(var[:n_out]), np.concatenate([bits(a) for a in r.var]))
    assert np.array_equal(bits(x[:3 * n_out]), np.concatenate([bits(np.ascontiguousarray(a)).ravel() for a in r.x]))
    assert (mean[n_out:] == SENTINEL).all() and (var[n_out:] == SENTINEL).all() and (x[3 * n_out:] == SENTINEL).all()
    assert np.array_equal(bits(lp), bits(r.logpdf)) and np.array_equal(info, r.info)
    # the training log-likelihood is that of the summed model
    for i in (0, 9, 21, 30, 41):
        s = sidx[i]
        tree = ("+", splits[i][0].to_tuple(), splits[i][1].to_tuple())
        want = O.gp_logpdf(tree, float(noises[i]), *series[s])
        assert abs(r.logpdf[i] - want) <= 1e-8 * max(1.0, abs(want)), i
    # the empty series: the prior of every part, exactly 0 scaled means
    a, b = yts[0]
    for i in np.flatnonzero(sidx == 0):
        assert r.logpdf[i] == 0.0 and (r.mean[i][:5] == (0.0 - b) / a + b / a).all() and (r.mean[i][5:] == (0.0 - b) / a).all()
    # the series without queries: nothing written, value and info set
    for i in np.flatnonzero(sidx == 1):
        assert r.mean[i].size == 0 and r.x[i].shape == (0, 3) and off[i] == off[i + 1] and np.isfinite(r.logpdf[i])


def test_exact_pins(pkg, engine, ragged):
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    P = len(splits)
    # 1. a Constant(0) sentinel component: scaled mean exactly 0, variance exactly the jitter (identity transform: scaled = raw)
    ident = run(engine, series, queries, splits, noises, sidx, None)
    assert (ident.info == 0).all()
    seen = 0
    for i, sp in enumerate(splits):
        m = len(queries[sidx[i]])
        for c, comp in enumerate(sp):
            if comp.to_tuple() == ("C", 0.0) and m:
                blk = slice(c * m, (c + 1) * m)
                assert (ident.mean[i][blk] == 0.0).all() and (ident.var[i][blk] == 1e-8).all(), (i, c)
                seen += 1
    assert seen >= 10
    # 2. noise_pred goes on the observable rows only
    zero = run(engine, series, queries, splits, noises, sidx, yts, noise_pred=np.zeros(P))
    own = run(engine, series, queries, splits, noises, sidx, yts, noise_pred=noises.copy())
    assert np.array_equal(sbits(own), sbits(r))          # NULL means the particle's own noise
    for i in range(P):
        s = sidx[i]; m = len(queries[s]); a = yts[s][0]
        F, X = slice(0, 2 * m), slice(2 * m, 3 * m)
        for what in ("mean", "var", "x"):
            assert np.array_equal(bits(np.ascontiguousarray(getattr(zero, what)[i][F])), bits(np.ascontiguousarray(getattr(own, what)[i][F]))), (i, what)
        assert np.array_equal(bits(zero.mean[i][X]), bits(own.mean[i][X])), i
        d = own.var[i][X] - zero.var[i][X]
        assert (np.abs(d - noises[i] / (a * a)) <= 4 * EPS * own.var[i][X]).all(), i
    # 3. the quantiles are fma(sqrt(var), z, mean) of the returned marginals
    z = R.ndtri(R.Q)
    worst = 0.0
    for i in range(P):
        sd = np.sqrt(r.var[i])
        want = r.mean[i][:, None] + sd[:, None] * z[None, :]
        scale = np.maximum(np.abs(r.mean[i])[:, None], np.abs(sd[:, None] * z[None, :]))
        if want.size:
            assert (np.abs(r.x[i] - want) <= 4 * EPS * scale).all(), i
            worst = max(worst, (np.abs(r.x[i] - want) / np.maximum(scale, 1e-300)).max() / EPS)
        assert np.array_equal(bits(np.ascontiguousarray(r.x[i][:, 1])), bits(r.mean[i]))      # q = 1/2: z = 0 exactly
    print(f"[series-sum] quantiles against their own marginals: worst {worst:.2f} eps")


@pytest.mark.parametrize("M", [1, 3])
def test_other_component_counts(pkg, engine, M):
    G = pkg
    ts, xs = G.prior.synthetic_series(256, seed=317, shuffle=True)
    n, m = 17, 6
    tq = R.RP.queries_for(ts, ts[:n], m)
    series, queries = [(ts[:n].copy(), xs[:n].copy())], [tq]
    parts = [G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Periodic(0.5, 0.1, 0.8) + G.WhiteNoise(0.1), 0.45, 0.05),
             G.Linear(0.3, 0.2, 0.7) * G.SquaredExponential(0.25, 0.8) + G.Constant(0.1), G.GammaExponential(0.4, 1.3, 0.6)]
    splits = [tuple(parts[:M]), tuple(parts[::-1][:M])]
    noises = np.array([0.1, 0.05])
    yts = np.array([(-0.8, 0.4)])
    r = run(engine, series, queries, splits, noises, [0, 0], yts, noise_pred=np.array([0.3, 0.0]))
    assert [len(a) for a in r.mean] == [(M + 1) * m] * 2
    check_against_oracle(f"M = {M}", r, series, queries, splits, noises, [0, 0], yts, noise_pred=[0.3, 0.0])


def test_evaluator_coverage(pkg, engine, golden):
    G = pkg
    cases = [c for c in golden["cases"] if "logpdf" in c and len(c["ts"]) <= G.SERIES_MAX_N]
    assert len(cases) >= 20
    series = [(np.array(c["ts"]), np.array(c["xs"])) for c in cases]
    leaf = (G.Periodic, G.Linear, G.SquaredExponential, G.GammaExponential, G.WhiteNoise, G.Constant)
    splits = [G.split_kernel_sop(G.from_tuple(to_tuple(c["tree"])), leaf[k % 6]) for k, c in enumerate(cases)]
    noises = np.array([c["noise"] for c in cases])
    queries = []
    for ts, _ in series:                                         # 7 queries (21 rows: two blocks): before, inside (one ON a training time), past
        lo, hi = ts.min(), ts.max()
        v = np.linspace(lo - 0.1 * (hi - lo + 1.0), hi + 0.3 * (hi - lo + 1.0), 7)
        v[3] = ts[len(ts) // 2]
        queries.append(v)
    sidx = np.arange(len(cases), dtype=np.int32)
    r = run(engine, series, queries, splits, noises, sidx)       # ONE ragged call, each case its own series
    check_against_oracle("golden", r, series, queries, splits, noises, sidx)
    # hand-written parts on a series with a repeated training time; the deep tree takes the D = 8 instantiation
    rng = np.random.default_rng(5)
    ts = rng.random(70); ts[41] = ts[7]
    xs = 0.5 * rng.standard_normal(70)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = TS.full_tree(G, 4)
    assert deep.size() == 31
    v = np.array([0.05, 0.31, 0.61, ts[7], ts[7], 1.2, -0.2])
    splits = [(nested, G.GammaExponential(0.42, 0.58, 3.2)), (deep, G.SquaredExponential(0.3, 0.5)),
              (G.Constant(0.5) * G.WhiteNoise(0.3), nested)]
    noises = np.array([0.1, 0.2, 0.05])
    r = run(engine, [(ts, xs)], [v], splits, noises, [0, 0, 0])
    check_against_oracle("hand-written", r, [(ts, xs)], [v], splits, noises, [0, 0, 0])
    # the longest ChangePoint chain that fits beside two selectors at the cap
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N, seed=4)
    v = np.linspace(-0.1, 1.3, 7); v[5] = ts[11]
    fit = max(k for k in range(1, 40) if R.series_sum_lds_bytes(N, [TS.cp_chain(G, k).to_tuple(), ("C", 1.0)]) <= R.R.LDS_BYTES)
    assert fit == 8
    splits = [(TS.cp_chain(G, fit), G.Constant(0.25))]
    r = run(engine, [(ts, xs)], [v], splits, [0.1], [0])
    check_against_oracle("ChangePoint chain at the cap", r, [(ts, xs)], [v], splits, [0.1], [0])


def test_agrees_with_resident_route(engine, ragged):
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    for s in (4, 6, 7):                                          # 17, 126 and 144 points
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        mean_r, x_r, info_r = engine.predict_sum_batch([splits[i] for i in sel], noises[sel], queries[s], q=R.Q, y_transform=tuple(yts[s]),
                                                       check=False)
        assert (np.asarray(info_r) == 0).all()
        for k, i in enumerate(sel):
            assert close(r.mean[i], mean_r[k]) and close(r.x[i], x_r[k]), (s, i)


def test_batch_independence_bitwise(engine, ragged):
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    P = len(splits)
    rev = np.arange(P)[::-1]
    r_rev = run(engine, series, queries, [splits[i] for i in rev], noises[rev], sidx[rev], yts)
    assert np.array_equal(sbits(r_rev), sbits(take(r, rev)))
    for s in range(len(series)):                                 # one series at a time
        sel = np.flatnonzero(sidx == s)
        one = run(engine, [series[s]], [queries[s]], [splits[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32), yts[s:s + 1])
        assert np.array_equal(sbits(one), sbits(take(r, sel))), s
    for p in range(P):                                           # each particle alone
        s = sidx[p]
        one = run(engine, [series[s]], [queries[s]], [splits[p]], noises[p:p + 1], [0], yts[s:s + 1])
        assert np.array_equal(sbits(one), sbits(take(r, [p]))), p


def test_stateless(pkg, ragged):
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    eng = pkg.GPEngine(0)
    try:
        r0 = run(eng, series, queries, splits, noises, sidx, yts)      # a fresh engine on which set_data was never called
        assert np.array_equal(sbits(r0), sbits(r))
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)      # (with copies: dedup counts them)
        tq = np.linspace(1.0, 1.2, 7)
        sum0 = eng.predict_sum_batch([pkg.split_kernel_sop(nd, pkg.Periodic) for nd in rn], rz, tq, q=R.Q, check=False)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max,
                    eng.predict_reuse_stats())
        before = snapshot()
        r1 = run(eng, series, queries, splits, noises, sidx, yts)
        assert np.array_equal(sbits(r1), sbits(r))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        sum1 = eng.predict_sum_batch([pkg.split_kernel_sop(nd, pkg.Periodic) for nd in rn], rz, tq, q=R.Q, check=False)
        assert np.array_equal(bits(sum1[0]), bits(sum0[0])) and np.array_equal(bits(sum1[1]), bits(sum0[1]))
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)      # the store still holds its factors: a longer prefix extends them
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_concurrent_callers(engine, ragged):
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    out = [None] * 4

    def work(i):
        out[i] = run(engine, series, queries, splits, noises, sidx, yts)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for o in out:
        assert o is not None and np.array_equal(sbits(o), sbits(r))


def test_non_positive_definite(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(40, seed=2)
    v = np.linspace(1.0, 1.5, 7)
    bad = (G.Constant(0.75), G.Constant(0.25))                   # K = 1 everywhere, noise -0.5: the second leading minor fails
    good = (G.SquaredExponential(0.3, 0.8), G.Constant(0.1))
    good2 = (G.Periodic(0.7, 0.3, 0.9), G.Linear(0.2, 0.3, 0.4))
    first = S.first_bad_minor(O.compute_cov_matrix_vectorized(("C", 1.0), -0.5, ts))
    assert first == 2
    r = run(engine, [(ts, xs)], [v], [good, bad, good2], np.array([0.1, -0.5, 0.2]), [0, 0, 0])
    assert r.info.tolist() == [0, first, 0]
    assert r.mean[1].shape == (21,) and np.isnan(r.mean[1]).all() and np.isnan(r.var[1]).all() and np.isnan(r.x[1]).all()
    assert np.isnan(r.logpdf[1])
    for i, (sp, nz) in ((0, (good, 0.1)), (2, (good2, 0.2))):
        alone = run(engine, [(ts, xs)], [v], [sp], np.array([nz]), [0])
        assert alone.info[0] == 0 and np.array_equal(sbits(alone), sbits(take(r, [i])))
    check_against_oracle("beside a failed particle", take(r, [0, 2]), [(ts, xs)], [v], [good, good2], [0.1, 0.2], [0, 0])
    with pytest.raises(G.PosDefException) as ei:
        engine.predict_sum_series_batch([(ts, xs), (ts, xs)], [v, v], [good, bad], [0.1, -0.5], [0, 1])
    assert ei.value.particle == 1 and ei.value.info == first


def test_row_level_info(pkg, engine):
    """a transform under which the raw means of F_2 and X overflow and those of F_1 do not: info = n + m + 1 (the first F_2 row: rows
    of three codes share block 0, and the blocks of other waves fail too), NaN in that particle's blocks alone"""
    G = pkg
    n, m = 17, 6
    ts, _ = G.prior.synthetic_series(64, seed=8, shuffle=True)
    ts = ts[:n].copy()
    xs = 1e9 + np.sin(7.0 * ts)                                  # a level only the Constant part explains
    v = R.RP.queries_for(np.linspace(0, 1, 5), ts, m)
    sp = (G.SquaredExponential(0.3, 1e-6), G.Constant(1.0))
    yt_bad, yt_ok = (1e-300, 0.0), (1.0, 0.0)
    want = R.series_sum_rows([c.to_tuple() for c in sp], 0.1, ts, xs, v, y_transform=yt_bad, q=R.Q)
    assert want[3] == n + m + 1                                  # the restated rule
    r = run(engine, [(ts, xs), (ts, xs)], [v, v], [sp, sp, sp], np.array([0.1, 0.1, 0.1]), [1, 0, 1], np.array([yt_bad, yt_ok]))
    assert r.info.tolist() == [0, n + m + 1, 0]
    assert np.isnan(r.mean[1]).all() and np.isnan(r.var[1]).all() and np.isnan(r.x[1]).all() and r.mean[1].shape == (3 * m,)
    assert np.isfinite(r.logpdf).all()                           # the factor itself is fine
    alone = run(engine, [(ts, xs)], [v], [sp], np.array([0.1]), [0], np.array([yt_ok]))
    for i in (0, 2):
        assert np.array_equal(sbits(alone), sbits(take(r, [i])))
    check_against_oracle("beside a failed row", alone, [(ts, xs)], [v], [sp], [0.1], [0])
    # an empty series reports the row of its prior the same way: n = 0, every raw mean overflows from row 0 on
    e = run(engine, [(ts[:0], xs[:0])], [v], [sp], np.array([0.1]), [0], np.array([(1e-308, 1e300)]))
    assert e.info.tolist() == [1] and np.isnan(e.mean[0]).all() and e.logpdf[0] == 0.0
    with pytest.raises(G.PosDefException) as ei:
        engine.predict_sum_series_batch([(ts, xs)], [v], [sp], [0.1], [0], y_transforms=[yt_bad])
    assert ei.value.info == n + m + 1


def test_errors_name_the_culprit(pkg, engine):
    G = pkg
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    v = np.linspace(1.0, 1.3, 5)
    good = (G.SquaredExponential(0.3, 0.8), G.Constant(0.1))
    s20, s9 = (ts[:20], xs[:20]), (ts[:9], xs[:9])
    ref = R.oracle_rows([c.to_tuple() for c in good], 0.1, *s20, v, q=R.Q)

    def valid():
        r = run(engine, [s20], [v], [good], np.array([0.1]), [0])
        assert r.info[0] == 0 and close(r.mean[0], ref[0]) and close(r.var[0], ref[1]) and close(r.x[0], ref[2])

    def refused(out, code, *words):
        rc, msg, off, mean, var, x, lp, info = out
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert (mean == SENTINEL).all() and (var == SENTINEL).all() and (x == SENTINEL).all() and (off == -1).all()
        assert (lp == SENTINEL).all() and (info == 7).all()
        valid()

    two = dict(series=[s20, s9], queries=[v, v], sidx=[0, 1], splits=[good, good], noises=[0.1, 0.1])
    call = lambda **kw: raw_call(engine, G, **{**two, **kw})
    # everything the predictive entry lists
    refused(call(q_off=[1, 5, 10]), -1, "q_off[0]")
    refused(call(q_off=[0, 5, 3]), -1, "series 1", "q_off decreases")
    for name in ("q_off", "ts_pred", "out_mean", "out_off", "out_info", "op_off", "out_x"):
        refused(call(null=(name,)), -1, "null pointer")
    refused(call(sidx=[0, 3]), -1, "particle 1", "series index 3")
    refused(call(series=[(ts[:5], xs[:5]), (ts, xs)]), -1, "series 1", str(N + 1))
    refused(call(pt_off=[0, 30, 20]), -1, "series 1", "pt_off decreases")
    # the components
    refused(call(M=0), -1, "M must be")
    op_off, ops, prm_off, prm = G.encode_batch([c for sp in two["splits"] for c in sp])
    bad_off = op_off.copy(); bad_off[3] = bad_off[2] - 1
    refused(call(programs=(bad_off, ops, prm_off, prm)), -1, "particle 1", "component 1")
    lone_plus = (np.array([0, 1, 2, 3, 4], dtype=np.int32), np.array([3, 1, 6, 1], dtype=np.uint8), np.array([0, 2, 3, 3, 4], dtype=np.int32),
                 np.array([0.3, 0.8, 0.1, 0.1]))
    refused(call(programs=lone_plus), -3, "particle 1", "underflow")
    # a composite over AGP_MAX_OPS nodes: two components of 127 nodes each (a chain of 63 ChangePoints) + 2 selectors + 3 operators
    big = TS.cp_chain(G, 63)
    assert big.size() == 127
    refused(call(splits=[good, (big, big)]), -3, "particle 1", "AGP_MAX_OPS")
    # tables that do not fit at the series' length: one ChangePoint more than fits beside the two selectors at the cap
    sN, s100 = (ts[:N], xs[:N]), (ts[:100], xs[:100])
    too_many = (TS.cp_chain(G, 9), G.Constant(0.25))
    refused(call(series=[s20, sN], splits=[good, too_many]), -3, "particle 1", "LDS", "selectors")
    r = run(engine, [s100], [v], [too_many], np.array([0.1]), [0])      # ... and fits a 100-point series
    check_against_oracle("nine ChangePoints at 100 points", r, [s100], [v], [too_many], [0.1], [0])
    # the read-out's arguments
    refused(call(q=[0.5, 1.0]), -1, "quantile 1", "(0, 1)")
    refused(call(q=[np.nan]), -1, "quantile 0")
    refused(call(nq=-1), -1, "negative")
    refused(call(slope=[1.0, 0.0], icpt=[0.0, 0.0]), -1, "series 1", "slope")
    refused(call(slope=[np.inf, 1.0], icpt=[0.0, 0.0]), -1, "series 0", "slope")
    refused(call(slope=[1.0, 1.0], icpt=[0.0, np.nan]), -1, "series 1", "intercept")
    # an output of 2^31 elements: 2^30 queries x (M + 1) rows (the query array is never read: the sizes are refused first)
    refused(call(q_off=[0, 5, 5 + (1 << 30)], sidx=[1, 1]), -1, "2^31")
    # out_var and out_logpdf may be NULL, and nq == 0 needs no out_x
    rc, msg, off, mean, var, x, lp, info = call(null=("out_var", "out_logpdf", "out_x"), q=[], nq=0)
    assert rc == 0 and (var == SENTINEL).all() and (lp == SENTINEL).all() and (x == SENTINEL).all() and off.tolist() == [0, 15, 30]
    assert close(mean[:15], ref[0]) and info.tolist() == [0, 0]
    # P == 0 touches nothing
    rc, msg, off, mean, var, x, lp, info = raw_call(engine, G, [s20], [v], np.zeros(0, dtype=np.int32), [], np.zeros(0),
                                                    programs=(np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint8),
                                                              np.zeros(1, dtype=np.int32), np.zeros(1)))
    assert rc == 0 and (mean == SENTINEL).all() and (off == -1).all()
    valid()


def test_chains_into_mixture_quantile(engine, ragged):
    """the (P_s, (M + 1) m_s) block of one series' adjacent particles goes to mixture_quantile as it is"""
    series, queries, splits, noises, sidx, yts, refs, r = ragged
    s = 7                                                        # 144 points, 12 queries
    sel = np.flatnonzero(sidx == s)
    assert len(sel) == 6 and (np.diff(sel) == 1).all()
    w = np.array([0.3, 0.1, 0.2, 0.15, 0.05, 0.2])
    qs = np.array([0.025, 0.5, 0.975])
    bm, bv = np.stack([r.mean[i] for i in sel]), np.stack([r.var[i] for i in sel])
    assert bm.shape == (6, 36)
    x, conv, _ = engine.mixture_quantile(bm, bv, w, qs, tol=1e-10)
    assert np.asarray(conv).all() and x.shape == (36, 3)
    span = np.abs(bm).max() + 10.0 * np.sqrt(bv.max())
    for row in (0, 11, 12, 23, 24, 35):                          # first and last row of F_1, F_2 and X
        for k, qv in enumerate(qs):
            want = R.mixture_quantile(bm[:, row], np.sqrt(bv[:, row]), w, qv, lo=-span, hi=span)
            assert abs(x[row, k] - want) <= 1e-8 * max(1.0, abs(want)), (row, k)
