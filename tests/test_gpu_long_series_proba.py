"""GPU tests of agp_predict_logpdf_long_series_batch (held-out scores of series of up to 512 JOINT points in one call;
k_long_series_predict_logpdf, csrc/agp_long_series_kernel.hpp, and the mixture read-out k_series_mix_logp): parity with the reference
restatement of the predictive log-density (tests/_pred_logpdf_ref.py) on one ragged call under both routings, the short routing and the
prior case bit for bit, cross-checks against differences of the long value entry and against the resident-series entry, the
per-point terms, the mixtures, the info rule on the joint index, batch and split independence (bitwise), refusals through the raw
entry, statelessness and concurrent callers.
Tolerance of every comparison with a reference or another route: |lp - ref| <= 1e-8 S per particle, S the sum of the magnitudes of
the terms the log-density is made of (tests/_pred_logpdf_ref.reference) — the tolerance and scale tests/test_gpu_series_proba.py and
tests/test_gpu_predict_logpdf.py use for the same quantity.  Up to n + m = 300 the mpmath / 80-bit arbiter decides a miss; above it
there is no arbiter and the fp64 reference decides.  Sums of the entry's own numbers in another order: 1e-12 S.  No particle is
skipped anywhere: the fp64 reference factors every particle of every case (asserted), unless the test is about failure.
Measured on one MI355X: worst |lp - ref| / S of the ragged case 8.3e-15 under either routing, 5.1e-15 against differences of the long
value entry, 1.1e-15 against the resident path (profiles/long_series_proba_perf.txt)."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import _long_series_proba_ref as LR
import _pred_logpdf_ref as PR
import _series_proba_ref as SPR
import test_gpu_long_series as TL
import test_gpu_series_proba as TP
from oracle import oracle as O

pytestmark = pytest.mark.gpu
bits = TL.bits
sbits, pbits, uniform_weights, lse = TP.sbits, TP.pbits, TP.uniform_weights, TP.lse
TOL = 1e-8
SENTINEL = 7.25
WS_512 = 8 * 256 * 528      # bytes of one 512-point workgroup's workspace


def scores(engine, series, qs, held, nodes, noises, sidx, **kw):
    kw.setdefault("check", False)
    return engine.predict_logpdf_long_series_batch(series, qs, held, nodes, noises, sidx, **kw)


def freeze(sc):
    for a in (sc.logpdf, sc.info, *([] if sc.series_logp is None else [sc.series_logp]), *([] if sc.terms is None else sc.terms)):
        a.setflags(write=False)
    return sc


@pytest.fixture(scope="module")
def ragged(engine):
    """tests/_long_series_proba_ref.ragged_case() through the entry under both routings, once, with the per-particle noise_pred,
    terms and uniform mixtures"""
    series, qs, held, nodes, noises, sidx, noise_pred = LR.ragged_case()
    w = uniform_weights(sidx)
    res = {flag: freeze(scores(engine, series, qs, held, nodes, noises, sidx, weights=w, noise_pred=noise_pred, want_terms=True,
                               all_long=flag)) for flag in (False, True)}
    return series, qs, held, nodes, noises, sidx, noise_pred, w, res


def take(series, qs, held, nodes, noises, sidx, sel, *more):
    """the sub-batch of the particles sel on the series they name, renumbered: (series, qs, held, nodes, noises, sidx, *more[sel])"""
    sel = np.asarray(sel)
    used = sorted(set(int(s) for s in sidx[sel]))
    renum = {s: i for i, s in enumerate(used)}
    return ([series[s] for s in used], [qs[s] for s in used], [held[s] for s in used], [nodes[i] for i in sel], noises[sel],
            np.array([renum[int(s)] for s in sidx[sel]], dtype=np.int32), *[m[sel] for m in more])


def test_ragged_parity_both_routings(ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    refs = LR.ragged_references()
    assert tuple((len(t), len(q)) for (t, _), q in zip(series, qs)) == LR.SHAPES and len(refs) == len(nodes) == 72
    for flag in (False, True):
        sc = res[flag]
        assert (sc.info == 0).all(), (flag, sc.info)
        assert [len(t) for t in sc.terms] == [len(qs[s]) for s in sidx]
        worst, n_checked = 0.0, 0
        for p, nd in enumerate(nodes):
            s = int(sidx[p])
            ref, S = refs[p]
            if len(qs[s]) == 0:                                  # nothing held out: 0, info 0, an empty block
                assert sc.logpdf[p] == 0.0 and sc.terms[p].size == 0
                n_checked += 1
                continue
            assert math.isfinite(ref) and S > 0.0
            ratio = abs(sc.logpdf[p] - ref) / S
            worst = max(worst, ratio)
            if not ratio <= TOL:                                 # a miss: the arbiter decides where there is one (n + m <= 300)
                PR.assert_close(float(sc.logpdf[p]), nd.to_tuple(), float(noises[p]), *series[s], qs[s], held[s], tol=TOL,
                                ctx=("ragged", flag, p, LR.SHAPES[s]), noise_pred=float(noise_pred[p]))
            n_checked += 1
        assert n_checked == len(nodes)                           # none is skipped
        print(f"[long-series-proba] ragged, all_long={flag}: worst |lp - ref| / S = {worst:.3e} over {len(nodes)} particles")
    # the two routings differ in arithmetic, not in what they compute
    for p in range(len(nodes)):
        assert abs(res[True].logpdf[p] - res[False].logpdf[p]) <= TOL * max(refs[p][1], 1e-300), p
    # above the short cap, and where nothing is held out, the flag changes nothing
    same = [p for p in range(len(nodes)) if sum(LR.SHAPES[sidx[p]]) > LR.N_SHORT or LR.SHAPES[sidx[p]][1] == 0]
    assert len(same) == 3 * 16 and np.array_equal(pbits(res[True], same), pbits(res[False], same))


def test_short_routing_is_bitwise(engine, ragged):
    """N = n_s + m_s <= AGP_SERIES_MAX_N: the launch is agp_predict_logpdf_series_batch's, and so are logpdf, terms, mixtures and info"""
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    short = np.flatnonzero(np.array([sum(LR.SHAPES[s]) <= LR.N_SHORT for s in sidx]))
    assert len(short) == 3 * 9 and (175, 1) in [LR.SHAPES[s] for s in sidx[short]]
    sub = take(series, qs, held, nodes, noises, sidx, short, w, noise_pred)
    ref = engine.predict_logpdf_series_batch(*sub[:6], weights=sub[6], noise_pred=sub[7], want_terms=True, check=False)
    assert np.array_equal(pbits(ref, range(len(short))), pbits(res[False], short))
    used = sorted(set(int(s) for s in sidx[short]))
    assert np.array_equal(bits(ref.series_logp), bits(res[False].series_logp[used]))
    # the same sub-batch through the long entry alone: the short classes' launches only
    alone = scores(engine, *sub[:6], weights=sub[6], noise_pred=sub[7], want_terms=True)
    assert np.array_equal(sbits(alone), sbits(ref))


def test_prior_case_is_bitwise(engine, ragged):
    """n_s = 0, y_slope NULL, noise_pred NULL: every row is a query row and out_logpdf is agp_logpdf_long_series_batch's on (tq, y)"""
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    for shape, flag in (((0, 177), False), ((0, 512), False), ((0, 512), True), ((0, 5), True)):
        s = LR.SHAPES.index(shape)
        sel = np.flatnonzero(sidx == s)
        nd, nz = [nodes[i] for i in sel], noises[sel]
        zeros = np.zeros(len(sel), dtype=np.int32)
        got = scores(engine, [series[s]], [qs[s]], [held[s]], nd, nz, zeros, all_long=flag, want_terms=True)
        lv, iv = engine.logpdf_long_series_batch([(qs[s], held[s])], nd, nz, zeros, all_long=flag, check=False)
        assert (got.info == 0).all() and (iv == 0).all()
        assert np.array_equal(bits(got.logpdf), bits(lv)), (shape, flag, got.logpdf, lv)
        # an explicit noise_pred equal to the noise and slopes of 1 are the same call
        same = scores(engine, [series[s]], [qs[s]], [held[s]], nd, nz, zeros, all_long=flag, want_terms=True, noise_pred=nz.copy(),
                      y_transforms=[(1.0, 0.0)])
        assert np.array_equal(sbits(same), sbits(got))


def test_agrees_with_differences_of_the_long_value_entry(engine, ragged):
    """noise_pred = noise, slope 1: log p(held-out | training) = logpdf_long(training ++ held-out) - logpdf_long(training);
    S = the sum of the magnitudes of both values"""
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    joint = [(np.concatenate([t, q]), np.concatenate([x, y])) for (t, x), q, y in zip(series, qs, held)]
    for flag in (False, True):
        sc = scores(engine, series, qs, held, nodes, noises, sidx, all_long=flag)
        lj, ij = engine.logpdf_long_series_batch(joint, nodes, noises, sidx, all_long=flag, check=False)
        lt, it = engine.logpdf_long_series_batch(series, nodes, noises, sidx, all_long=flag, check=False)
        assert (ij == 0).all() and (it == 0).all() and (sc.info == 0).all()
        worst = 0.0
        for p in range(len(nodes)):
            S = abs(lj[p]) + abs(lt[p])
            worst = max(worst, abs(sc.logpdf[p] - (lj[p] - lt[p])) / max(S, 1e-300))
            assert abs(sc.logpdf[p] - (lj[p] - lt[p])) <= TOL * max(S, 1e-300), (flag, p, sc.logpdf[p], lj[p] - lt[p])
        print(f"[long-series-proba] against differences of the value entry, all_long={flag}: worst |d| / S = {worst:.3e}")


def test_agrees_with_resident_series_path(engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    refs = LR.ragged_references()
    worst = 0.0
    for shape in ((144, 36), (442, 70)):
        s = LR.SHAPES.index(shape)
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        lp_r, info_r = engine.predict_logpdf_batch([nodes[i] for i in sel], noises[sel], qs[s], held[s], noise_pred=noise_pred[sel],
                                                   check=False)
        assert (np.asarray(info_r) == 0).all()
        for k, i in enumerate(sel):
            worst = max(worst, abs(res[False].logpdf[i] - lp_r[k]) / refs[i][1])
            assert abs(res[False].logpdf[i] - lp_r[k]) <= TOL * refs[i][1], (shape, i)
    print(f"[long-series-proba] against set_data + predict_logpdf_batch: worst |d| / S = {worst:.3e}")


def test_terms(pkg, engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    refs = LR.ragged_references()
    for flag, sc in res.items():
        for p in range(len(nodes)):
            if sc.terms[p].size:
                assert abs(sc.terms[p].sum() - sc.logpdf[p]) <= 1e-12 * refs[p][1], (flag, p)
    # the partial sums are the entry's own scores of the first j held-out points: a (160, 40) split, whose truncations end on both
    # sides of the short cap (joint lengths 175 .. 177) and of the block boundary at joint position 192, the first and the last point
    n, m = 160, 40
    ts, xs = pkg.prior.synthetic_series(256, seed=8, shuffle=True)
    rng = np.random.default_rng(2)
    tq = rng.random(m); y = 0.5 * rng.standard_normal(m)
    nd = SPR.fixture_kernels(pkg)[2:]
    nz = np.full(len(nd), 0.15)
    train = (ts[:n].copy(), xs[:n].copy())
    js = (1, 15, 16, 17, 31, 32, 33, 40)
    S = {(j, k): PR.reference(nd[k].to_tuple(), 0.15, *train, tq[:j], y[:j], noise_pred=0.05)[1] for j in js for k in range(len(nd))}
    for flag in (False, True):
        full = scores(engine, [train], [tq], [y], nd, nz, np.zeros(len(nd), dtype=np.int32), noise_pred=0.05, want_terms=True,
                      all_long=flag, check=True)
        # ONE call: series j = the same training points with the first j held-out points
        many = scores(engine, [train] * len(js), [tq[:j] for j in js], [y[:j] for j in js], nd * len(js), np.tile(nz, len(js)),
                      np.repeat(np.arange(len(js)), len(nd)), noise_pred=0.05, all_long=flag, check=True)
        for a, j in enumerate(js):
            for k in range(len(nd)):
                assert abs(full.terms[k][:j].sum() - many.logpdf[a * len(nd) + k]) <= TOL * S[j, k], (flag, j, k)
        assert np.array_equal(bits(many.logpdf[-len(nd):]), bits(full.logpdf))


def test_mixture(pkg, engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    for flag, sc in res.items():
        for s in range(len(series)):
            sel = np.flatnonzero(sidx == s)
            if len(qs[s]) == 0:
                assert sc.series_logp[s] == 0.0 and not np.signbit(sc.series_logp[s])      # exactly 0.0
                continue
            ref = lse(sc.logpdf[sel], w[sel])
            assert abs(sc.series_logp[s] - ref) <= 1e-12 * max(1.0, abs(ref)), (flag, s)
    # k_series_mix_logp runs unchanged behind the launches: a short-routed series' mixture has the short entry's bits (the same
    # kernel fed the same logpdf; test_short_routing_is_bitwise), and a long series' bits are those of the series alone (below).
    # Particles of a series not adjacent, a zero weight, a series without particles, a transform on one series, nothing held out:
    G = pkg
    pick = [LR.SHAPES.index(x) for x in ((144, 36), (5, 0), (300, 37), (126, 18), (161, 16))]
    ser = [series[s] for s in pick]; q = [qs[s] for s in pick]; y = [held[s] for s in pick]
    nd = SPR.fixture_kernels(G)[2:7]
    mix_nodes = [nd[0], nd[1], nd[2], nd[3], nd[4], nd[0], nd[1], nd[2]]
    mix_sidx = np.array([0, 2, 0, 1, 2, 0, 1, 3], dtype=np.int32)       # series 4 has no particle
    mix_w = np.array([0.25, 0.4, 0.0, 0.5, 0.6, 0.75, 0.5, 1.0])
    nz = np.full(8, 0.1)
    yt = [(1.0, 0.0), (1.0, 0.0), (-2.5, 0.3), (1.0, 0.0), (1.0, 0.0)]
    raw = [y[0], y[1], (y[2] - 0.3) / -2.5, y[3], y[4]]                  # raw values whose scaled images are the ragged case's
    sc = scores(engine, ser, q, raw, mix_nodes, nz, mix_sidx, weights=mix_w, y_transforms=yt, check=True)
    plain = scores(engine, ser, q, y, mix_nodes, nz, mix_sidx, weights=mix_w, check=True)
    for s in (0, 2, 3):
        sel = np.flatnonzero(mix_sidx == s)
        ref = lse(sc.logpdf[sel], mix_w[sel])
        assert abs(sc.series_logp[s] - ref) <= 1e-12 * max(1.0, abs(ref)), s
    assert sc.series_logp[1] == 0.0 and not np.signbit(sc.series_logp[1]) and math.isnan(sc.series_logp[4])
    # the short-routed series of this call, through the short entry: the mixture's bits
    short = engine.predict_logpdf_series_batch([ser[3]], [q[3]], [y[3]], [mix_nodes[7]], nz[7:], [0], weights=mix_w[7:])
    assert np.array_equal(bits(short.series_logp), bits(plain.series_logp[3:4])) and np.array_equal(bits(short.logpdf), bits(plain.logpdf[7:]))
    # raw space: the transform adds m log|slope| to every particle of that series and to its mixture, and nothing elsewhere
    shift = len(q[2]) * math.log(2.5)
    for p in np.flatnonzero(mix_sidx == 2):
        want = plain.logpdf[p] + shift
        assert abs(sc.logpdf[p] - want) <= 1e-12 * (abs(plain.logpdf[p]) + shift), p
    assert abs(sc.series_logp[2] - (plain.series_logp[2] + shift)) <= 1e-12 * (abs(plain.series_logp[2]) + shift)
    other = np.flatnonzero(mix_sidx != 2)
    assert np.array_equal(bits(sc.logpdf[other]), bits(plain.logpdf[other]))
    assert np.array_equal(bits(sc.series_logp[[0, 1, 3]]), bits(plain.series_logp[[0, 1, 3]]))
    # a failed particle at weight 0 on a LONG series: NaN for ITS series only, the other series' bits unchanged
    bad_nodes = list(mix_nodes); bad_nz = nz.copy()
    bad_nodes[2] = G.Constant(1.0); bad_nz[2] = -0.5
    bad = scores(engine, ser, q, y, bad_nodes, bad_nz, mix_sidx, weights=mix_w)
    assert bad.info[2] > 0 and math.isnan(bad.logpdf[2]) and math.isnan(bad.series_logp[0])
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert np.array_equal(pbits(bad, keep), pbits(plain, keep))
    assert np.array_equal(bits(bad.series_logp[[1, 2, 3]]), bits(plain.series_logp[[1, 2, 3]])) and math.isnan(bad.series_logp[4])
    with pytest.raises(G.PosDefException):
        scores(engine, ser, q, y, bad_nodes, bad_nz, mix_sidx, weights=mix_w, check=True)


def test_info_is_the_first_bad_pivot_of_the_joint_factor(pkg, engine):
    ts, xs, tq, y, nodes, noises, at = LR.bad_pivot_case()      # (every position is asserted on the CPU with first_bad_minor there)
    P = len(nodes)
    zeros = np.zeros(P, dtype=np.int32)
    sc = scores(engine, [(ts, xs)], [tq], [y], nodes, noises, zeros, want_terms=True)
    assert sc.info.tolist() == [*LR.BAD_POSITIONS[:at], 0, *LR.BAD_POSITIONS[at:]], sc.info
    for p in range(P):
        assert sc.terms[p].shape == (len(tq),)
        if p != at:
            assert math.isnan(sc.logpdf[p]) and np.isnan(sc.terms[p]).all()
    alone = scores(engine, [(ts, xs)], [tq], [y], [nodes[at]], noises[at:at + 1], [0], want_terms=True, check=True)
    assert np.isfinite(alone.logpdf).all() and np.array_equal(pbits(alone, [0]), pbits(sc, [at]))
    PR.assert_close(float(sc.logpdf[at]), nodes[at].to_tuple(), float(noises[at]), ts, xs, tq, y, tol=TOL, ctx="beside failed particles")
    with pytest.raises(pkg.PosDefException) as ei:
        scores(engine, [(ts, xs)], [tq], [y], nodes, noises, zeros, check=True)
    assert ei.value.particle == 0 and ei.value.info == 1


def test_batch_and_split_independence_bitwise(engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    P = len(nodes)
    rev = np.arange(P)[::-1]
    for flag in (False, True):
        sc = res[flag]
        kw = dict(want_terms=True, all_long=flag)
        again = scores(engine, series, qs, held, nodes, noises, sidx, weights=w, noise_pred=noise_pred, **kw)      # the call repeated
        assert np.array_equal(sbits(again), sbits(sc)), flag
        r_rev = scores(engine, series, qs, held, [nodes[i] for i in rev], noises[rev], sidx[rev], weights=w[rev], noise_pred=noise_pred[rev], **kw)
        assert np.array_equal(pbits(r_rev, range(P)), pbits(sc, rev)), flag
        # (uniform weights, reversed order inside each mixture: the same set of numbers summed in another order)
        both = np.isfinite(sc.series_logp)
        assert np.array_equal(both, np.isfinite(r_rev.series_logp))
        assert (np.abs(r_rev.series_logp[both] - sc.series_logp[both]) <= 1e-12 * np.maximum(1.0, np.abs(sc.series_logp[both]))).all()
        for s in range(len(series)):                             # one series per call: its particles' bits and its mixture's
            sel = np.flatnonzero(sidx == s)
            one = scores(engine, [series[s]], [qs[s]], [held[s]], [nodes[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32),
                         weights=w[sel], noise_pred=noise_pred[sel], **kw)
            assert np.array_equal(pbits(one, range(len(sel))), pbits(sc, sel)), (flag, s)
            assert np.array_equal(bits(one.series_logp), bits(sc.series_logp[s:s + 1])), (flag, s)
        if not flag:
            for p in range(P):                                   # each particle alone
                s = sidx[p]
                one = scores(engine, [series[s]], [qs[s]], [held[s]], [nodes[p]], noises[p:p + 1], [0], noise_pred=noise_pred[p:p + 1],
                             want_terms=True)
                assert np.array_equal(pbits(one, [0]), pbits(sc, [p])), p
        # a workspace limit that admits two but not three 512-point workgroups per launch: several launches
        limit = 3 << 20
        assert 2 * WS_512 <= limit < 3 * WS_512
        engine.set_workspace_limit(limit)
        try:
            split = scores(engine, series, qs, held, nodes, noises, sidx, weights=w, noise_pred=noise_pred, **kw)
        finally:
            engine.set_workspace_limit(0)
        assert np.array_equal(sbits(split), sbits(sc)), flag


def raw_call(engine, series, qs, held, sidx, programs, noises, flags=0, weights=None, y_slope=None, null=(), mix=None):
    """the C entry itself with sentinel-filled outputs: (rc, msg, logpdf, terms, out_off, series_logp, info); out_series_logp is
    passed exactly when weights are, unless `mix` says otherwise"""
    op_off, ops, prm_off, prm = programs
    P = len(noises)
    S = len(series)
    pt_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(t) for t, _ in series])]), dtype=np.int64)
    q_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(q) for q in qs])]), dtype=np.int64)
    sidx = np.ascontiguousarray(sidx, dtype=np.int32)
    f = lambda parts: np.ascontiguousarray(np.concatenate(list(parts) + [np.zeros(1)]), dtype=np.float64)      # noqa: E731
    ts, xs, tq, yq = f(t for t, _ in series), f(x for _, x in series), f(qs), f(held)
    noises = np.ascontiguousarray(noises, dtype=np.float64)
    total = int(sum(len(qs[s]) for s in sidx if 0 <= s < len(qs)))
    lp = np.full(P + 1, SENTINEL); terms = np.full(total + 16, SENTINEL); mixo = np.full(S + 1, SENTINEL)
    off = np.full(P + 1, -1, dtype=np.int64); info = np.full(P + 1, 7, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    sl = None if y_slope is None else np.ascontiguousarray(y_slope, dtype=np.float64)
    dp, ip, lp_ = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    arg = lambda name, a, t: None if (name in null or a is None) else a.ctypes.data_as(t)      # noqa: E731
    rc = engine._lib.agp_predict_logpdf_long_series_batch(
        engine._ctx, S, pt_off.ctypes.data_as(lp_), ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), arg("q_off", q_off, lp_),
        arg("ts_pred", tq, dp), arg("y_pred", yq, dp), P, sidx.ctypes.data_as(ip), op_off.ctypes.data_as(ip),
        ops.ctypes.data_as(C.POINTER(C.c_uint8)), prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp), None,
        arg("y_slope", sl, dp), arg("weights", w, dp), arg("out_logpdf", lp, dp), arg("out_terms", terms, dp), arg("out_off", off, lp_),
        arg("out_series_logp", mixo if ((w is not None) if mix is None else mix) else None, dp), arg("out_info", info, ip), flags)
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), lp, terms, off, mixo, info


def untouched(out):
    rc, msg, lp, terms, off, mixo, info = out
    return bool((lp == SENTINEL).all() and (terms == SENTINEL).all() and (off == -1).all() and (mixo == SENTINEL).all()
                and (info == 7).all())


def test_refusals_leave_outputs_untouched(pkg, engine):
    G = pkg
    N = G.LONG_SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    q = np.linspace(1.0, 1.3, 9); y = np.linspace(-0.4, 0.4, 9)
    good = G.SquaredExponential(0.3, 0.8)
    progs = G.encode_batch([good, good])
    s200, s9 = (ts[:200], xs[:200]), (ts[:9], xs[:9])
    ref200, S200 = PR.reference(good.to_tuple(), 0.1, *s200, q, y)

    def valid():
        sc = scores(engine, [s200], [q], [y], [good], [0.1], [0], check=True)
        assert sc.info[0] == 0 and abs(sc.logpdf[0] - ref200) <= TOL * S200

    two = ([s200, s9], [q, q], [y, y], [0, 1], progs, [0.1, 0.1])
    # the call as it is: valid, and the sentinels behind the outputs stay
    out = raw_call(engine, *two, weights=[1.0, 1.0])
    assert out[0] == 0 and out[2][2] == SENTINEL and out[3][18] == SENTINEL and out[5][2] == SENTINEL and out[4].tolist() == [0, 9, 18]
    assert abs(out[2][0] - ref200) <= TOL * S200 and out[5][0] == out[2][0] and out[5][1] == out[2][1]      # one particle at weight 1
    # N = 513: both counts and the constant in the message
    sbig = (ts[:N - 8], xs[:N - 8])
    out = raw_call(engine, [s9, sbig], [q, q], [y, y], [0, 1], progs, [0.1, 0.1])
    assert out[0] == -1 and "series 1" in out[1] and f" {N - 8} " in out[1] and " 9 " in out[1] and "AGP_LONG_SERIES_MAX_N" in out[1] \
        and "(512)" in out[1] and untouched(out), out[1]
    out = raw_call(engine, [s9, sbig], [q, q[:8]], [y, y[:8]], [0, 1], progs, [0.1, 0.1])      # exactly the cap
    assert out[0] == 0 and (out[6][:2] == 0).all() and np.isfinite(out[2][:2]).all()
    out = raw_call(engine, [s9, (ts[:N], xs[:N])], [q, q[:0]], [y, y[:0]], [0, 1], progs, [0.1, 0.1])      # nothing held out: no joint limit
    assert out[0] == 0 and out[2][1] == 0.0
    out = raw_call(engine, [s9, (ts, xs)], [q, q[:0]], [y, y[:0]], [0, 1], progs, [0.1, 0.1])             # 513 training points
    assert out[0] == -1 and "series 1" in out[1] and str(N + 1) in out[1] and "AGP_LONG_SERIES_MAX_N" in out[1] and untouched(out)
    with pytest.raises(ValueError, match="series 0 has 504 training and 9 held-out points"):
        scores(engine, [sbig], [q], [y], [good], [0.1], [0])
    # unknown flag bits
    for flags in (2, 1 | 4, 0x80000000):
        out = raw_call(engine, *two, flags=flags)
        assert out[0] == -1 and "flag" in out[1] and untouched(out), (flags, out[1])
    valid()
    # a held-out value that is not finite
    for badv in (math.nan, math.inf):
        yb = y.copy(); yb[4] = badv
        out = raw_call(engine, [s200, s9], [q, q], [y, yb], [0, 1], progs, [0.1, 0.1])
        assert out[0] == -1 and "series 1" in out[1] and "not finite" in out[1] and untouched(out)
    out = raw_call(engine, *two, null=("y_pred",))
    assert out[0] == -1 and "y_pred" in out[1] and untouched(out)
    # the slopes
    for badv in (0.0, math.nan, -math.inf):
        out = raw_call(engine, *two, y_slope=[1.0, badv])
        assert out[0] == -1 and "series 1" in out[1] and "slope" in out[1] and untouched(out)
    # the weights, per series
    for wts, what in (([1.0, math.nan], "finite"), ([1.0, -1.0], ">= 0"), ([1.0, 0.5], "sum to 1")):
        out = raw_call(engine, *two, weights=wts)
        assert out[0] == -1 and "series 1" in out[1] and what in out[1] and untouched(out)
    out = raw_call(engine, *two, weights=[1.0, 1.0], mix=False)
    assert out[0] == -1 and "out_series_logp" in out[1] and untouched(out)
    for name in ("q_off", "ts_pred", "out_logpdf", "out_info"):
        out = raw_call(engine, *two, null=(name,))
        assert out[0] == -1 and "null pointer" in out[1] and untouched(out), name
    valid()
    # LDS, counted from the kernel's own map at N = 512 joint points: the longest ChangePoint chain that fits scores, one more is refused
    n, m = N - 9, 9
    k_fit = max(k for k in range(1, 60) if LR.cp_chain_fits(k, n, m))
    assert k_fit == 34
    sN = (ts[:n], xs[:n])
    fits, too_many = TL.cp_chain(G, k_fit), TL.cp_chain(G, k_fit + 1)
    sc = scores(engine, [sN], [q], [y], [fits], [0.1], [0], check=True)
    PR.assert_close(float(sc.logpdf[0]), fits.to_tuple(), 0.1, *sN, q, y, tol=TOL, ctx=f"{k_fit} ChangePoints at 512 joint points")
    out = raw_call(engine, [sN], [q], [y], [0, 0], G.encode_batch([good, too_many]), [0.1, 0.1])
    assert out[0] == -3 and "particle 1" in out[1] and "LDS" in out[1] and str(N) in out[1] and untouched(out), out[1]
    # P == 0 without mixtures touches nothing
    out = raw_call(engine, [s200], [q], [y], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert out[0] == 0 and untouched(out)
    valid()


def test_stateless(pkg, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    call = lambda e, flag: scores(e, series, qs, held, nodes, noises, sidx, weights=w, noise_pred=noise_pred, want_terms=True,  # noqa: E731
                                  all_long=flag)
    eng = pkg.GPEngine(0)
    try:
        # a fresh engine on which set_data was never called
        assert np.array_equal(sbits(call(eng, False)), sbits(res[False]))
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
        assert np.array_equal(sbits(call(eng, True)), sbits(res[True]))
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
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    out = [None] * 4

    def work(i):
        out[i] = scores(engine, series, qs, held, nodes, noises, sidx, weights=w, noise_pred=noise_pred, want_terms=True,
                        all_long=bool(i % 2))

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i, o in enumerate(out):
        assert o is not None and np.array_equal(sbits(o), sbits(res[bool(i % 2)])), i
