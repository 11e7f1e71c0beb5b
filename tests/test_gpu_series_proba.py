"""GPU tests of agp_predict_logpdf_series_batch (held-out scores of many short series in one fused launch; k_series_predict_logpdf,
csrc/agp_series_kernel.hpp, and the mixture read-out k_series_mix_logp): parity with the reference restatement of the predictive
log-density (tests/_pred_logpdf_ref.py) on one ragged call, evaluator coverage, cross-checks against the resident-series entry and
against differences of the value entry, the per-point terms, the mixtures, the info rule on the joint points, batch independence
(bitwise), statelessness, a poisoned engine, argument errors and concurrent callers.
Tolerance of every comparison with a reference or another route: |lp - ref| <= 1e-8 S per particle, S the sum of the magnitudes of
the terms the log-density is made of (tests/_pred_logpdf_ref.reference) — the tolerance and scale tests/test_gpu_predict_logpdf.py
uses for the same quantity; n + m <= 176 is always inside the range of its mpmath / 80-bit arbiter, which decides misses.  Sums of
the entry's own numbers in another order: 1e-12 S.  No particle is skipped anywhere: the fp64 reference factors every particle of
every case (asserted), unless the test is about failure."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import _pred_logpdf_ref as PR
import _series_cases as SC
import _series_proba_ref as R
import test_gpu_series as TS
from oracle import oracle as O

pytestmark = pytest.mark.gpu
bits = TS.bits
TOL = 1e-8


def sbits(sc):
    """every output of a call as one int64 vector: logpdf, terms, mixtures (bit patterns), info"""
    parts = [bits(sc.logpdf)]
    if sc.terms is not None:
        parts += [bits(t) for t in sc.terms]
    if sc.series_logp is not None:
        parts.append(bits(sc.series_logp))
    parts.append(np.asarray(sc.info, dtype=np.int64))
    return np.concatenate(parts)


def pbits(sc, sel):
    """the per-particle outputs of the particles sel, in that order"""
    sel = list(sel)
    parts = [bits(sc.logpdf[sel])] + ([bits(sc.terms[i]) for i in sel] if sc.terms is not None else [])
    return np.concatenate(parts + [np.asarray(sc.info[sel], dtype=np.int64)])


def uniform_weights(sidx):
    sidx = np.asarray(sidx)
    return np.array([1.0 / (sidx == s).sum() for s in sidx])


def check_parity(name, sc, series, qs, held, nodes, noises, sidx, noise_pred=None):
    """every particle through _pred_logpdf_ref.assert_close (its reference must factor: none is skipped); returns [(ref, S)]"""
    out = []
    worst = 0.0
    assert (np.asarray(sc.info) == 0).all(), (name, sc.info)
    for p, nd in enumerate(nodes):
        s = int(sidx[p])
        npp = None if noise_pred is None else float(noise_pred[p])
        if len(qs[s]) == 0:
            assert sc.logpdf[p] == 0.0, (name, p)
            out.append((0.0, 0.0))
            continue
        ref, S = PR.assert_close(float(sc.logpdf[p]), nd.to_tuple(), float(noises[p]), *series[s], qs[s], held[s], tol=TOL,
                                 ctx=(name, p, s), noise_pred=npp)      # (raises PosDefException where the reference cannot factor)
        assert math.isfinite(ref) and S > 0.0, (name, p)
        worst = max(worst, abs(sc.logpdf[p] - ref) / S)
        out.append((ref, S))
    assert len(out) == len(nodes)                      # none is skipped
    print(f"[series-proba] {name}: worst |lp - ref| / S = {worst:.3e} over {len(nodes)} particles")
    return out


@pytest.fixture(scope="module")
def ragged(engine):
    """tests/_series_proba_ref.ragged_case() through the entry, once per noise_pred variant, with terms and uniform mixtures"""
    series, qs, held, nodes, noises, sidx, noise_pred = R.ragged_case()
    w = uniform_weights(sidx)
    res = {}
    for key, npred in (("default", None), ("per particle", noise_pred)):
        sc = engine.predict_logpdf_series_batch(series, qs, held, nodes, noises, sidx, weights=w, noise_pred=npred, want_terms=True,
                                                check=False)
        for a in (sc.logpdf, sc.series_logp, sc.info, *sc.terms):
            a.setflags(write=False)
        res[key] = sc
    return series, qs, held, nodes, noises, sidx, noise_pred, w, res


@pytest.fixture(scope="module")
def scales(ragged):
    """(ref, S) of every particle of the ragged case, per noise_pred variant — the parity check itself, computed once"""
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    return {key: check_parity("ragged, noise_pred " + key, res[key], series, qs, held, nodes, noises, sidx, npred)
            for key, npred in (("default", None), ("per particle", noise_pred))}


def test_ragged_parity(pkg, ragged, scales):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    assert tuple((len(t), len(q)) for (t, _), q in zip(series, qs)) == R.SHAPES and len(nodes) == 13 * len(R.SHAPES)
    assert (noise_pred[::2] < noises[::2]).all()
    for key in res:
        assert len(scales[key]) == len(nodes)
        sc = res[key]
        assert [len(t) for t in sc.terms] == [len(qs[s]) for s in sidx]
        # nothing held out: 0, info 0, an empty block
        for p in np.flatnonzero(sidx == 2):
            assert sc.logpdf[p] == 0.0 and sc.info[p] == 0 and sc.terms[p].size == 0
    # the prior predictive of the empty series is that of K22 + noise_pred I
    for p in np.flatnonzero(sidx == 0):
        K = O.compute_cov_matrix_vectorized(nodes[p].to_tuple(), float(noises[p]), qs[0])
        direct = O.mvnormal_logpdf(held[0], K)
        assert abs(res["default"].logpdf[p] - direct) <= TOL * scales["default"][p][1]


def test_remaining_block_counts(pkg, engine):
    """the joint lengths of the ragged case end in 1, 2, 3, 5, 9 or 11 blocks of 16: here 4, 6, 7, 8 and 10"""
    rng = np.random.default_rng(77)
    series, qs, held, nodes, noises, sidx = [], [], [], [], [], []
    for s, (n, m) in enumerate(R.EXTRA_SHAPES):
        ts, xs = pkg.prior.synthetic_series(256, seed=700 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        qs.append(R.queries(R.QUERY_KINDS[s % 3], ts[:n], m, rng)); held.append(0.5 * rng.standard_normal(m))
        nd = R.fixture_kernels(pkg)[2:8]
        nodes += nd; noises += [0.1] * len(nd); sidx += [s] * len(nd)
    sc = engine.predict_logpdf_series_batch(series, qs, held, nodes, noises, sidx, noise_pred=0.04, check=False)
    check_parity("remaining block counts", sc, series, qs, held, nodes, noises, sidx, noise_pred=np.full(len(nodes), 0.04))


def test_evaluator_coverage(pkg, engine):
    G = pkg
    rng = np.random.default_rng(5)
    ts = rng.random(70); ts[41] = ts[7]                                  # a repeated time point
    xs = 0.5 * rng.standard_normal(70)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = TS.full_tree(G, 4)                                            # 31 nodes, evaluation stack of depth 5: the D = 8 instantiation
    assert deep.size() == 31
    q = np.array([0.05, 0.29, 0.31, 0.45, 0.59, 0.61, 0.95, ts[7], ts[7], ts[0], 1.2, -0.2, 0.3, 0.6, 0.5, 0.7, 0.1])
    y = 0.5 * rng.standard_normal(q.size)
    nodes = [nested, deep, G.GammaExponential(0.42, 0.58, 3.2), G.Constant(0.5) * G.WhiteNoise(0.3)]
    noises = np.array([0.1, 0.2, 0.05, 0.3])
    sidx = np.zeros(4, dtype=np.int32)
    sc = engine.predict_logpdf_series_batch([(ts, xs)], [q], [y], nodes, noises, sidx, noise_pred=0.5 * noises, check=False)
    check_parity("hand-written", sc, [(ts, xs)], [q], [y], nodes, noises, sidx, noise_pred=0.5 * noises)
    # the longest ChangePoint chain that fits at the cap (counted from the kernel's own map), and the split in the last block
    N = G.SERIES_MAX_N
    n, m = 150, 26
    assert n + m == N
    k_fit = max(k for k in range(1, 40) if R.cp_chain_fits(k, n, m))
    ts, xs = G.prior.synthetic_series(N, seed=4)
    tq = np.linspace(-0.1, 1.3, m); tq[5] = ts[11]
    y = 0.5 * rng.standard_normal(m)
    chain, too_long = TS.cp_chain(G, k_fit), TS.cp_chain(G, k_fit + 1)
    one = ([(ts[:n], xs[:n])], [tq], [y])
    sc = engine.predict_logpdf_series_batch(*one, [chain], [0.1], [0], check=False)
    check_parity("ChangePoint chain at N = 176", sc, *one, [chain], [0.1], [0])
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*LDS"):
        engine.predict_logpdf_series_batch(*one, [chain, too_long], [0.1, 0.1], [0, 0])
    # ... which fits a shorter joint series
    short = ([(ts[:60], xs[:60])], [tq], [y])
    sc = engine.predict_logpdf_series_batch(*short, [too_long], [0.1], [0], check=False)
    check_parity("one more ChangePoint at 86 points", sc, *short, [too_long], [0.1], [0])


def test_agrees_with_resident_series_path(engine, ragged, scales):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    for s in (R.SHAPES.index((17, 5)), R.SHAPES.index((126, 18)), R.SHAPES.index((144, 32))):
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        for key, npred in (("default", None), ("per particle", noise_pred)):
            lp_r, info_r = engine.predict_logpdf_batch([nodes[i] for i in sel], noises[sel], qs[s], held[s],
                                                       noise_pred=None if npred is None else npred[sel], check=False)
            assert (np.asarray(info_r) == 0).all()
            for k, i in enumerate(sel):
                assert abs(res[key].logpdf[i] - lp_r[k]) <= TOL * scales[key][i][1], (s, key, i)


def test_agrees_with_differences_of_the_value_entry(engine, ragged):
    """noise_pred = noise, slope 1: log p(held-out | training) = logpdf_series_batch(training ++ held-out) - logpdf_series_batch(training);
    S = the sum of the magnitudes of both values"""
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    joint = [(np.concatenate([t, q]), np.concatenate([x, y])) for (t, x), q, y in zip(series, qs, held)]
    lj, ij = engine.logpdf_series_batch(joint, nodes, noises, sidx, check=False)
    lt, it = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)
    assert (ij == 0).all() and (it == 0).all()
    lp = res["default"].logpdf
    for p in range(len(nodes)):
        S = abs(lj[p]) + abs(lt[p])
        assert abs(lp[p] - (lj[p] - lt[p])) <= TOL * max(S, 1e-300), (p, lp[p], lj[p] - lt[p])


def test_terms(pkg, engine, ragged, scales):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    for key, sc in res.items():
        for p in range(len(nodes)):
            if sc.terms[p].size:
                assert abs(sc.terms[p].sum() - sc.logpdf[p]) <= 1e-12 * scales[key][p][1], (key, p)
    # the partial sums are the entry's own scores of the first j held-out points: both sides of the block boundaries at joint
    # positions 32 and 48 of a (17, 40) split, the first and the last point
    n, m = 17, 40
    ts, xs = pkg.prior.synthetic_series(256, seed=8, shuffle=True)
    rng = np.random.default_rng(2)
    tq = rng.random(m); y = 0.5 * rng.standard_normal(m)
    nd = R.fixture_kernels(pkg)[2:]
    nz = np.full(len(nd), 0.15)
    train = (ts[:n].copy(), xs[:n].copy())
    full = engine.predict_logpdf_series_batch([train], [tq], [y], nd, nz, np.zeros(len(nd), dtype=np.int32), noise_pred=0.05,
                                              want_terms=True)
    js = (1, 14, 15, 16, 30, 31, 32, 39, 40)
    # ONE call: series j = the same training points with the first j held-out points
    many = engine.predict_logpdf_series_batch([train] * len(js), [tq[:j] for j in js], [y[:j] for j in js], nd * len(js),
                                              np.tile(nz, len(js)), np.repeat(np.arange(len(js)), len(nd)), noise_pred=0.05)
    for a, j in enumerate(js):
        for k in range(len(nd)):
            _, S = PR.reference(nd[k].to_tuple(), 0.15, *train, tq[:j], y[:j], noise_pred=0.05)
            assert abs(full.terms[k][:j].sum() - many.logpdf[a * len(nd) + k]) <= TOL * S, (j, k)
    assert np.array_equal(bits(many.logpdf[-len(nd):]), bits(full.logpdf))


def lse(lp, w):
    keep = w > 0
    M = lp[keep].max()
    return M + math.log(np.sum(w[keep] * np.exp(lp[keep] - M)))


def test_mixture(pkg, engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    for sc in res.values():
        for s in range(len(series)):
            sel = np.flatnonzero(sidx == s)
            if len(qs[s]) == 0:
                assert sc.series_logp[s] == 0.0 and not np.signbit(sc.series_logp[s])      # exactly 0.0
                continue
            ref = lse(sc.logpdf[sel], w[sel])
            assert abs(sc.series_logp[s] - ref) <= 1e-12 * max(1.0, abs(ref)), s
    # particles of a series not adjacent, a zero weight, a series without particles, a transform on one series
    G = pkg
    pick = [R.SHAPES.index(x) for x in ((17, 5), (5, 0), (33, 47), (16, 16))]
    ser = [series[s] for s in pick]; q = [qs[s] for s in pick]; y = [held[s] for s in pick]
    nd = R.fixture_kernels(G)[2:7]
    mix_nodes = [nd[0], nd[1], nd[2], nd[3], nd[4], nd[0], nd[1]]
    mix_sidx = np.array([0, 2, 0, 1, 2, 0, 1], dtype=np.int32)           # series 3 has no particle
    mix_w = np.array([0.25, 0.4, 0.0, 0.5, 0.6, 0.75, 0.5])
    nz = np.full(7, 0.1)
    yt = [(1.0, 0.0), (1.0, 0.0), (-2.5, 0.3), (1.0, 0.0)]
    raw = [y[0], y[1], (y[2] - 0.3) / -2.5, y[3]]                        # raw values whose scaled images are the ragged case's
    sc = engine.predict_logpdf_series_batch(ser, q, raw, mix_nodes, nz, mix_sidx, weights=mix_w, y_transforms=yt)
    plain = engine.predict_logpdf_series_batch(ser, q, y, mix_nodes, nz, mix_sidx, weights=mix_w)
    for s in (0, 2):
        sel = np.flatnonzero(mix_sidx == s)
        ref = lse(sc.logpdf[sel], mix_w[sel])
        assert abs(sc.series_logp[s] - ref) <= 1e-12 * max(1.0, abs(ref)), s
    assert sc.series_logp[1] == 0.0 and math.isnan(sc.series_logp[3])
    # raw space: the transform adds m log|slope| to every particle of that series and to its mixture, and nothing elsewhere
    shift = len(q[2]) * math.log(2.5)
    for p in np.flatnonzero(mix_sidx == 2):
        want = plain.logpdf[p] + shift
        assert abs(sc.logpdf[p] - want) <= 1e-12 * (abs(plain.logpdf[p]) + shift), p
    assert abs(sc.series_logp[2] - (plain.series_logp[2] + shift)) <= 1e-12 * (abs(plain.series_logp[2]) + shift)
    other = np.flatnonzero(mix_sidx != 2)
    assert np.array_equal(bits(sc.logpdf[other]), bits(plain.logpdf[other]))
    assert np.array_equal(bits(sc.series_logp[[0, 1]]), bits(plain.series_logp[[0, 1]]))
    # a failed particle at weight 0: NaN for ITS series only, the other series' bits unchanged
    bad_nodes = list(mix_nodes); bad_nz = nz.copy()
    bad_nodes[2] = G.Constant(1.0); bad_nz[2] = -0.5
    bad = engine.predict_logpdf_series_batch(ser, q, y, bad_nodes, bad_nz, mix_sidx, weights=mix_w, check=False)
    assert bad.info[2] > 0 and math.isnan(bad.logpdf[2]) and math.isnan(bad.series_logp[0])
    keep = [0, 1, 3, 4, 5, 6]
    assert np.array_equal(pbits(bad, keep), pbits(plain, keep))
    assert np.array_equal(bits(bad.series_logp[[1, 2]]), bits(plain.series_logp[[1, 2]])) and math.isnan(bad.series_logp[3])
    with pytest.raises(G.PosDefException):
        engine.predict_logpdf_series_batch(ser, q, y, bad_nodes, bad_nz, mix_sidx, weights=mix_w)


INFO_N = 40
INFO_POSITIONS = (1, 16, 17, INFO_N, INFO_N + 1, INFO_N + 16, SC.N_CAP)


def test_info_is_the_first_bad_pivot_of_the_joint_factor(pkg, engine):
    """changepoint_particle on the JOINT times: the first INFO_N points of CP_TS train, the rest are held out, both noises CP_NOISE"""
    G = pkg
    ts, tq = SC.CP_TS[:INFO_N], SC.CP_TS[INFO_N:]
    rng = np.random.default_rng(3)
    xs = 0.3 * rng.standard_normal(INFO_N); y = 0.3 * rng.standard_normal(len(tq))
    good = [G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.3, 0.9) + G.Linear(0.2, 0.3, 0.4)]
    nodes, noises = [good[0]], [0.1]
    for pos in INFO_POSITIONS:
        node = SC.changepoint_particle(G, pos - 1)
        assert SC.first_bad_minor(O.compute_cov_matrix_vectorized(node.to_tuple(), SC.CP_NOISE, SC.CP_TS)) == pos
        nodes.append(node); noises.append(SC.CP_NOISE)
    nodes.append(good[1]); noises.append(0.2)
    P = len(nodes)
    sc = engine.predict_logpdf_series_batch([(ts, xs)], [tq], [y], nodes, noises, np.zeros(P, dtype=np.int32), want_terms=True, check=False)
    assert sc.info.tolist() == [0, *INFO_POSITIONS, 0]
    for p in range(1, P - 1):
        assert math.isnan(sc.logpdf[p]) and sc.terms[p].shape == (len(tq),) and np.isnan(sc.terms[p]).all()
    for p, (nd, nz) in ((0, (good[0], 0.1)), (P - 1, (good[1], 0.2))):      # the neighbours: the bits of the particle alone
        alone = engine.predict_logpdf_series_batch([(ts, xs)], [tq], [y], [nd], [nz], [0], want_terms=True)
        assert np.isfinite(alone.logpdf).all() and np.array_equal(pbits(alone, [0]), pbits(sc, [p]))
        PR.assert_close(float(sc.logpdf[p]), nd.to_tuple(), nz, ts, xs, tq, y, tol=TOL, ctx=("beside failed particles", p))
    with pytest.raises(G.PosDefException) as ei:
        engine.predict_logpdf_series_batch([(ts, xs)], [tq], [y], nodes, noises, np.zeros(P, dtype=np.int32))
    assert ei.value.particle == 1 and ei.value.info == 1


def test_batch_independence_bitwise(engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    sc = res["per particle"]
    P = len(nodes)
    rev = np.arange(P)[::-1]
    r_rev = engine.predict_logpdf_series_batch(series, qs, held, [nodes[i] for i in rev], noises[rev], sidx[rev], weights=w[rev],
                                               noise_pred=noise_pred[rev], want_terms=True, check=False)
    assert np.array_equal(pbits(r_rev, range(P)), pbits(sc, rev))
    # (uniform weights, reversed order inside each mixture: the same set of numbers summed in another order)
    both = np.isfinite(sc.series_logp)
    assert np.array_equal(both, np.isfinite(r_rev.series_logp))
    assert (np.abs(r_rev.series_logp[both] - sc.series_logp[both]) <= 1e-12 * np.maximum(1.0, np.abs(sc.series_logp[both]))).all()
    for s in range(len(series)):                                 # one series at a time: its particles' bits and its mixture's
        sel = np.flatnonzero(sidx == s)
        one = engine.predict_logpdf_series_batch([series[s]], [qs[s]], [held[s]], [nodes[i] for i in sel], noises[sel],
                                                 np.zeros(len(sel), dtype=np.int32), weights=w[sel], noise_pred=noise_pred[sel],
                                                 want_terms=True, check=False)
        assert np.array_equal(pbits(one, range(len(sel))), pbits(sc, sel)), s
        assert np.array_equal(bits(one.series_logp), bits(sc.series_logp[s:s + 1])), s
    for p in range(P):                                           # each particle alone
        s = sidx[p]
        one = engine.predict_logpdf_series_batch([series[s]], [qs[s]], [held[s]], [nodes[p]], noises[p:p + 1], [0],
                                                 noise_pred=noise_pred[p:p + 1], want_terms=True, check=False)
        assert np.array_equal(pbits(one, [0]), pbits(sc, [p])), p


def test_stateless(pkg, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    call = lambda e: e.predict_logpdf_series_batch(series, qs, held, nodes, noises, sidx, weights=w, want_terms=True, check=False)  # noqa: E731
    eng = pkg.GPEngine(0)
    try:
        # a fresh engine on which set_data was never called
        assert np.array_equal(sbits(call(eng)), sbits(res["default"]))
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
        assert np.array_equal(sbits(call(eng)), sbits(res["default"]))
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


POISON_LENS = (0, 1, 17, 33, 150)
POISON_HELD = (3, 0, 17, 65, 26)


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    """under AGP_POISON=1 (every `values` buffer of the slot is NaN bytes before the call) the entry returns, bit for bit, what an
    engine without poison returns"""
    G = pkg
    rng = np.random.default_rng(41)
    series, qs, held, nodes, noises, sidx = [], [], [], [], [], []
    for s, (n, m) in enumerate(zip(POISON_LENS, POISON_HELD)):
        ts, xs = G.prior.synthetic_series(256, seed=900 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        tq = 1.0 + 0.01 * np.arange(1, m + 1)
        if m and n:
            tq[0] = ts[0]
        qs.append(tq); held.append(0.5 * rng.standard_normal(m))
        nd = R.fixture_kernels(G)[6:8]
        nodes += nd; noises += [0.1, 0.2]; sidx += [s, s]
    nodes += [TS.cp_chain(G, 4), TS.full_tree(G, 4)]; noises += [0.1, 0.2]; sidx += [4, 4]
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    w = uniform_weights(sidx)
    yt = [(1.0, 0.0), (2.0, 0.5), (-0.5, 0.1), (1.0, 0.0), (1.5, -0.2)]
    call = lambda e: e.predict_logpdf_series_batch(series, qs, held, nodes, noises, sidx, weights=w, y_transforms=yt,  # noqa: E731
                                                   noise_pred=0.5 * noises, want_terms=True, check=False)
    ref = call(engine)
    assert (ref.info == 0).all() and np.isfinite(ref.logpdf).all() and np.isfinite(ref.series_logp).all()
    assert all(np.isfinite(t).all() for t in ref.terms) and [len(t) for t in ref.terms] == [POISON_HELD[s] for s in sidx]
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = G.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = call(e)
            assert np.array_equal(sbits(got), sbits(ref)), (poison, np.flatnonzero(sbits(got) != sbits(ref))[:8])
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()


def test_concurrent_callers(engine, ragged):
    series, qs, held, nodes, noises, sidx, noise_pred, w, res = ragged
    out = [None] * 4

    def work(i):
        out[i] = engine.predict_logpdf_series_batch(series, qs, held, nodes, noises, sidx, weights=w, want_terms=True, check=False)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for o in out:
        assert o is not None and np.array_equal(sbits(o), sbits(res["default"]))


SENTINEL = 7.25


def raw_call(engine, series, qs, held, sidx, programs, noises, weights=None, y_slope=None, pt_off=None, q_off=None, null=(), mix=None):
    """the C entry itself with sentinel-filled outputs: (rc, msg, logpdf, terms, out_off, series_logp, info); out_series_logp is
    passed exactly when weights are, unless `mix` says otherwise"""
    op_off, ops, prm_off, prm = programs
    P = len(noises)
    S = len(series)
    if pt_off is None:
        pt_off = np.concatenate([[0], np.cumsum([len(t) for t, _ in series])])
    if q_off is None:
        q_off = np.concatenate([[0], np.cumsum([len(q) for q in qs])])
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.int64)
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
    rc = engine._lib.agp_predict_logpdf_series_batch(
        engine._ctx, S, pt_off.ctypes.data_as(lp_), ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), arg("q_off", q_off, lp_),
        arg("ts_pred", tq, dp), arg("y_pred", yq, dp), P, sidx.ctypes.data_as(ip), op_off.ctypes.data_as(ip),
        ops.ctypes.data_as(C.POINTER(C.c_uint8)), prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp), None,
        arg("y_slope", sl, dp), arg("weights", w, dp), arg("out_logpdf", lp, dp), arg("out_terms", terms, dp), arg("out_off", off, lp_),
        arg("out_series_logp", mixo if ((w is not None) if mix is None else mix) else None, dp), arg("out_info", info, ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), lp, terms, off, mixo, info


def test_errors_name_the_culprit(pkg, engine):
    G = pkg
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    q = np.linspace(1.0, 1.3, 9); y = np.linspace(-0.4, 0.4, 9)
    good = G.SquaredExponential(0.3, 0.8)
    progs = G.encode_batch([good, good])
    s20, s9 = (ts[:20], xs[:20]), (ts[:9], xs[:9])
    ref20, S20 = PR.reference(good.to_tuple(), 0.1, *s20, q, y)

    def valid():
        sc = engine.predict_logpdf_series_batch([s20], [q], [y], [good], [0.1], [0])
        assert sc.info[0] == 0 and abs(sc.logpdf[0] - ref20) <= TOL * S20

    def untouched(out):
        rc, msg, lp, terms, off, mixo, info = out
        return bool((lp == SENTINEL).all() and (terms == SENTINEL).all() and (off == -1).all() and (mixo == SENTINEL).all()
                    and (info == 7).all())

    two = ([s20, s9], [q, q], [y, y], [0, 1], progs, [0.1, 0.1])
    # the call as it is: valid, and the sentinels behind the outputs stay
    out = raw_call(engine, *two, weights=[1.0, 1.0])
    assert out[0] == 0 and out[2][2] == SENTINEL and out[3][18] == SENTINEL and out[5][2] == SENTINEL and out[4].tolist() == [0, 9, 18]
    assert abs(out[2][0] - ref20) <= TOL * S20 and out[5][0] == out[2][0] and out[5][1] == out[2][1]      # one particle at weight 1
    # everything agp_predict_series_batch reports
    out = raw_call(engine, *two, q_off=[1, 9, 18])
    assert out[0] == -1 and "q_off[0]" in out[1] and untouched(out)
    out = raw_call(engine, *two, q_off=[0, 9, 5])
    assert out[0] == -1 and "series 1" in out[1] and "q_off decreases" in out[1] and untouched(out)
    out = raw_call(engine, *two, pt_off=[0, 30, 20])
    assert out[0] == -1 and "series 1" in out[1] and "pt_off decreases" in out[1] and untouched(out)
    for name in ("q_off", "ts_pred", "out_logpdf", "out_info"):
        out = raw_call(engine, *two, null=(name,))
        assert out[0] == -1 and "null pointer" in out[1], name
    valid()
    with pytest.raises(G.AGPError, match=r"particle 1.*series index 3"):
        engine.predict_logpdf_series_batch([s20, s9], [q, q], [y, y], [good, good], [0.1, 0.1], [0, 3])
    out = raw_call(engine, [(ts[:5], xs[:5]), (ts, xs)], [q, q], [y, y], [0, 1], progs, [0.1, 0.1])
    assert out[0] == -1 and "series 1" in out[1] and str(N + 1) in out[1] and untouched(out)
    # training and held-out points together beyond the cap: both counts are given
    sbig = (ts[:N - 5], xs[:N - 5])
    out = raw_call(engine, [s20, sbig], [q, q], [y, y], [0, 1], progs, [0.1, 0.1])
    assert out[0] == -1 and "series 1" in out[1] and str(N - 5) in out[1] and " 9 " in out[1] and "AGP_SERIES_MAX_N" in out[1] and untouched(out)
    out = raw_call(engine, [s20, sbig], [q, q[:5]], [y, y[:5]], [0, 1], progs, [0.1, 0.1])      # exactly the cap
    assert out[0] == 0 and (out[6][:2] == 0).all()
    out = raw_call(engine, [s20, (ts[:N], xs[:N])], [q, q[:0]], [y, y[:0]], [0, 1], progs, [0.1, 0.1])      # nothing held out: no limit
    assert out[0] == 0 and out[2][1] == 0.0
    # the held-out values
    out = raw_call(engine, *two, null=("y_pred",))
    assert out[0] == -1 and "y_pred" in out[1] and untouched(out)
    for badv in (math.nan, math.inf):
        yb = y.copy(); yb[4] = badv
        out = raw_call(engine, [s20, s9], [q, q], [y, yb], [0, 1], progs, [0.1, 0.1])
        assert out[0] == -1 and "series 1" in out[1] and "not finite" in out[1] and untouched(out)
    # the slopes
    for badv in (0.0, math.nan, -math.inf):
        out = raw_call(engine, *two, y_slope=[1.0, badv])
        assert out[0] == -1 and "series 1" in out[1] and "slope" in out[1] and untouched(out)
    # the weights: the band entry's check, per series
    for wts, what in (([1.0, math.nan], "finite"), ([1.0, -1.0], ">= 0"), ([1.0, 0.5], "sum to 1")):
        out = raw_call(engine, *two, weights=wts)
        assert out[0] == -1 and "series 1" in out[1] and what in out[1] and untouched(out)
    out = raw_call(engine, *two, weights=[1.0, 1.0 + 1e-9])
    assert out[0] == 0
    out = raw_call(engine, *two, weights=[1.0, 1.0], mix=False)
    assert out[0] == -1 and "out_series_logp" in out[1] and untouched(out)
    out = raw_call(engine, *two, mix=True)
    assert out[0] == -1 and "out_series_logp" in out[1] and untouched(out)
    valid()
    # a malformed program: particle 1 is a lone '+'
    op_off, ops, prm_off, prm = G.encode_batch([good])
    bad_prog = (np.array([0, ops.size, ops.size + 1], dtype=np.int32), np.concatenate([ops, np.array([6], dtype=np.uint8)]),
                np.array([0, prm.size, prm.size], dtype=np.int32), prm)
    out = raw_call(engine, [s20], [q], [y], [0, 0], bad_prog, [0.1, 0.1])
    assert out[0] == -3 and "particle 1" in out[1] and "underflow" in out[1] and untouched(out)
    # the LDS refusal at N points leaves the outputs alone too
    k_fit = max(k for k in range(1, 40) if R.cp_chain_fits(k, N - 9, 9))
    progs2 = G.encode_batch([good, TS.cp_chain(G, k_fit + 1)])
    out = raw_call(engine, [(ts[:N - 9], xs[:N - 9])], [q], [y], [0, 0], progs2, [0.1, 0.1])
    assert out[0] == -3 and "particle 1" in out[1] and "LDS" in out[1] and str(N) in out[1] and untouched(out)
    # P == 0 without mixtures touches nothing; with them every series is without particles
    out = raw_call(engine, [s20], [q], [y], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert out[0] == 0 and untouched(out)
    valid()
