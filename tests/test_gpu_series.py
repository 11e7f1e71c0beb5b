"""GPU tests of agp_logpdf_series_batch (many short series in one fused launch; csrc/agp_series_kernel.hpp): parity with the oracle
on ragged input, every leaf and combinator, agreement with the resident-series path, batch independence (bitwise), statelessness,
non-PD reporting, argument errors and concurrent callers.  Tolerance of every value comparison: |d| <= 1e-8 max(1, |logpdf|)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import _series_cases as S
from oracle import oracle as O
from conftest import to_tuple

pytestmark = pytest.mark.gpu
LP_TOL = 1e-8


def close(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= LP_TOL * np.maximum(1.0, np.abs(b))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The shared case: ten ragged series (prefixes of shuffled synthetic series), six prior particles each, and the oracle's values
    (computed once, never modified)."""
    import __graft_entry__ as g
    pkg = g.load_package()
    lens = [0, 1, 2, 15, 16, 17, 33, 126, 144, pkg.SERIES_MAX_N]
    rng = np.random.default_rng(20261018)
    series, nodes, noises, sidx = [], [], [], []
    for s, n in enumerate(lens):
        ts, xs = pkg.prior.synthetic_series(256, seed=100 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        nd, nz = pkg.prior.sample_particles(rng, 6, max_depth=3)
        nodes += nd; noises += list(nz); sidx += [s] * 6
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), *series[s]) for nd, nz, s in zip(nodes, noises, sidx)])
    for a in (noises, sidx, ref):
        a.setflags(write=False)
    return series, nodes, noises, sidx, ref


@pytest.fixture(scope="module")
def ragged(engine):
    series, nodes, noises, sidx, ref = ragged_case()
    lp, info = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)
    lp.setflags(write=False)
    return series, nodes, noises, sidx, ref, lp, info


def test_ragged_parity(pkg, ragged):
    series, nodes, noises, sidx, ref, lp, info = ragged
    assert len(nodes) == 60 and np.isfinite(ref).all()          # the oracle factorises every particle: none is skipped
    ops = set()
    for nd in nodes:
        ops |= {type(x).__name__ for x in pkg.unroll(nd)}
    assert {"Linear", "GammaExponential", "Periodic", "Plus", "Times", "ChangePoint"} <= ops
    err = np.abs(lp - ref) / np.maximum(1.0, np.abs(ref))
    print("ragged parity: worst relative error", err.max(), "at particle", int(err.argmax()))
    assert (info == 0).all()
    assert (lp[sidx == 0] == 0.0).all()                          # the empty series
    assert close(lp, ref).all(), (int(err.argmax()), err.max())


def full_tree(G, d, i=0):
    leafs = [G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13), G.GammaExponential(0.42, 0.58, 3.2),
             G.Periodic(0.96, 0.21, 1.1), G.Constant(0.5), G.WhiteNoise(0.3)]
    if d == 0:
        return leafs[i % 6]
    l, r = full_tree(G, d - 1, 2 * i + 1), full_tree(G, d - 1, 2 * i + 2)
    return l + r if (d + i) % 2 else l * r


def test_every_leaf_and_combinator(pkg, engine, golden):
    G = pkg
    cases = [c for c in golden["cases"] if "logpdf" in c and len(c["ts"]) <= G.SERIES_MAX_N]
    assert len(cases) >= 20
    kinds = set()
    for c in cases:
        kinds |= {type(x).__name__ for x in G.unroll(G.from_tuple(to_tuple(c["tree"])))}
    assert {"Constant", "SquaredExponential", "WhiteNoise"} <= kinds
    series = [(np.array(c["ts"]), np.array(c["xs"])) for c in cases]
    nodes = [G.from_tuple(to_tuple(c["tree"])) for c in cases]
    noises = np.array([c["noise"] for c in cases])
    lp, info = engine.logpdf_series_batch(series, nodes, noises, np.arange(len(cases)))      # ONE ragged call, each case its own series
    ref = np.array([c["logpdf"] for c in cases])
    assert (info == 0).all()
    bad = ~close(lp, ref)
    assert not bad.any(), [(cases[i]["name"], lp[i], ref[i]) for i in np.flatnonzero(bad)]

    # hand-written: nested ChangePoints, a 16-leaf tree (evaluation stack of depth 5: the D = 8 instantiation), and a
    # GammaExponential on a series with a repeated time point (dt = 0 off the diagonal)
    rng = np.random.default_rng(5)
    ts = rng.random(70); ts[41] = ts[7]
    xs = 0.5 * rng.standard_normal(70)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = full_tree(G, 4)
    assert deep.size() == 31
    ge = G.GammaExponential(0.42, 0.58, 3.2)
    nodes = [nested, deep, ge, G.Constant(0.5) * G.WhiteNoise(0.3)]
    noises = np.array([0.1, 0.2, 0.05, 0.3])
    lp, info = engine.logpdf_series_batch([(ts, xs)], nodes, noises, np.zeros(4, dtype=np.int32))
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), ts, xs) for nd, nz in zip(nodes, noises)])
    assert (info == 0).all() and np.isfinite(ref).all()
    assert close(lp, ref).all(), (lp, ref)


def test_agrees_with_resident_series_path(engine, ragged):
    series, nodes, noises, sidx, ref, lp, info = ragged
    for s in (5, 7, 8):                                          # 17, 126 and 144 points
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        lp_res, info_res = engine.logpdf_batch([nodes[i] for i in sel], noises[sel])
        assert (info_res == 0).all()
        assert close(lp[sel], lp_res).all(), (s, lp[sel], lp_res)


def test_batch_independence_bitwise(engine, ragged):
    series, nodes, noises, sidx, ref, lp, info = ragged
    P = len(nodes)
    rev = np.arange(P)[::-1]
    lp_rev, _ = engine.logpdf_series_batch(series, [nodes[i] for i in rev], noises[rev], sidx[rev], check=False)
    assert np.array_equal(bits(lp_rev), bits(lp[rev]))
    for s in range(len(series)):                                 # one series at a time
        sel = np.flatnonzero(sidx == s)
        one, _ = engine.logpdf_series_batch([series[s]], [nodes[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32),
                                            check=False)
        assert np.array_equal(bits(one), bits(lp[sel])), s
    for p in range(P):                                           # each particle alone
        one, _ = engine.logpdf_series_batch([series[sidx[p]]], [nodes[p]], noises[p:p + 1], [0], check=False)
        assert bits(one)[0] == bits(lp)[p], p


def test_stateless(pkg, ragged):
    series, nodes, noises, sidx, ref, lp, info = ragged
    eng = pkg.GPEngine(0)
    try:
        # a fresh engine on which set_data was never called
        lp0, info0 = eng.logpdf_series_batch(series, nodes, noises, sidx, check=False)
        assert np.array_equal(bits(lp0), bits(lp)) and (info0 == 0).all()
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)      # (with copies: dedup counts them)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max)
        before = snapshot()
        lp1, _ = eng.logpdf_series_batch(series, nodes, noises, sidx, check=False)
        assert np.array_equal(bits(lp1), bits(lp))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        # the store still holds its factors: a longer prefix extends them
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_non_positive_definite(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(40, seed=2)
    bad, good = G.Constant(1.0), G.SquaredExponential(0.3, 0.8)
    K = O.compute_cov_matrix_vectorized(bad.to_tuple(), -0.5, ts)
    first = None
    for k in range(1, 41):
        try:
            np.linalg.cholesky(K[:k, :k])
        except np.linalg.LinAlgError:
            first = k
            break
    assert first == 2                                            # first pivot 0.5 > 0, second minor negative
    lp, info = engine.logpdf_series_batch([(ts, xs)], [bad, good], [-0.5, 0.1], [0, 0], check=False)
    assert info.tolist() == [first, 0] and np.isnan(lp[0])
    alone, info1 = engine.logpdf_series_batch([(ts, xs)], [good], [0.1], [0], check=False)
    assert info1[0] == 0 and bits(alone)[0] == bits(lp)[1]
    assert close(lp[1], O.gp_logpdf(good.to_tuple(), 0.1, ts, xs))
    with pytest.raises(G.PosDefException) as ei:
        engine.logpdf_series_batch([(ts, xs), (ts, xs)], [good, bad], [0.1, -0.5], [0, 1], check=True)
    assert ei.value.particle == 1 and ei.value.info == first


def test_info_at_every_sub_step_and_block(pkg, engine):
    """info through the real entry at every 4-wide sub-step of block 0, on both sides of block boundaries and at the last point:
    thirteen particles that stop being positive definite at a chosen point of one 176-point series, one call, a good particle among
    them (CPU twin: tests/test_series_cpu.py::test_changepoint_particles_fail_at_the_chosen_point)"""
    ts = S.CP_TS
    xs = np.random.default_rng(31).standard_normal(ts.size)
    good = pkg.SquaredExponential(0.3, 0.8)
    nodes = [S.changepoint_particle(pkg, k) for k in S.CP_POINTS]
    first = [S.first_bad_minor(O.compute_cov_matrix_vectorized(nd.to_tuple(), S.CP_NOISE, ts)) for nd in nodes]
    assert first == [k + 1 for k in S.CP_POINTS]
    at = 6                                                       # the good particle sits between the failing ones
    nodes.insert(at, good)
    noises = np.full(len(nodes), S.CP_NOISE); noises[at] = 0.1
    lp, info = engine.logpdf_series_batch([(ts, xs)], nodes, noises, np.zeros(len(nodes), dtype=np.int32), check=False)
    assert np.delete(info, at).tolist() == first, info
    assert np.isnan(np.delete(lp, at)).all()
    alone, info1 = engine.logpdf_series_batch([(ts, xs)], [good], [0.1], [0], check=False)
    assert info[at] == 0 and info1[0] == 0 and bits(alone)[0] == bits(lp)[at]
    assert close(lp[at], O.gp_logpdf(good.to_tuple(), 0.1, ts, xs))


def test_parity_at_the_remaining_block_counts(pkg, engine):
    """the lengths of ragged_case() end in 1, 2, 3, 8, 9 or 11 blocks of 16: here every other final block count (4, 5, 6, 7, 10), full
    and ragged, against the oracle"""
    lens = (49, 80, 81, 97, 112, 145, 161)
    rng = np.random.default_rng(20261019)
    series, nodes, noises, sidx = [], [], [], []
    for s, n in enumerate(lens):
        ts, xs = pkg.prior.synthetic_series(256, seed=200 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        nd, nz = pkg.prior.sample_particles(rng, 6, max_depth=3)
        nodes += nd; noises += list(nz); sidx += [s] * 6
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), *series[s]) for nd, nz, s in zip(nodes, noises, sidx)])
    assert len(nodes) == 42 and np.isfinite(ref).all()          # the oracle factorises every particle: none is skipped
    lp, info = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)
    err = np.abs(lp - ref) / np.maximum(1.0, np.abs(ref))
    print("block-count parity: worst relative error", err.max(), "at particle", int(err.argmax()))
    assert (info == 0).all()
    assert close(lp, ref).all(), (int(err.argmax()), err.max())


def raw_call(engine, pt_off, ts, xs, sidx, programs, noises):
    op_off, ops, prm_off, prm = programs
    P = len(noises)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int64); sidx = np.ascontiguousarray(sidx, dtype=np.int32)
    ts = np.ascontiguousarray(ts, dtype=np.float64); xs = np.ascontiguousarray(xs, dtype=np.float64)
    noises = np.ascontiguousarray(noises, dtype=np.float64)
    out = np.zeros(P); info = np.zeros(P, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = engine._lib.agp_logpdf_series_batch(engine._ctx, len(pt_off) - 1, pt_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                             ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), P, sidx.ctypes.data_as(ip),
                                             op_off.ctypes.data_as(ip), ops.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp),
                                             out.ctypes.data_as(dp), info.ctypes.data_as(ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), out, info


def cp_chain(G, k):
    nd = G.Constant(0.5)
    for i in range(k):
        nd = G.ChangePoint(nd, G.Constant(0.3 + 0.01 * i), 0.1 + 0.8 * i / max(1, k - 1), 0.05)
    return nd


def test_errors_name_the_culprit(pkg, engine):
    G = pkg
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    good = G.SquaredExponential(0.3, 0.8)
    progs = G.encode_batch([good, good])

    def valid():
        lp, info = engine.logpdf_series_batch([(ts[:20], xs[:20])], [good], [0.1], [0])
        assert info[0] == 0 and close(lp[0], O.gp_logpdf(good.to_tuple(), 0.1, ts[:20], xs[:20]))

    with pytest.raises(G.AGPError, match=r"particle 1.*series index 3"):
        engine.logpdf_series_batch([(ts[:20], xs[:20]), (ts[:9], xs[:9])], [good, good], [0.1, 0.1], [0, 3])
    valid()
    with pytest.raises(G.AGPError, match=r"particle 0.*series index -1"):
        engine.logpdf_series_batch([(ts[:20], xs[:20])], [good], [0.1], [-1])
    rc, msg, _, _ = raw_call(engine, [0, 30, 20], ts[:30], xs[:30], [0, 1], progs, [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and "decreases" in msg
    valid()
    rc, msg, _, _ = raw_call(engine, [0, 5, 5 + N + 1], np.tile(ts, 2), np.tile(xs, 2), [0, 1], progs, [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and str(N + 1) in msg
    rc, msg, _, _ = raw_call(engine, [1, 5], ts[:5], xs[:5], [0, 0], progs, [0.1, 0.1])
    assert rc == -1 and "pt_off[0]" in msg
    with pytest.raises(ValueError, match="series 0"):
        engine.logpdf_series_batch([(ts, xs)], [good], [0.1], [0])
    valid()
    # a malformed program: particle 1 is a lone '+'
    op_off, ops, prm_off, prm = G.encode_batch([good])
    bad_prog = (np.array([0, ops.size, ops.size + 1], dtype=np.int32), np.concatenate([ops, np.array([6], dtype=np.uint8)]),
                np.array([0, prm.size, prm.size], dtype=np.int32), prm)
    rc, msg, _, _ = raw_call(engine, [0, 20], ts[:20], xs[:20], [0, 0], bad_prog, [0.1, 0.1])
    assert rc == -3 and "particle 1" in msg and "underflow" in msg
    valid()
    # per-point tables beyond the LDS budget at the cap: a chain of ChangePoints (8 fit, 16 do not — and do fit a shorter series)
    fits, too_many = cp_chain(G, 8), cp_chain(G, 16)
    lp, info = engine.logpdf_series_batch([(ts[:N], xs[:N])], [fits], [0.1], [0])
    assert info[0] == 0 and close(lp[0], O.gp_logpdf(fits.to_tuple(), 0.1, ts[:N], xs[:N]))
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*LDS"):
        engine.logpdf_series_batch([(ts[:N], xs[:N])], [good, too_many], [0.1, 0.1], [0, 0])
    lp, info = engine.logpdf_series_batch([(ts[:100], xs[:100])], [too_many], [0.1], [0])
    assert info[0] == 0 and close(lp[0], O.gp_logpdf(too_many.to_tuple(), 0.1, ts[:100], xs[:100]))
    # P == 0 touches nothing
    rc, msg, _, _ = raw_call(engine, [0], ts[:1], xs[:1], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert rc == 0
    valid()


def test_concurrent_callers(engine, ragged):
    series, nodes, noises, sidx, ref, lp, info = ragged
    out = [None] * 4

    def work(i):
        out[i] = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)[0]

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for o in out:
        assert o is not None and np.array_equal(bits(o), bits(lp))
