"""GPU tests of agp_logpdf_long_series_batch (series of up to 512 points; csrc/agp_long_series_kernel.hpp): parity with the oracle
on ragged input under both routings, every block count, every leaf and combinator, agreement with the resident-series path, batch
independence (bitwise, the workspace split included), bad pivots at chosen points, capacity and refusals, statelessness and
concurrent callers.  Tolerance of every value comparison: |d| <= 1e-8 max(1, |logpdf|), the family's."""
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
LENS = [0, 1, 2, 15, 16, 17, 33, 176, 177, 192, 193, 255, 256, 257, 442, 512]      # both sides of 16, 128, 176 and 256; 442; the cap
BLOCK_LENS = (1, 5, 16, 17, 33, 48, 49, 80, 81, 112, 129, 145, 176, 177, 209, 241, 273, 305, 337, 369, 401, 433, 465, 497, 512)
CP_N = 512
CP_POINTS = (0, 1, 3, 4, 15, 16, 17, 175, 176, 177, 255, 256, 257, 447, 448, 495, 496, 511)
CP_NOISE = -0.5


def close(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) <= LP_TOL * np.maximum(1.0, np.abs(b))


def relerr(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(b))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cp_ts():
    return np.linspace(0.0, 1.0, CP_N)


def changepoint_particle(G, k):
    """With noise CP_NOISE on cp_ts(): diagonal 0.5 before point k and -0.499 from k on (the ChangePoint switches half a grid step
    before ts[k], 9.8 scales away from either neighbour: sigma is 0 or 1 to 3e-9) -> the first failing leading minor is k + 1
    (CPU twin: tests/test_long_series_cpu.py)"""
    return G.ChangePoint(G.WhiteNoise(1.0), G.Constant(1e-3), cp_ts()[k] - 0.5 / (CP_N - 1), 1e-4)


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The shared case: sixteen ragged series (prefixes of shuffled synthetic series), four prior particles each, and the oracle's
    values (computed once, never modified)."""
    import __graft_entry__ as g
    pkg = g.load_package()
    rng = np.random.default_rng(20261021)
    series, nodes, noises, sidx = [], [], [], []
    for s, n in enumerate(LENS):
        ts, xs = pkg.prior.synthetic_series(512, seed=300 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        nd, nz = pkg.prior.sample_particles(rng, 4, max_depth=3)
        nodes += nd; noises += list(nz); sidx += [s] * 4
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), *series[s]) for nd, nz, s in zip(nodes, noises, sidx)])
    for a in (noises, sidx, ref):
        a.setflags(write=False)
    return series, nodes, noises, sidx, ref


@pytest.fixture(scope="module")
def ragged(engine):
    series, nodes, noises, sidx, ref = ragged_case()
    lp, info = engine.logpdf_long_series_batch(series, nodes, noises, sidx, check=False)
    la, ia = engine.logpdf_long_series_batch(series, nodes, noises, sidx, all_long=True, check=False)
    lp.setflags(write=False); la.setflags(write=False)
    return series, nodes, noises, sidx, ref, (lp, info), (la, ia)


def test_ragged_parity_both_routings(pkg, engine, ragged):
    series, nodes, noises, sidx, ref, default, all_long = ragged
    assert len(nodes) == 64 and np.isfinite(ref).all()          # the oracle factorises every particle: none is skipped
    ops = set()
    for nd in nodes:
        ops |= {type(x).__name__ for x in pkg.unroll(nd)}
    assert {"Linear", "GammaExponential", "Periodic", "Plus", "Times", "ChangePoint"} <= ops
    for name, (lp, info) in (("default routing", default), ("all_long", all_long)):
        err = relerr(lp, ref)
        print(f"ragged parity, {name}: worst relative error", err.max(), "at particle", int(err.argmax()))
        assert (info == 0).all(), name
        assert (lp[sidx == 0] == 0.0).all(), name                # the empty series
        assert close(lp, ref).all(), (name, int(err.argmax()), err.max())
    # default routing: up to the short cap the launch is logpdf_series_batch's, and so are the bits
    short = np.flatnonzero(np.array([len(series[s][0]) for s in sidx]) <= pkg.SERIES_MAX_N)
    n_short = int(sidx[short].max()) + 1
    assert len(short) == 4 * n_short == 32
    ls, _ = engine.logpdf_series_batch(series[:n_short], [nodes[i] for i in short], noises[short], sidx[short], check=False)
    assert np.array_equal(bits(ls), bits(default[0][short]))


def test_every_block_count(pkg, engine):
    """all_long: one series per final block count 1 .. 32, full and ragged, two particles each.  n <= 256: exact_particles — the
    covariance is exact in float64, any error belongs to the factorisation"""
    rng = np.random.default_rng(20261022)
    series, nodes, noises, sidx = [], [], [], []
    for s, n in enumerate(BLOCK_LENS):
        if n <= 256:
            ts, particles = S.exact_particles(pkg, n)
            xs = 0.5 * rng.standard_normal(n)
            nd, nz = [q[0] for q in particles], [q[1] for q in particles]
        else:
            ts, xs = pkg.prior.synthetic_series(512, seed=400 + s, shuffle=True)
            ts, xs = ts[:n].copy(), xs[:n].copy()
            nd, nz = pkg.prior.sample_particles(rng, 2, max_depth=3)
        series.append((ts, xs))
        nodes += list(nd); noises += list(nz); sidx += [s, s]
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), *series[s]) for nd, nz, s in zip(nodes, noises, sidx)])
    assert len(nodes) == 50 and np.isfinite(ref).all()
    lp, info = engine.logpdf_long_series_batch(series, nodes, noises, sidx, all_long=True, check=False)
    err = relerr(lp, ref)
    print("every block count: worst relative error", err.max(), "at n =", BLOCK_LENS[int(sidx[err.argmax()])])
    assert (info == 0).all()
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
    cases = [c for c in golden["cases"] if "logpdf" in c and len(c["ts"]) <= G.LONG_SERIES_MAX_N]
    assert len(cases) >= 20
    kinds = set()
    for c in cases:
        kinds |= {type(x).__name__ for x in G.unroll(G.from_tuple(to_tuple(c["tree"])))}
    assert {"Constant", "SquaredExponential", "WhiteNoise"} <= kinds
    series = [(np.array(c["ts"]), np.array(c["xs"])) for c in cases]
    nodes = [G.from_tuple(to_tuple(c["tree"])) for c in cases]
    noises = np.array([c["noise"] for c in cases])
    lp, info = engine.logpdf_long_series_batch(series, nodes, noises, np.arange(len(cases)), all_long=True)
    ref = np.array([c["logpdf"] for c in cases])
    print("golden cases, all_long: worst relative error", relerr(lp, ref).max(), "over", len(cases), "cases")
    assert (info == 0).all()
    bad = ~close(lp, ref)
    assert not bad.any(), [(cases[i]["name"], lp[i], ref[i]) for i in np.flatnonzero(bad)]

    # hand-written, at 300 points: nested ChangePoints, a 16-leaf tree (evaluation stack of depth 5: the D = 8 instantiation), a
    # GammaExponential on a series with a repeated time point (dt = 0 off the diagonal), Constant * WhiteNoise
    rng = np.random.default_rng(5)
    ts = rng.random(300); ts[241] = ts[7]
    xs = 0.5 * rng.standard_normal(300)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = full_tree(G, 4)
    assert deep.size() == 31
    nodes = [nested, deep, G.GammaExponential(0.42, 0.58, 3.2), G.Constant(0.5) * G.WhiteNoise(0.3)]
    noises = np.array([0.1, 0.2, 0.05, 0.3])
    lp, info = engine.logpdf_long_series_batch([(ts, xs)], nodes, noises, np.zeros(4, dtype=np.int32))
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), ts, xs) for nd, nz in zip(nodes, noises)])
    print("hand-written trees at 300 points: worst relative error", relerr(lp, ref).max())
    assert (info == 0).all() and np.isfinite(ref).all()
    assert close(lp, ref).all(), (lp, ref)


def test_agrees_with_resident_series_path(engine, ragged):
    series, nodes, noises, sidx, ref, (lp, info), _ = ragged
    worst = 0.0
    for n in (177, 257, 442, 512):
        s = LENS.index(n)
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        lp_res, info_res = engine.logpdf_batch([nodes[i] for i in sel], noises[sel])
        assert (info_res == 0).all()
        worst = max(worst, relerr(lp[sel], lp_res).max())
        assert close(lp[sel], lp_res).all(), (n, lp[sel], lp_res)
    print("long kernel against set_data + logpdf_batch: worst relative difference", worst)


def test_batch_independence_bitwise(pkg, engine, ragged):
    series, nodes, noises, sidx, ref, default, all_long = ragged
    P = len(nodes)
    rev = np.arange(P)[::-1]
    for flag, (lp, _) in ((False, default), (True, all_long)):
        call = functools.partial(engine.logpdf_long_series_batch, all_long=flag, check=False)
        again, _ = call(series, nodes, noises, sidx)                                   # the call repeated
        assert np.array_equal(bits(again), bits(lp)), flag
        lp_rev, _ = call(series, [nodes[i] for i in rev], noises[rev], sidx[rev])      # reversed particle order
        assert np.array_equal(bits(lp_rev), bits(lp[rev])), flag
        for s in range(len(series)):                                                   # one series per call
            sel = np.flatnonzero(sidx == s)
            one, _ = call([series[s]], [nodes[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32))
            assert np.array_equal(bits(one), bits(lp[sel])), (flag, s)
        # a workspace limit of 3 MiB: at most two 512-point factors (1.03 MiB each) per launch, so the four 512-point particles
        # and the rest of the long ones are spread over several launches on the call's stream
        engine.set_workspace_limit(3 << 20)
        try:
            split, info = call(series, nodes, noises, sidx)
        finally:
            engine.set_workspace_limit(0)
        assert (info == 0).all() and np.array_equal(bits(split), bits(lp)), flag


def test_bad_pivots_at_chosen_points(pkg, engine):
    """eighteen particles that stop being positive definite at a chosen point of one 512-point series — every side of the 4-wide
    sub-steps, of block, wave-round (64 rows) and short-cap boundaries, the last block, the last point — and a good particle among
    them, in one call: info is the pivot, NaN in that particle only"""
    ts = cp_ts()
    xs = np.random.default_rng(31).standard_normal(ts.size)
    good = pkg.SquaredExponential(0.3, 0.8)
    nodes = [changepoint_particle(pkg, k) for k in CP_POINTS]
    at = 7                                                       # the good particle sits between the failing ones
    nodes.insert(at, good)
    noises = np.full(len(nodes), CP_NOISE); noises[at] = 0.1
    lp, info = engine.logpdf_long_series_batch([(ts, xs)], nodes, noises, np.zeros(len(nodes), dtype=np.int32), check=False)
    assert np.delete(info, at).tolist() == [k + 1 for k in CP_POINTS], info
    assert np.isnan(np.delete(lp, at)).all()
    alone, info1 = engine.logpdf_long_series_batch([(ts, xs)], [good], [0.1], [0], check=False)
    assert info[at] == 0 and info1[0] == 0 and bits(alone)[0] == bits(lp)[at]
    assert close(lp[at], O.gp_logpdf(good.to_tuple(), 0.1, ts, xs))
    with pytest.raises(pkg.PosDefException) as ei:
        engine.logpdf_long_series_batch([(ts, xs)], nodes[at:at + 2], noises[at:at + 2], [0, 0], check=True)
    assert ei.value.particle == 1 and ei.value.info == CP_POINTS[at] + 1


def raw_call(engine, pt_off, ts, xs, sidx, programs, noises, flags=0):
    """the C entry itself on pre-filled outputs: (rc, message, out_logpdf, out_info)"""
    op_off, ops, prm_off, prm = programs
    P = len(noises)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int64); sidx = np.ascontiguousarray(sidx, dtype=np.int32)
    ts = np.ascontiguousarray(ts, dtype=np.float64); xs = np.ascontiguousarray(xs, dtype=np.float64)
    noises = np.ascontiguousarray(noises, dtype=np.float64)
    out = np.full(max(P, 1), 7.25); info = np.full(max(P, 1), -77, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = engine._lib.agp_logpdf_long_series_batch(engine._ctx, len(pt_off) - 1, pt_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), P, sidx.ctypes.data_as(ip),
                                                  op_off.ctypes.data_as(ip), ops.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp),
                                                  flags, out.ctypes.data_as(dp), info.ctypes.data_as(ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), out, info


def untouched(out, info):
    return (out == 7.25).all() and (info == -77).all()


def cp_chain(G, k):
    nd = G.Constant(0.5)
    for i in range(k):
        nd = G.ChangePoint(nd, G.Constant(0.3 + 0.01 * i), 0.1 + 0.8 * i / max(1, k - 1), 0.05)
    return nd


def test_capacity_and_refusals(pkg, engine):
    G = pkg
    N = G.LONG_SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    good = G.SquaredExponential(0.3, 0.8)
    # ten ChangePoint nodes at the cap: the short entry's capacity at its own cap
    fits = cp_chain(G, 10)
    lp, info = engine.logpdf_long_series_batch([(ts[:N], xs[:N])], [fits], [0.1], [0])
    want = O.gp_logpdf(fits.to_tuple(), 0.1, ts[:N], xs[:N])
    print("ten ChangePoint nodes at 512 points: relative error", relerr(lp[0], want))
    assert info[0] == 0 and close(lp[0], want)
    # forty (160 KiB of tables alone): AGP_ERR_PROGRAM, naming the particle
    progs = G.encode_batch([good, cp_chain(G, 40)])
    rc, msg, out, info = raw_call(engine, [0, N], ts[:N], xs[:N], [0, 0], progs, [0.1, 0.1])
    assert rc == -3 and "particle 1" in msg and "LDS" in msg and untouched(out, info), (rc, msg)
    # 513 points: AGP_ERR_ARG, naming the series, its length and the cap
    progs = G.encode_batch([good, good])
    rc, msg, out, info = raw_call(engine, [0, 5, 5 + N + 1], np.concatenate([ts[:5], ts]), np.concatenate([xs[:5], xs]), [0, 1], progs,
                                  [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and str(N + 1) in msg and "AGP_LONG_SERIES_MAX_N" in msg and untouched(out, info), (rc, msg)
    with pytest.raises(ValueError, match="series 0"):
        engine.logpdf_long_series_batch([(ts, xs)], [good], [0.1], [0])
    # an unknown flag bit
    rc, msg, out, info = raw_call(engine, [0, 20, 40], ts[:40], xs[:40], [0, 1], progs, [0.1, 0.1], flags=2)
    assert rc == -1 and "flag" in msg and untouched(out, info), (rc, msg)
    rc, msg, out, info = raw_call(engine, [0, 20, 40], ts[:40], xs[:40], [0, 1], progs, [0.1, 0.1], flags=1 | 4)
    assert rc == -1 and untouched(out, info), (rc, msg)
    # P == 0 touches nothing
    rc, msg, out, info = raw_call(engine, [0], ts[:1], xs[:1], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert rc == 0 and untouched(out, info)
    # ... and the entry still answers
    lp, info = engine.logpdf_long_series_batch([(ts[:200], xs[:200])], [good], [0.1], [0])
    assert info[0] == 0 and close(lp[0], O.gp_logpdf(good.to_tuple(), 0.1, ts[:200], xs[:200]))


def test_stateless(pkg, ragged):
    series, nodes, noises, sidx, ref, (lp, _), _ = ragged
    eng = pkg.GPEngine(0)
    try:
        # a fresh engine on which set_data was never called
        lp0, info0 = eng.logpdf_long_series_batch(series, nodes, noises, sidx, check=False)
        assert np.array_equal(bits(lp0), bits(lp)) and (info0 == 0).all()
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)      # (with copies: dedup counts them)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max)
        before = snapshot()
        lp1, _ = eng.logpdf_long_series_batch(series, nodes, noises, sidx, check=False)
        assert np.array_equal(bits(lp1), bits(lp))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        # the store still holds its factors: a longer prefix extends them
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_concurrent_callers(engine, ragged):
    """four threads, each with its own ragged family (the shared series rotated, every thread its own flag), against the serial call"""
    series, nodes, noises, sidx, ref, _, _ = ragged
    S_ = len(series)

    def family(i):
        order = [(s + 4 * i) % S_ for s in range(S_)]               # thread i's series list: the shared one rotated by 4 i
        where = {s: j for j, s in enumerate(order)}
        return [series[s] for s in order], np.array([where[int(s)] for s in sidx], dtype=np.int32), bool(i % 2)

    fams = [family(i) for i in range(4)]
    serial = [engine.logpdf_long_series_batch(f[0], nodes, noises, f[1], all_long=f[2], check=False)[0] for f in fams]
    out = [None] * 4

    def work(i):
        out[i] = engine.logpdf_long_series_batch(fams[i][0], nodes, noises, fams[i][1], all_long=fams[i][2], check=False)[0]

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for o, want in zip(out, serial):
        assert o is not None and np.array_equal(bits(o), bits(want))
