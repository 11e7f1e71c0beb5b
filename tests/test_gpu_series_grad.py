"""GPU tests of agp_logpdf_grad_series_batch (value and gradient of many short series in one fused launch; k_series_logpdf_grad,
csrc/agp_series_kernel.hpp): parity with the oracle on ragged input — values to |d| <= 1e-8 max(1, |logpdf|), every gradient component
to 1e-7 of its own scale S_k (oracle/gradcheck.py; a miss goes to the 80-bit arbiter) — at every block count, on the kernels where small
components live and on hand-written trees; value bits equal to agp_logpdf_series_batch's; agreement with the resident-series path;
batch independence (bitwise); statelessness; non-PD reporting at every sub-step; argument errors; concurrent callers.
No particle is skipped anywhere: info == 0 and an oracle reference for every particle, unless the test is about failure."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import _series_cases as S
import _series_grad_ref as R
import test_gpu_series as TS
from test_gpu_grad_components import small_kernels, irregular_series
from oracle import gradcheck as GC
from oracle import oracle as O

pytestmark = pytest.mark.gpu
close, bits = TS.close, TS.bits


def gbits(res):
    """every output of a call as one int64 vector: logpdf, gradients, d/dnoise (bit patterns), info"""
    lp, g, gn, info = res
    return np.concatenate([bits(lp)] + [bits(x) for x in g] + [bits(gn), np.asarray(info, dtype=np.int64)])


def take(res, sel):
    lp, g, gn, info = res
    return lp[sel], [g[i] for i in sel], gn[sel], info[sel]


def check_population(name, res, series, nodes, noises, sidx, refs):
    """values and every gradient component of every particle against the oracle; returns the worst accepted |g_k - ref_k| / S_k"""
    lp, g, gn, info = res
    assert (info == 0).all(), (name, info)
    assert all(r is not None for r in refs), name
    fails, worst = [], 0.0
    for i, r in enumerate(refs):
        if not close(lp[i], r.lp):
            fails.append(f"{name} particle {i}: logpdf {lp[i]} vs {r.lp}")
        try:
            worst = max(worst, GC.assert_grad_components(g[i], gn[i], r, tau=GC.TAU_ORACLE, ctx=(name, i, r.tree, r.noise, r.n),
                                                         particle_wide=False))
        except AssertionError as e:
            fails.append(str(e))
    print(f"[series-grad] {name}: worst |g_k - ref_k| / S_k = {worst:.3e} over {len(refs)} particles")
    assert not fails, "\n".join(fails)
    return worst


def population_refs(series, nodes, noises, sidx):
    out = [None] * len(nodes)
    for s in sorted(set(int(x) for x in sidx)):
        sel = [i for i in range(len(nodes)) if sidx[i] == s]
        if len(series[s][0]) == 0:
            continue
        for i, r in zip(sel, GC.references([nodes[i] for i in sel], [noises[i] for i in sel], *series[s])):
            out[i] = r
    return out


@functools.lru_cache(maxsize=None)
def ragged_refs():
    series, nodes, noises, sidx, _ = TS.ragged_case()
    return population_refs(series, nodes, noises, sidx)


@pytest.fixture(scope="module")
def ragged(engine):
    """test_gpu_series.ragged_case() (the population known to factor) through the new entry, once"""
    series, nodes, noises, sidx, ref_lp = TS.ragged_case()
    res = engine.logpdf_grad_series_batch(series, nodes, noises, sidx, check=False)
    for a in (res[0], res[2], res[3], *res[1]):
        a.setflags(write=False)
    return series, nodes, noises, sidx, ref_lp, res


def test_ragged_parity(pkg, ragged):
    series, nodes, noises, sidx, ref_lp, res = ragged
    lp, g, gn, info = res
    assert [len(t) for t, _ in series] == [0, 1, 2, 15, 16, 17, 33, 126, 144, pkg.SERIES_MAX_N] and len(nodes) == 60
    assert (info == 0).all() and close(lp, ref_lp).all()
    empty = np.flatnonzero(sidx == 0)
    assert (lp[empty] == 0.0).all() and (gn[empty] == 0.0).all() and all((g[i] == 0.0).all() for i in empty)
    for i in range(len(nodes)):
        assert g[i].shape == (pkg.encode(nodes[i])[1].size,)
    keep = np.flatnonzero(sidx != 0)
    refs = [ragged_refs()[i] for i in keep]
    check_population("ragged", take(res, keep), series, nodes, noises, sidx, refs)


def test_parity_at_the_remaining_block_counts(pkg, engine):
    lens = (49, 80, 81, 97, 112, 145, 161)
    rng = np.random.default_rng(20261019)
    series, nodes, noises, sidx = [], [], [], []
    for s, n in enumerate(lens):
        ts, xs = pkg.prior.synthetic_series(256, seed=200 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        nd, nz = pkg.prior.sample_particles(rng, 6, max_depth=3)
        nodes += nd; noises += list(nz); sidx += [s] * 6
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    res = engine.logpdf_grad_series_batch(series, nodes, noises, sidx, check=False)
    assert len(nodes) == 42
    check_population("block counts", res, series, nodes, noises, sidx, population_refs(series, nodes, noises, sidx))


@pytest.mark.parametrize("n", [2, 17, 48, 176])
def test_small_components(pkg, engine, n):
    """a duplicated time, gamma near 0.05 and 2, a period below the spacing, a ChangePoint on a point at scale 1e-3, Linear products of
    degree 1-4, noise from 1e-5 up

    (n = 48, particle 12 — the ChangePoint on a point at scale 1e-3 — is the case the complement tables of the kernel are for: every
    term of its derivative by the scale comes from points at |loc - t| / scale >= 13.7, and with 1 - sigma subtracted from the rounded
    sigma that component was 4.4e-7 S_k off the oracle.)"""
    ts, xs = irregular_series(n, seed=1000 + n)
    kernels, noises = small_kernels(pkg, ts, duplicates=True)
    sidx = np.zeros(len(kernels), dtype=np.int32)
    res = engine.logpdf_grad_series_batch([(ts, xs)], kernels, noises, sidx, check=False)
    check_population(f"small components n={n}", res, [(ts, xs)], kernels, noises, sidx,
                     population_refs([(ts, xs)], kernels, noises, sidx))


def test_hand_written_trees(pkg, engine):
    """nested ChangePoints, the 31-node tree (tape of 64 nodes, evaluation stack of depth 5), a GammaExponential on a repeated time"""
    G = pkg
    rng = np.random.default_rng(5)
    ts = rng.random(70); ts[41] = ts[7]
    xs = 0.5 * rng.standard_normal(70)
    nested = G.ChangePoint(G.ChangePoint(G.Linear(0.1, 1.3, 0.7), G.Periodic(0.96, 0.21, 1.1), 0.3, 0.05),
                           G.SquaredExponential(0.47, 0.13) + G.WhiteNoise(0.2), 0.6, 0.1)
    deep = TS.full_tree(G, 4)
    assert deep.size() == 31
    wide = TS.full_tree(G, 3) + TS.full_tree(G, 2, 1)      # 15 + 1 + 7 = 23 nodes, stack depth 4: the tape-64 / depth-4 instantiation
    assert wide.size() == 23
    nodes = [nested, deep, G.GammaExponential(0.42, 0.58, 3.2), G.Constant(0.5) * G.WhiteNoise(0.3), wide]
    noises = np.array([0.1, 0.2, 0.05, 0.3, 0.15])
    sidx = np.zeros(len(nodes), dtype=np.int32)
    res = engine.logpdf_grad_series_batch([(ts, xs)], nodes, noises, sidx, check=False)
    check_population("hand-written", res, [(ts, xs)], nodes, noises, sidx, population_refs([(ts, xs)], nodes, noises, sidx))
    lp_v, info_v = engine.logpdf_series_batch([(ts, xs)], nodes, noises, sidx, check=False)
    assert np.array_equal(bits(lp_v), bits(res[0])) and np.array_equal(info_v, res[3])


def test_tree_of_65_nodes_is_refused(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(20, seed=4)
    good = G.SquaredExponential(0.3, 0.8)
    big = G.Constant(0.1)
    for i in range(32):
        big = big + G.Constant(0.1 + 0.01 * i)
    assert big.size() == 65
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*64 nodes"):
        engine.logpdf_grad_series_batch([(ts, xs)], [good, big], [0.1, 0.1], [0, 0])
    lp, g, gn, info = engine.logpdf_grad_series_batch([(ts, xs)], [good], [0.1], [0])
    ref = GC.reference(good.to_tuple(), 0.1, ts, xs)
    assert info[0] == 0 and close(lp[0], ref.lp)
    GC.assert_grad_components(g[0], gn[0], ref, tau=GC.TAU_ORACLE, particle_wide=False)
    # the largest tape: 63 nodes pass
    full = TS.full_tree(G, 5)
    assert full.size() == 63
    res = engine.logpdf_grad_series_batch([(ts, xs)], [full], [0.2], [0], check=False)
    check_population("63 nodes", res, [(ts, xs)], [full], [0.2], [0], population_refs([(ts, xs)], [full], [0.2], [0]))


def test_value_bits_are_the_value_entry_s(engine, ragged):
    series, nodes, noises, sidx, ref_lp, res = ragged
    lp_v, info_v = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)
    assert np.array_equal(bits(lp_v), bits(res[0])) and np.array_equal(info_v, res[3])


def test_agrees_with_resident_series_path(engine, ragged):
    series, nodes, noises, sidx, ref_lp, res = ragged
    worst = 0.0
    for s in (5, 7, 8):                                          # 17, 126 and 144 points
        sel = np.flatnonzero(sidx == s)
        engine.set_data(*series[s])
        lp_r, g_r, gn_r, info_r = engine.logpdf_grad_batch([nodes[i] for i in sel], noises[sel], check=False)
        assert (info_r == 0).all() and close(res[0][sel], lp_r).all()
        for k, i in enumerate(sel):
            r = ragged_refs()[i]
            assert r is not None
            worst = max(worst, GC.assert_grad_components(res[1][i], res[2][i], r, tau=GC.TAU_ORACLE, against=(g_r[k], gn_r[k]),
                                                         ctx=("resident", s, i), particle_wide=False))
    print(f"[series-grad] fused entry vs set_data + logpdf_grad_batch: worst |delta| / S_k = {worst:.3e}")


def test_batch_independence_bitwise(engine, ragged):
    series, nodes, noises, sidx, ref_lp, res = ragged
    P = len(nodes)
    rev = np.arange(P)[::-1]
    r_rev = engine.logpdf_grad_series_batch(series, [nodes[i] for i in rev], noises[rev], sidx[rev], check=False)
    assert np.array_equal(gbits(r_rev), gbits(take(res, rev)))
    for s in range(len(series)):                                 # one series at a time
        sel = np.flatnonzero(sidx == s)
        one = engine.logpdf_grad_series_batch([series[s]], [nodes[i] for i in sel], noises[sel], np.zeros(len(sel), dtype=np.int32),
                                              check=False)
        assert np.array_equal(gbits(one), gbits(take(res, sel))), s
    for p in range(P):                                           # each particle alone
        one = engine.logpdf_grad_series_batch([series[sidx[p]]], [nodes[p]], noises[p:p + 1], [0], check=False)
        assert np.array_equal(gbits(one), gbits(take(res, [p]))), p


def test_stateless(pkg, ragged):
    series, nodes, noises, sidx, ref_lp, res = ragged
    eng = pkg.GPEngine(0)
    try:
        # a fresh engine on which set_data was never called
        r0 = eng.logpdf_grad_series_batch(series, nodes, noises, sidx, check=False)
        assert np.array_equal(gbits(r0), gbits(res))
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)      # (with copies: dedup counts them)
        gres0 = eng.logpdf_grad_batch(rn, rz, check=False)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max,
                    eng.grad_reuse_stats(), eng.grad_lag_domain_particles(), eng.grad_toeplitz_particles(),
                    eng.grad_structured_particles())
        before = snapshot()
        r1 = eng.logpdf_grad_series_batch(series, nodes, noises, sidx, check=False)
        assert np.array_equal(gbits(r1), gbits(res))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        gres1 = eng.logpdf_grad_batch(rn, rz, check=False)
        assert np.array_equal(gbits(gres1), gbits(gres0))
        # the store still holds its factors: a longer prefix extends them
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_non_positive_definite(pkg, engine):
    G = pkg
    ts, xs = G.prior.synthetic_series(40, seed=2)
    bad = G.Constant(1.0)
    good, good2 = G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.3, 0.9) + G.Linear(0.2, 0.3, 0.4)
    first = S.first_bad_minor(O.compute_cov_matrix_vectorized(bad.to_tuple(), -0.5, ts))
    assert first == 2
    res = engine.logpdf_grad_series_batch([(ts, xs)], [good, bad, good2], [0.1, -0.5, 0.2], [0, 0, 0], check=False)
    lp, g, gn, info = res
    assert info.tolist() == [0, first, 0]
    assert np.isnan(lp[1]) and np.isnan(gn[1]) and g[1].shape == (1,) and np.isnan(g[1]).all()
    for i, (nd, nz) in ((0, (good, 0.1)), (2, (good2, 0.2))):
        alone = engine.logpdf_grad_series_batch([(ts, xs)], [nd], [nz], [0], check=False)
        assert alone[3][0] == 0 and np.array_equal(gbits(alone), gbits(take(res, [i])))
        ref = GC.reference(nd.to_tuple(), nz, ts, xs)
        assert close(lp[i], ref.lp)
        GC.assert_grad_components(g[i], gn[i], ref, tau=GC.TAU_ORACLE, particle_wide=False)
    with pytest.raises(G.PosDefException) as ei:
        engine.logpdf_grad_series_batch([(ts, xs), (ts, xs)], [good, bad], [0.1, -0.5], [0, 1], check=True)
    assert ei.value.particle == 1 and ei.value.info == first


def test_info_at_every_sub_step_and_block(pkg, engine):
    """thirteen particles that stop being positive definite at a chosen point of one 176-point series, a good particle among them: info
    at every 4-wide sub-step and block boundary, NaN in every failed particle's outputs, the good one's gradient against the oracle"""
    ts = S.CP_TS
    xs = np.random.default_rng(31).standard_normal(ts.size)
    good = pkg.SquaredExponential(0.3, 0.8)
    nodes = [S.changepoint_particle(pkg, k) for k in S.CP_POINTS]
    first = [k + 1 for k in S.CP_POINTS]
    at = 6
    nodes.insert(at, good)
    noises = np.full(len(nodes), S.CP_NOISE); noises[at] = 0.1
    lp, g, gn, info = engine.logpdf_grad_series_batch([(ts, xs)], nodes, noises, np.zeros(len(nodes), dtype=np.int32), check=False)
    assert np.delete(info, at).tolist() == first, info
    for i in range(len(nodes)):
        if i == at:
            continue
        assert np.isnan(lp[i]) and np.isnan(gn[i]) and g[i].size > 0 and np.isnan(g[i]).all(), i
    assert info[at] == 0 and np.isfinite(lp[at]) and np.isfinite(gn[at]) and np.isfinite(g[at]).all()
    ref = GC.reference(good.to_tuple(), 0.1, ts, xs)
    assert close(lp[at], ref.lp)
    GC.assert_grad_components(g[at], gn[at], ref, tau=GC.TAU_ORACLE, particle_wide=False)
    alone = engine.logpdf_grad_series_batch([(ts, xs)], [good], [0.1], [0], check=False)
    assert np.array_equal(gbits(alone), gbits((lp[[at]], [g[at]], gn[[at]], info[[at]])))


def raw_call(engine, pt_off, ts, xs, sidx, programs, noises, null_grad=False, null_gnoise=False):
    op_off, ops, prm_off, prm = programs
    P = len(noises)
    pt_off = np.ascontiguousarray(pt_off, dtype=np.int64); sidx = np.ascontiguousarray(sidx, dtype=np.int32)
    ts = np.ascontiguousarray(ts, dtype=np.float64); xs = np.ascontiguousarray(xs, dtype=np.float64)
    noises = np.ascontiguousarray(noises, dtype=np.float64)
    out = np.full(P, 7.0); info = np.full(P, 7, dtype=np.int32); gn = np.full(P, 7.0)
    grad = np.full(max(1, int(prm_off[-1]) if len(prm_off) else 1), 7.0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = engine._lib.agp_logpdf_grad_series_batch(engine._ctx, len(pt_off) - 1, pt_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), P, sidx.ctypes.data_as(ip),
                                                  op_off.ctypes.data_as(ip), ops.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp), noises.ctypes.data_as(dp),
                                                  out.ctypes.data_as(dp), None if null_grad else grad.ctypes.data_as(dp),
                                                  None if null_gnoise else gn.ctypes.data_as(dp), info.ctypes.data_as(ip))
    msg = engine._lib.agp_last_error(engine._ctx)
    return rc, (msg.decode() if msg else ""), out, grad, gn, info


def test_errors_name_the_culprit(pkg, engine):
    G = pkg
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N + 1, seed=4)
    good = G.SquaredExponential(0.3, 0.8)
    progs = G.encode_batch([good, good])
    ref20 = GC.reference(good.to_tuple(), 0.1, ts[:20], xs[:20])

    def valid():
        lp, g, gn, info = engine.logpdf_grad_series_batch([(ts[:20], xs[:20])], [good], [0.1], [0])
        assert info[0] == 0 and close(lp[0], ref20.lp)
        GC.assert_grad_components(g[0], gn[0], ref20, tau=GC.TAU_ORACLE, particle_wide=False)

    with pytest.raises(G.AGPError, match=r"particle 1.*series index 3"):
        engine.logpdf_grad_series_batch([(ts[:20], xs[:20]), (ts[:9], xs[:9])], [good, good], [0.1, 0.1], [0, 3])
    valid()
    with pytest.raises(G.AGPError, match=r"particle 0.*series index -1"):
        engine.logpdf_grad_series_batch([(ts[:20], xs[:20])], [good], [0.1], [-1])
    rc, msg, *_ = raw_call(engine, [0, 30, 20], ts[:30], xs[:30], [0, 1], progs, [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and "decreases" in msg
    valid()
    rc, msg, *_ = raw_call(engine, [0, 5, 5 + N + 1], np.tile(ts, 2), np.tile(xs, 2), [0, 1], progs, [0.1, 0.1])
    assert rc == -1 and "series 1" in msg and str(N + 1) in msg
    rc, msg, *_ = raw_call(engine, [1, 5], ts[:5], xs[:5], [0, 0], progs, [0.1, 0.1])
    assert rc == -1 and "pt_off[0]" in msg
    with pytest.raises(ValueError, match="series 0"):
        engine.logpdf_grad_series_batch([(ts, xs)], [good], [0.1], [0])
    valid()
    # null gradient outputs: out_grad with parameters present, out_grad_noise always
    rc, msg, *_ = raw_call(engine, [0, 20], ts[:20], xs[:20], [0, 0], progs, [0.1, 0.1], null_grad=True)
    assert rc == -1 and "out_grad" in msg
    rc, msg, *_ = raw_call(engine, [0, 20], ts[:20], xs[:20], [0, 0], progs, [0.1, 0.1], null_gnoise=True)
    assert rc == -1 and "out_grad_noise" in msg
    valid()
    # a malformed program: particle 1 is a lone '+'
    op_off, ops, prm_off, prm = G.encode_batch([good])
    bad_prog = (np.array([0, ops.size, ops.size + 1], dtype=np.int32), np.concatenate([ops, np.array([6], dtype=np.uint8)]),
                np.array([0, prm.size, prm.size], dtype=np.int32), prm)
    rc, msg, *_ = raw_call(engine, [0, 20], ts[:20], xs[:20], [0, 0], bad_prog, [0.1, 0.1])
    assert rc == -3 and "particle 1" in msg and "underflow" in msg
    valid()
    # per-point tables beyond the LDS budget at the cap, counted from the gradient kernel's own map: the longest chain of
    # ChangePoints that fits is scored, one more is refused — and fits a 100-point series
    k_fit = max(k for k in range(1, 40) if R.cp_chain_fits(k, N, grad=True))
    assert k_fit < max(k for k in range(1, 40) if R.cp_chain_fits(k, N, grad=False))
    fits, too_many = TS.cp_chain(G, k_fit), TS.cp_chain(G, k_fit + 1)
    res = engine.logpdf_grad_series_batch([(ts[:N], xs[:N])], [fits], [0.1], [0])
    check_population("ChangePoint chain at the cap", res, None, [fits], [0.1], [0], [GC.reference(fits.to_tuple(), 0.1, ts[:N], xs[:N])])
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*LDS"):
        engine.logpdf_grad_series_batch([(ts[:N], xs[:N])], [good, too_many], [0.1, 0.1], [0, 0])
    res = engine.logpdf_grad_series_batch([(ts[:100], xs[:100])], [too_many], [0.1], [0])
    check_population("ChangePoint chain at 100 points", res, None, [too_many], [0.1], [0],
                     [GC.reference(too_many.to_tuple(), 0.1, ts[:100], xs[:100])])
    # P == 0 touches nothing
    rc, msg, out, grad, gn, info = raw_call(engine, [0], ts[:1], xs[:1], np.zeros(0, dtype=np.int32), G.encode_batch([]), np.zeros(0))
    assert rc == 0 and (grad == 7.0).all()
    valid()


def test_concurrent_callers(engine, ragged):
    series, nodes, noises, sidx, ref_lp, res = ragged
    out = [None] * 4

    def work(i):
        out[i] = engine.logpdf_grad_series_batch(series, nodes, noises, sidx, check=False)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for o in out:
        assert o is not None and np.array_equal(gbits(o), gbits(res))
