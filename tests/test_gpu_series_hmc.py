"""GPU tests of agp_hmc_series_batch (in-kernel HMC rejuvenation of many short series; k_series_hmc, csrc/agp_series_kernel.hpp) on the
cases of tests/golden/series_hmc_v1.json (generator beside it): chain parity with the fp64 reference — every accept decision equal, z,
z_noise, alpha and logpdf within the case's MEASURED tolerance; out_logpdf bit-identical to the value entry on (out_prm, out_noise); fixed
slots and, with L_noise = 0, the noise bit-identical to the input; energy consistency without a reference; batch independence (bitwise);
n_exit; not positive definite, at the start and on a trajectory; errors that name the culprit; statelessness; agreement with the host
route (a Python loop over logpdf_grad_series_batch with the same draws).  No admitted case is skipped."""
import ctypes as C
import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest

import _series_hmc_ref as H
import test_gpu_series as TS

pytestmark = pytest.mark.gpu
bits = TS.bits
GOLD = json.loads((Path(__file__).parent / "golden" / "series_hmc_v1.json").read_text())
TF = np.array(GOLD["tf"])
CASES = {c["name"]: c for c in GOLD["cases"]}


def to_node(G, t):
    return G.from_tuple(tuple_tree(t))


def tuple_tree(t):
    return tuple(tuple_tree(v) if isinstance(v, list) else v for v in t)


def call(engine, G, cases, want_trace=True, order=None, seeds=None, **over):
    """the cases as ONE call (they share a schedule); returns the engine's namespace"""
    order = list(range(len(cases))) if order is None else order
    cs = [cases[i] for i in order]
    kw = dict(cs[0]["sched"]); kw.update(over)
    series = [(np.array(c["ts"]), np.array(c["xs"])) for c in cs]
    return engine.hmc_series_batch(series, [to_node(G, c["tree"]) for c in cs], [c["z"] for c in cs], [c["z_noise"] for c in cs],
                                   [c["cls"] for c in cs], TF, np.arange(len(cs)), kw["n_hmc"],
                                   [c["seed"] for c in cs] if seeds is None else seeds, noise_jitter=cs[0].get("jitter", 1e-5),
                                   L_param=kw["L_param"], eps_param=kw["eps_param"], L_noise=kw["L_noise"], eps_noise=kw["eps_noise"],
                                   n_exit=kw.get("n_exit"), want_trace=want_trace, check=False)


def rbits(r, sel=None):
    sel = range(len(r.z)) if sel is None else sel
    parts = []
    for i in sel:
        parts += [bits(r.z[i]), bits(r.prm[i]), bits(r.z_noise[i:i + 1]), bits(r.noise[i:i + 1]), bits(r.logpdf[i:i + 1]),
                  r.counts[i].astype(np.int64), r.info[i:i + 1].astype(np.int64)]
        if r.trace is not None:
            parts.append(bits(r.trace[i].ravel()))
    return np.concatenate(parts)


def decisions(trace):
    return [[None if math.isnan(m[1]) else bool(m[1] < m[0]) for m in row] for row in np.asarray(trace).tolist()]


def check_chain(name, c, r, i, tol):
    e = c["expect"]
    tr = r.trace[i]
    assert r.info[i] == 0, (name, r.info[i])
    assert decisions(tr) == decisions(e["trace"]), (name, tr.tolist(), e["trace"])
    assert r.counts[i].tolist() == e["counts"], (name, r.counts[i], e["counts"])
    dev = [np.abs(r.z[i] - np.array(e["z"])).max(), abs(r.z_noise[i] - e["z_noise"]), abs(r.logpdf[i] - e["logpdf"])]
    for ra, rb in zip(tr.tolist(), e["trace"]):
        for ma, mb in zip(ra, rb):
            if math.isnan(mb[1]):
                assert math.isnan(ma[0]) and math.isnan(ma[1]), name
                continue
            assert abs(ma[1] - mb[1]) <= 1e-14 * max(1.0, abs(mb[1])), (name, "log u", ma, mb)
            if math.isfinite(mb[0]):
                dev.append(abs(ma[0] - mb[0]))
            else:
                assert ma[0] == mb[0], (name, ma, mb)
    print(f"[series-hmc] {name}: worst deviation {max(dev):.3e} (tolerance {tol:.3e})")
    assert max(dev) <= tol, (name, dev, tol)
    return max(dev)


@functools.lru_cache(maxsize=None)
def short_cases():
    return tuple(c for c in GOLD["cases"] if c["sched"]["n_hmc"] == 3)


@pytest.fixture(scope="module")
def short_run(pkg, engine):
    """the n_hmc = 3, L = 3 cases (n = 1, 15, 16, 17, 33, 49, 176) in one call, once"""
    return call(engine, pkg, list(short_cases()))


def test_chain_parity_short(pkg, short_run):
    cs = short_cases()
    assert sorted(c["n"] for c in cs) == [1, 15, 16, 17, 33, 49, 176]
    for i, c in enumerate(cs):
        check_chain(c["name"], c, short_run, i, c["tol"])


@pytest.mark.parametrize("name", ["defaults_n144", "tiny_se_n12", "tiny_ge_plus_lin_n24"])
def test_chain_parity_other_schedules(pkg, engine, name):
    c = CASES[name]
    if name == "defaults_n144":
        assert (c["sched"]["n_hmc"], c["sched"]["L_param"], c["sched"]["L_noise"], c["sched"]["eps_param"]) == (10, 10, 10, 0.02)
    check_chain(name, c, call(engine, pkg, [c]), 0, c["tol"])


def test_logpdf_bits_fixed_slots_and_frozen_noise(pkg, engine, short_run):
    G = pkg
    cs = short_cases()
    nodes = [G.with_params(to_node(G, c["tree"]), short_run.prm[i]) for i, c in enumerate(cs)]
    series = [(np.array(c["ts"]), np.array(c["xs"])) for c in cs]
    lp, info = engine.logpdf_series_batch(series, nodes, short_run.noise, np.arange(len(cs)))
    assert (info == 0).all() and np.array_equal(bits(lp), bits(short_run.logpdf))
    moved = 0
    for i, c in enumerate(cs):
        cls = np.array(c["cls"]); z0 = np.array(c["z"])
        fixed = cls < 0
        assert np.array_equal(bits(short_run.z[i][fixed]), bits(z0[fixed])) and np.array_equal(bits(short_run.prm[i][fixed]), bits(z0[fixed]))
        moved += int(fixed.sum())
        for k in np.flatnonzero(~fixed):
            assert abs(short_run.prm[i][k] - G.prior.hmc_transform(short_run.z[i][k], cls[k], TF)) <= 1e-14 * abs(short_run.prm[i][k])
    assert moved == 4      # the ChangePoint chain's four scales
    r0 = call(engine, G, list(cs), L_noise=0)
    assert np.array_equal(bits(r0.z_noise), bits(np.array([c["z_noise"] for c in cs]))) and (r0.counts[:, 2] == 0).all()
    assert np.isnan(r0.trace[:, :, 1, :]).all() and not np.isnan(r0.trace[:, :, 0, :]).any()
    lp0, _ = engine.logpdf_series_batch(series, [G.with_params(to_node(G, c["tree"]), r0.prm[i]) for i, c in enumerate(cs)], r0.noise,
                                        np.arange(len(cs)))
    assert np.array_equal(bits(lp0), bits(r0.logpdf))


def test_energy_consistency(pkg, engine):
    """no reference involved: halving eps over the same trajectory length (twice the steps) must divide the first move's energy error
    by about four — the leapfrog scheme is of second order (a wrong chain rule or transform derivative leaves a first-order term: a
    ratio near 2).  Cases chosen on the CPU: the reference's own ratio lies in [3.5, 4.5]."""
    cs = [c for c in GOLD["cases"] if c["energy"] and c["sched"]["n_hmc"] == 3]
    assert len(cs) >= 3
    a1 = call(engine, pkg, cs, n_hmc=1).trace[:, 0, 0, 0]
    a2 = call(engine, pkg, cs, n_hmc=1, eps_param=cs[0]["sched"]["eps_param"] / 2, L_param=2 * cs[0]["sched"]["L_param"]).trace[:, 0, 0, 0]
    for c, x, y in zip(cs, a1, a2):
        print(f"[series-hmc] energy {c['name']}: alpha(eps) / alpha(eps/2) = {x / y:.4f} (reference {c['alpha_ratio_ref']:.4f})")
        assert 3.0 <= x / y <= 5.0, (c["name"], x, y)


def test_batch_independence_bitwise(pkg, engine, short_run):
    cs = list(short_cases())
    P = len(cs)
    rev = list(range(P))[::-1]
    r_rev = call(engine, pkg, cs, order=rev)
    assert np.array_equal(rbits(r_rev), rbits(short_run, rev))
    for i in range(P):
        one = call(engine, pkg, cs, order=[i])
        assert np.array_equal(rbits(one), rbits(short_run, [i])), cs[i]["name"]
    two = call(engine, pkg, cs, order=[2, 2])
    assert np.array_equal(rbits(two, [0]), rbits(two, [1])) and np.array_equal(rbits(two, [0]), rbits(short_run, [2]))
    other = call(engine, pkg, cs, order=[2], seeds=[cs[2]["seed"] + 1])
    assert not np.array_equal(bits(other.z[0]), bits(short_run.z[2]))


def test_n_exit(pkg, engine):
    c = GOLD["exit_case"]
    r = call(engine, pkg, [c])
    e = c["expect"]
    assert r.counts[0].tolist() == e["counts"] and r.counts[0][:2].tolist() == [0, 2]
    assert decisions(r.trace[0]) == decisions(e["trace"])
    tr = r.trace[0]
    assert np.isnan(tr[2:]).all() and not np.isnan(tr[:2, :, 1]).any()      # iterations 2 .. 4 were never made; both moves of 0 and 1 were
    for ra, rb in zip(tr[:2].tolist(), e["trace"][:2]):
        for ma, mb in zip(ra, rb):
            assert abs(ma[1] - mb[1]) <= 1e-14 * max(1.0, abs(mb[1]))
            assert (ma[0] == mb[0]) if not math.isfinite(mb[0]) else abs(ma[0] - mb[0]) <= 1e-9 * max(1.0, abs(mb[0])), (ma, mb)
    assert np.array_equal(bits(r.z[0]), bits(np.array(c["z"])))      # every parameter move was rejected
    never = call(engine, pkg, [c], n_exit=0)
    assert never.counts[0][1] == c["sched"]["n_hmc"] and not np.isnan(never.trace[0][:, 0, 1]).any()


def test_not_positive_definite(pkg, engine):
    G = pkg
    # a trajectory that leaves the positive definite region: rejected, counted, the state unchanged
    c = GOLD["notpd_case"]
    r = call(engine, G, [c])
    e = c["expect"]
    assert r.info[0] == 0 and r.counts[0].tolist() == e["counts"] and e["counts"][3] >= 1
    assert decisions(r.trace[0]) == decisions(e["trace"])
    lost = [(i, mv) for i, row in enumerate(e["trace"]) for mv, m in enumerate(row) if m[0] == -math.inf]
    assert lost and all(r.trace[0][i, mv, 0] == -math.inf for i, mv in lost)
    assert abs(r.z_noise[0] - e["z_noise"]) <= 1e-9 and np.abs(r.z[0] - np.array(e["z"])).max() <= 1e-9
    if e["counts"][2] == 0:
        assert np.array_equal(bits(r.z_noise), bits(np.array([c["z_noise"]])))
    # an initial state with a bad pivot (a rank-one kernel under a negative noise): info = the pivot, NaN, the inputs back, no move;
    # its neighbours are untouched
    ts, xs = G.prior.synthetic_series(40, seed=2)
    good, bad = G.SquaredExponential(1, 1), G.Constant(1)
    kw = dict(n_hmc=2, seeds=[5, 6, 7], noise_jitter=-0.75, L_param=2, L_noise=2, want_trace=True, check=False)
    z = [[0.1, -0.2], [math.log(1.0) + 1.5], [0.3, 0.1]]
    zn = [2.0, -1.0, 2.0]
    cls = [[0, 0], [0], [0, 0]]
    r = engine.hmc_series_batch([(ts, xs)], [good, bad, good], z, zn, cls, TF, [0, 0, 0], **kw)
    assert r.info.tolist() == [0, 2, 0] and np.isnan(r.logpdf[1]) and (r.counts[1] == 0).all() and np.isnan(r.trace[1]).all()
    assert np.array_equal(bits(r.z[1]), bits(np.array(z[1]))) and bits(r.z_noise[1:2])[0] == bits(np.array([-1.0]))[0]
    assert abs(r.prm[1][0] - 1.0) < 1e-12 and abs(r.noise[1] - (math.exp(-2.5) - 0.75)) < 1e-12
    kw["seeds"] = [5, 7]
    alone = engine.hmc_series_batch([(ts, xs)], [good, good], [z[0], z[2]], [2.0, 2.0], [cls[0], cls[2]], TF, [0, 0], **kw)
    assert np.array_equal(rbits(alone), rbits(r, [0, 2])) and (r.counts[[0, 2], 1] == 2).all()
    with pytest.raises(G.PosDefException) as ei:
        kw["seeds"] = [5, 6, 7]; kw["check"] = True
        engine.hmc_series_batch([(ts, xs)], [good, bad, good], z, zn, cls, TF, [0, 0, 0], **kw)
    assert ei.value.particle == 1 and ei.value.info == 2


def test_errors_name_the_culprit(pkg, engine):
    G = pkg
    N = G.SERIES_MAX_N
    ts, xs = G.prior.synthetic_series(N, seed=4)
    good = G.SquaredExponential(1, 1)
    base = dict(n_hmc=1, L_param=1, L_noise=1, check=False)

    def run(nodes, n=20, **kw):
        cls = [G.prior.hmc_classes(nd) for nd in nodes]
        z = [np.where(k >= 0, 0.1, 0.05) for k in cls]
        a = dict(base); a.update(kw)
        cls = a.pop("cls", cls)
        return engine.hmc_series_batch([(ts[:n], xs[:n])], nodes, z, np.zeros(len(nodes)), cls, a.pop("tf", TF), np.zeros(len(nodes), dtype=np.int32),
                                       seeds=np.arange(len(nodes)), **a)

    big = G.Constant(0.1)
    for i in range(32):
        big = big + G.Constant(0.1 + 0.01 * i)
    assert big.size() == 65
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*64 nodes"):
        run([good, big])
    # the ChangePoint fit boundary, counted from the HMC kernel's own map: the longest chain that fits moves, one more is refused
    k_fit = max(k for k in range(1, 40) if H.cp_chain_fits_hmc(k, N))
    assert k_fit == 4
    r = run([TS.cp_chain(G, k_fit)], n=N)
    assert r.info[0] == 0 and np.isfinite(r.logpdf[0]) and r.counts[0][1] == 1
    with pytest.raises(G.AGPError, match=r"\(-3\).*particle 1.*LDS"):
        run([good, TS.cp_chain(G, k_fit + 1)], n=N)
    assert run([TS.cp_chain(G, k_fit + 1)], n=100).info[0] == 0
    with pytest.raises(G.AGPError, match=r"\(-1\).*particle 1.*class 3"):
        run([good, good], cls=[np.array([0, 0], dtype=np.int32), np.array([0, 3], dtype=np.int32)])
    bad_tf = TF.copy(); bad_tf[1, 1] = 0.0
    with pytest.raises(G.AGPError, match=r"\(-1\).*class 1.*sigma"):
        run([good], tf=bad_tf)
    for kw in (dict(n_hmc=-1), dict(L_param=-1), dict(L_noise=-1), dict(eps_param=-0.1), dict(eps_noise=-0.1)):
        with pytest.raises(G.AGPError, match=r"\(-1\).*negative"):
            run([good], **kw)
    # n_hmc == 0: the transformed inputs and their log-density
    r = run([good], n_hmc=0)
    lp, _ = engine.logpdf_series_batch([(ts[:20], xs[:20])], [G.with_params(good, r.prm[0])], r.noise, [0])
    assert np.array_equal(bits(lp), bits(r.logpdf)) and (r.counts == 0).all() and np.array_equal(bits(r.z[0]), bits(np.array([0.1, 0.1])))
    # null outputs; P == 0
    dp = C.POINTER(C.c_double)
    rc = engine._lib.agp_hmc_series_batch(engine._ctx, 0, np.zeros(1, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64)), None, None, 1,
                                          None, None, None, None, None, None, None, 3, TF.ctypes.data_as(dp), 0, 1e-5, 1, 1, 0.02, 1, 0.02, 1,
                                          None, 0, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"null pointer" in engine._lib.agp_last_error(engine._ctx)
    rc = engine._lib.agp_hmc_series_batch(engine._ctx, 0, None, None, None, 0, None, None, None, None, None, None, None, 3, None, 0, 1e-5, 1, 1,
                                          0.02, 1, 0.02, 1, None, 0, None, None, None, None, None, None, None, None)
    assert rc == 0


def test_stateless(pkg, short_run):
    cs = list(short_cases())
    eng = pkg.GPEngine(0)
    try:
        assert np.array_equal(rbits(call(eng, pkg, cs)), rbits(short_run))      # a fresh engine on which set_data was never called
        ts, xs = pkg.prior.synthetic_series(300, seed=9)
        eng.set_data(ts, xs)
        rn, rz = pkg.prior.sample_particles(np.random.default_rng(3), 5, max_depth=3)
        eng.logpdf_batch_extend(rn, rz, n=200, check=False)
        res0, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)

        def snapshot():
            return (eng.extend_stats(), eng.lag_stats(), eng.dedup_stats(), eng.mixture_stats(), eng.coalesce_stats(), eng.n_max,
                    eng.grad_reuse_stats(), eng.grad_lag_domain_particles(), eng.grad_toeplitz_particles(),
                    eng.grad_structured_particles())
        before = snapshot()
        assert np.array_equal(rbits(call(eng, pkg, cs)), rbits(short_run))
        assert snapshot() == before
        res1, _ = eng.logpdf_batch(rn + rn[:2], np.concatenate([rz, rz[:2]]), check=False)
        assert np.array_equal(bits(res1), bits(res0))
        eng.logpdf_batch_extend(rn, rz, n=300, check=False)
        assert eng.extend_stats()["extended"] > before[0]["extended"]
    finally:
        eng.close()


def test_agrees_with_host_route(pkg, engine, short_run):
    """the same chain driven from the host: the reference's loop with logpdf_grad_series_batch as its evaluation"""
    G = pkg
    cs = short_cases()
    for i, c in enumerate(cs):
        if c["n"] not in (17, 33, 176):
            continue
        series = [(np.array(c["ts"]), np.array(c["xs"]))]

        def ev(tree, noise):
            lp, g, gn, info = engine.logpdf_grad_series_batch(series, [G.from_tuple(tree)], [noise], [0], check=False)
            return float(lp[0]), [float(v) for v in g[0]], float(gn[0]), int(info[0])
        k = c["sched"]
        h = H.hmc_chain(tuple_tree(c["tree"]), c["z"], c["z_noise"], c["cls"], TF, c["seed"], k["n_hmc"], ev, L_param=k["L_param"],
                        eps_param=k["eps_param"], L_noise=k["L_noise"], eps_noise=k["eps_noise"])
        assert decisions(h["trace"]) == decisions(short_run.trace[i]) and h["counts"] == short_run.counts[i].tolist()
        dev = max(np.abs(np.array(h["z"]) - short_run.z[i]).max(), abs(h["z_noise"] - short_run.z_noise[i]), abs(h["logpdf"] - short_run.logpdf[i]),
                  np.nanmax(np.abs(np.array(h["trace"])[:, :, 0] - short_run.trace[i][:, :, 0])))
        print(f"[series-hmc] host route {c['name']}: deviation {dev:.3e} (tolerance {c['tol']:.3e})")
        assert dev <= c["tol"], (c["name"], dev)


def test_mcmc_parameters_series(pkg, engine):
    """the public wrapper: trees and noises in, moved trees and noises out, ready for the read-outs of the family"""
    G = pkg
    ts, xs = G.prior.synthetic_series(60, seed=11)
    nodes = [G.SquaredExponential(0.3, 0.8) + G.Periodic(0.7, 0.3, 0.9), G.ChangePoint(G.Linear(0.2, 0.3, 0.4), G.GammaExponential(0.4, 1.2, 0.7), 0.5, 0.001)]
    noises = np.array([0.1, 0.2])
    new, nz, counts, r = G.mcmc_parameters_series(engine, [(ts, xs)], nodes, noises, [0, 0], 3, [1, 2], hmc_config=dict(L_param=3, L_noise=3))
    assert counts.shape == (2, 4) and (counts[:, 1] == 3).all() and new[1].scale == 0.001
    lp, info = engine.logpdf_series_batch([(ts, xs)], new, nz, [0, 0])
    assert (info == 0).all() and np.array_equal(bits(lp), bits(r.logpdf))
    same, nz0, c0, r0 = G.mcmc_parameters_series(engine, [(ts, xs)], nodes, noises, [0, 0], 0, [1, 2])
    for a, b in zip(same, nodes):
        assert np.allclose(G.encode(a)[1], G.encode(b)[1], rtol=1e-13)
    assert np.allclose(nz0, noises, rtol=1e-12)
    means, vars_, pinfo = engine.predict_series_batch([(ts, xs)], [np.linspace(1.0, 1.2, 5)], new, nz, [0, 0])
    assert (pinfo == 0).all() and all(np.isfinite(m).all() for m in means) and all((v > 0).all() for v in vars_)
