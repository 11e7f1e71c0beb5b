"""GPU parity tests (run with `-m gpu` on an MI355X).  Every call goes through the C ABI
(include/autogp_hip.h) via ctypes; the oracle is only the checker.

Tolerances (fp64, stated by BASELINE.json / SURVEY.md §8c):
    logpdf            |gpu - ref| <= 1e-8 * max(1, |ref|)
    predictive        |gpu - ref|_inf <= 1e-8 * max(1, |ref|_inf)
    covariance entry  |gpu - ref| <= 1e-13 * max(1, |K|_inf)   (few ulp of exp/sin/pow argument error)
"""
import ctypes
import threading

import numpy as np
import pytest
import scipy.linalg as sla

from conftest import to_tuple
from oracle import gradcheck as GC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LP_TOL = 1e-8
K_TOL = 1e-13


def lp_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def base_kernels(G):
    return [G.WhiteNoise(1), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
            G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1)]      # test/test_GP.jl:24-33


# ---------------------------------------------------------------------------------------------
def test_native_library_loaded(pkg, engine):
    """The HIP extension is what runs: the .so is mapped in this process and reports gfx950."""
    assert "gfx950" in engine.version
    maps = open("/proc/self/maps").read()
    assert "libautogp_hip.so" in maps


def test_mfma_f64_layout(engine):
    """A=asymmetric probe of v_mfma_f64_16x16x4: C/D row = 4*reg + lane/16, col = lane%16."""
    rng = np.random.default_rng(0)
    A = rng.standard_normal((16, 4)); B = rng.standard_normal((4, 16))
    assert np.allclose(engine.debug_mfma_probe(A, B), A @ B, rtol=0, atol=1e-14)


def test_cov_matrix_fixture_kernels(pkg, engine):
    """eval_cov / compute_cov_matrix_vectorized for the six fixture kernels and all 6x6x3 composites
    on range(-10,10,100) scaled and raw (test/test_GP.jl:35-68 uses both spaces)."""
    G = pkg
    raw = np.linspace(-10, 10, 100)
    scaled = (raw - raw.min()) / (raw.max() - raw.min())
    base = base_kernels(G)
    kernels = list(base)
    for x in base:
        for y in base:
            kernels += [x + y, x * y, G.ChangePoint(x, y, 0.5, 0.95)]
    worst = 0.0
    for ts in (scaled, raw):
        for k in kernels:
            Kd = engine.cov_matrix(k, 0.37, ts)
            Ko = O.compute_cov_matrix_vectorized(k.to_tuple(), 0.37, ts)
            err = np.abs(Kd - Ko).max() / max(1.0, np.abs(Ko).max())
            worst = max(worst, err)
            assert err <= K_TOL, (k, err)
            assert np.array_equal(Kd, Kd.T)
    # scalar twin (src/GP.jl:674-684) on a subset
    for k in kernels[::7]:
        Kd = engine.cov_matrix(k, 0.1, scaled[:40])
        assert np.allclose(Kd, O.compute_cov_matrix(k.to_tuple(), 0.1, scaled[:40]), rtol=1e-13, atol=1e-14)


def test_cov_matrix_edge_cases(pkg, engine):
    G = pkg
    # duplicate time points with WhiteNoise (src/GP.jl:137-140), ts outside [0,1] (add_data!), n = 1, 2, 129
    ts = np.array([0.3, 0.3, -0.5, 1.7, 0.3, 0.9])
    k = G.WhiteNoise(0.8) + G.SquaredExponential(0.2, 1.5)
    assert np.allclose(engine.cov_matrix(k, 0.05, ts), O.compute_cov_matrix_vectorized(k.to_tuple(), 0.05, ts), atol=1e-15)
    for n in (1, 2, 127, 128, 129, 257):
        t = np.linspace(0, 1, n) if n > 1 else np.array([0.4])
        k = G.ChangePoint(G.GammaExponential(0.1, 2.0, 1.0), G.Periodic(0.3, 0.1, 2.0), 0.5, 0.001)   # tanh saturates
        Kd = engine.cov_matrix(k, 1e-5, t)
        assert np.abs(Kd - O.compute_cov_matrix_vectorized(k.to_tuple(), 1e-5, t)).max() <= K_TOL * max(1, np.abs(Kd).max())
    # Int-typed parameters (test/test_GP.jl:109)
    assert np.allclose(engine.cov_matrix(G.Linear(1), 0, np.array([0., 1., 2.])),
                       O.compute_cov_matrix_vectorized(("LIN", 1, 1, 1), 0, np.array([0., 1., 2.])))


def test_deep_trees_and_stack_reordering(pkg, engine):
    """Right-deep chains (worst case for a naive postfix stack) and a full depth-6 tree."""
    G = pkg
    ts = np.linspace(0, 1, 150)
    leafs = base_kernels(G)[1:]
    chain = leafs[0]
    for i in range(1, 40):                      # right-deep: Strahler number 2, naive stack depth 40
        chain = (leafs[i % 5] + chain) if i % 2 else (leafs[i % 5] * chain)
    Kd = engine.cov_matrix(chain, 0.1, ts)
    Ko = O.compute_cov_matrix_vectorized(chain.to_tuple(), 0.1, ts)
    assert np.abs(Kd - Ko).max() <= 1e-12 * np.abs(Ko).max()

    def full(d, i=0):
        if d == 1:
            return leafs[i % 5]
        l, r = full(d - 1, 2 * i + 1), full(d - 1, 2 * i + 2)
        return G.ChangePoint(l, r, 0.3 + 0.05 * d, 0.01 * d) if d >= 5 else (l + r if (d + i) % 2 else l * r)
    k = full(6)                                  # 63 nodes, 32 leaves, needs the depth-8 stack kernel
    assert k.size() == 63
    Kd = engine.cov_matrix(k, 0.1, ts)
    Ko = O.compute_cov_matrix_vectorized(k.to_tuple(), 0.1, ts)
    assert np.abs(Kd - Ko).max() <= 1e-12 * max(1.0, np.abs(Ko).max())


def test_golden_vectors_logpdf_and_predictive(pkg, engine, golden):
    """All committed golden vectors through agp_logpdf_batch / agp_predict_batch."""
    G = pkg
    from collections import defaultdict
    groups = defaultdict(list)
    for c in golden["cases"]:
        groups[(tuple(c["ts"]), tuple(c["xs"]))].append(c)
    n_checked = 0
    for (ts, xs), cases in groups.items():
        ts = np.array(ts); xs = np.array(xs)
        engine.set_data(ts, xs)
        nodes = [G.from_tuple(to_tuple(c["tree"])) for c in cases]
        noises = np.array([c["noise"] for c in cases])
        lp, info = engine.logpdf_batch(nodes, noises)
        ref = np.array([c["logpdf"] for c in cases])
        assert (info == 0).all()
        err = lp_err(lp, ref)
        assert err.max() <= LP_TOL, (cases[int(err.argmax())]["name"], err.max())
        for c, v in zip(cases, lp):
            if "logpdf_mp" in c:
                assert abs(v - float(c["logpdf_mp"])) <= LP_TOL * max(1.0, abs(v)), c["name"]
        # predictive, grouped by identical query set
        pg = defaultdict(list)
        for c, nd in zip(cases, nodes):
            if "ts_pred" in c:
                pg[tuple(c["ts_pred"])].append((c, nd))
        for tp, items in pg.items():
            tp = np.array(tp)
            mean, var, _, info = engine.predict_batch([nd for _, nd in items], [c["noise"] for c, _ in items], tp)
            for i, (c, _) in enumerate(items):
                mu_ref = np.array(c["pred_mean"]); var_ref = np.array(c["pred_var"])
                assert np.abs(mean[i] - mu_ref).max() <= LP_TOL * max(1.0, np.abs(mu_ref).max()), c["name"]
                assert np.abs(var[i] - var_ref).max() <= LP_TOL * max(1.0, np.abs(var_ref).max()), c["name"]
                q = mean[i][:, None] + np.sqrt(var[i])[:, None] * O.ndtri(np.array([0.025, 0.5, 0.975]))[None, :]
                assert np.abs(q - np.array(c["pred_q"])).max() <= LP_TOL * max(1.0, np.abs(q).max()), c["name"]
        n_checked += len(cases)
    assert n_checked == golden["n_cases"]


_REF_GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden" / "golden_ref_v1.json"


@pytest.mark.skipif(not _REF_GOLDEN.exists(), reason="tests/golden/golden_ref_v1.json absent: generate it with the real AutoGP.jl "
                                                      "(julia tools/make_golden_reference.jl)")
def test_reference_golden_vectors_on_gpu(pkg, engine):
    """The HIP path against outputs of the REAL AutoGP.jl (file written by tools/make_golden_reference.jl under Julia;
    same cases as golden_v1.json).  logpdf within 1e-8 relative, predictive mean / variance / quantiles within 1e-8."""
    import json
    from collections import defaultdict
    ref = json.loads(_REF_GOLDEN.read_text())
    groups = defaultdict(list)
    for c in ref["cases"]:
        groups[(tuple(c["ts"]), tuple(c["xs"]))].append(c)
    for (ts, xs), cases in groups.items():
        ts = np.array(ts); xs = np.array(xs)
        engine.set_data(ts, xs)
        nodes = [pkg.from_tuple(to_tuple(c["tree"])) for c in cases]
        noises = np.array([c["noise"] for c in cases])
        lp, info = engine.logpdf_batch(nodes, noises)
        want = np.array([c["logpdf"] for c in cases])
        assert (info == 0).all() and lp_err(lp, want).max() <= LP_TOL
        for c, nd in zip(cases, nodes):
            if "ts_pred" not in c:
                continue
            mean, var, _, _ = engine.predict_batch([nd], [c["noise"]], np.array(c["ts_pred"]))
            pm = np.array(c["pred_mean"]); pv = np.array(c["pred_var"])
            assert np.abs(mean[0] - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max()), c["name"]
            assert np.abs(var[0] - pv).max() <= 1e-8 * max(1.0, np.abs(pv).max()), c["name"]


@pytest.mark.parametrize("n,P,max_depth", [(1, 4, 2), (2, 4, 2), (17, 6, 3), (127, 8, 3), (128, 8, 3), (129, 8, 3),
                                            (256, 8, 3), (700, 12, 4), (1024, 16, 3)])
def test_logpdf_batch_vs_oracle(pkg, engine, n, P, max_depth):
    """Seeded prior particles; sizes cover n=1,2, tile boundaries, config 1 (256) and config 2 (1024)."""
    ts, xs = pkg.prior.synthetic_series(max(n, 2), seed=n, shuffle=(n % 2 == 0))
    ts, xs = ts[:n], xs[:n]
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n), P, max_depth=max_depth)
    engine.set_data(ts, xs)
    lp, info = engine.logpdf_batch(nodes, noises)
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), ts, xs) for nd, nz in zip(nodes, noises)])
    assert (info == 0).all()
    assert lp_err(lp, ref).max() <= LP_TOL
    # single-particle entry (what Gen calls): bit for bit the batch entry's value when it runs the plain sweep, to rounding
    # when it goes through the factor store (the default: its sweep evaluates every tile inside the factorisation kernels)
    one = engine.logpdf(nodes[0], float(noises[0]))
    assert abs(one - lp[0]) <= 1e-12 * max(1.0, abs(lp[0]))
    engine.set_factor_cache(False)
    try:
        assert engine.logpdf(nodes[0], float(noises[0])) == lp[0]
    finally:
        engine.set_factor_cache(True)


@pytest.mark.parametrize("n,P", [(300, 300), (521, 263), (1000, 257)])
def test_large_population_path_vs_oracle(pkg, engine, n, P):
    """Populations of >= 256 particles take the path the benchmark measures: cost-sorted particles, covariance
    tiles evaluated inside the factorisation kernel (expensive trees prebuilt), diagonal tiles in their own
    lower-triangle-only launch, sub-diagonal tiles with the in-register solve.  Every particle is checked
    against the oracle; P is not a multiple of 8 and n not a multiple of the tile."""
    ts, xs = pkg.prior.synthetic_series(n, seed=n + 1, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n), P, max_depth=4, max_size=31)
    engine.set_data(ts, xs)
    lp, info = engine.logpdf_batch(nodes, noises, check=False)
    ok = info == 0
    assert ok.sum() >= P - 3
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), ts, xs) if g else np.nan for nd, nz, g in zip(nodes, noises, ok)])
    assert lp_err(lp[ok], ref[ok]).max() <= LP_TOL
    # the same particles in small batches (mixed kernel, prebuilt tiles) agree to rounding
    sub = np.flatnonzero(ok)[:16]
    lp_small, _ = engine.logpdf_batch([nodes[i] for i in sub], noises[sub], check=False)
    assert lp_err(lp_small, lp[sub]).max() <= 1e-11


def test_gamma_exponential_table_path(pkg, engine, monkeypatch):
    """agp_set_data tabulates log|t_i - t_j| once; GammaExp leaves of the logpdf sweeps then evaluate
    (|dt|/l)^gamma = exp(gamma (log|dt| - log l)) from it.  Same values as the direct power (engine created with
    AGP_GE_TABLE=0) and as the oracle, including duplicate time points (dt = 0), prefixes of the data and both
    the small-batch (k_cov_tiles) and the >= 256-particle (in-kernel evaluation) paths."""
    G = pkg
    rng = np.random.default_rng(77)
    n = 300
    ts = np.sort(rng.random(n)); ts[100] = ts[99]; ts[200] = ts[199]; xs = 0.5 * rng.standard_normal(n)
    def ge(): return G.GammaExponential(np.exp(-1.5 + rng.standard_normal()), 2 / (1 + np.exp(-rng.standard_normal())), np.exp(-1 + rng.standard_normal()))
    small = [ge(), ge() + G.Linear(0.1, 0.3, 0.7), ge() * ge(), G.ChangePoint(ge(), G.Periodic(0.9, 0.2, 1.1), 0.4, 0.1),
             G.GammaExponential(0.3, 2.0, 1.0), G.GammaExponential(0.3, 0.05, 1.0)]
    big = small + [ge() + G.Linear(*np.exp(-1 + rng.standard_normal(3))) for _ in range(260)]
    monkeypatch.setenv("AGP_GE_TABLE", "0")
    direct = G.GPEngine(0)
    monkeypatch.delenv("AGP_GE_TABLE")
    try:
        for eng_ in (engine, direct):
            eng_.set_data(ts, xs)
        for pop in (small, big):
            nz = np.full(len(pop), 0.15)
            for m in (n, 170):
                a, ia = engine.logpdf_batch(pop, nz, n=m, check=False)
                b, ib = direct.logpdf_batch(pop, nz, n=m, check=False)
                assert np.array_equal(ia, ib) and (ia == 0).all()
                assert lp_err(a, b).max() <= 1e-11
                for i in (0, 2, 3, 5, len(pop) - 1):
                    ref = O.gp_logpdf(pop[i].to_tuple(), 0.15, ts[:m], xs[:m])
                    assert abs(a[i] - ref) <= LP_TOL * max(1.0, abs(ref))
    finally:
        direct.close()


_REFS = {}       # oracle gradients (with their per-component scales) shared by the parametrisations of one test


@pytest.mark.parametrize("env", [{"AGP_SPLIT_DIAG": "0"}, {"AGP_SPLIT_DIAG": "1"}, {"AGP_FUSE": "0"}, {"AGP_FUSE": "1"},
                                 {"AGP_DEDUP": "0", "AGP_GE_TABLE": "0"}, {"AGP_RIGHT_LOOKING": "0"}, {"AGP_RIGHT_LOOKING": "1"},
                                 {"AGP_SPLIT_DIAG": "0", "AGP_RIGHT_LOOKING": "0"}, {"AGP_FLOW": "0"}, {"AGP_FLOW": "1"},
                                 {"AGP_FLOW": "1", "AGP_FUSE": "0"}, {"AGP_FLOW": "0", "AGP_RIGHT_LOOKING": "0"},
                                 {"AGP_GRAD_FFT": "0"}, {"AGP_GRAD_FFT": "1"}, {"AGP_GRAD_LAGDOM": "0"}, {"AGP_GRAD_LAGDOM": "1"}, {"AGP_LAG_RANK": "0"},
                                 {"AGP_LAG": "0"}, {"AGP_LAG": "3"}, {"AGP_LATTICE": "0"}, {"AGP_REFERENCE_ARITHMETIC": "1"}])
def test_runtime_switches_agree_with_default(pkg, engine, monkeypatch, env):
    """Every documented schedule / path switch selects different kernels for the same arithmetic: value,
    info and gradient agree with the default engine to rounding, on a 260-particle population (in-kernel evaluation, split
    launches) and on a 12-particle one (mixed launch).  (The regular-grid switches change how t_i - t_j is formed: 1e-10.)"""
    tol = 1e-10 if any(k.startswith("AGP_LAG") or k == "AGP_REFERENCE_ARITHMETIC" for k in env) else 1e-11
    ts, xs = pkg.prior.synthetic_series(300, seed=9, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(9), 260, max_depth=4, max_size=15)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other = pkg.GPEngine(0)
    for k in env:
        monkeypatch.delenv(k)
    try:
        engine.set_data(ts, xs); other.set_data(ts, xs)
        for sl in (slice(0, 260), slice(0, 12)):
            a, ia = engine.logpdf_batch(nodes[sl], noises[sl], check=False)
            b, ib = other.logpdf_batch(nodes[sl], noises[sl], check=False)
            ok = ia == 0
            assert np.array_equal(ia > 0, ib > 0) and ok.sum() >= 10
            assert lp_err(a[ok], b[ok]).max() <= tol
        ga = engine.logpdf_grad_batch(nodes[:40], noises[:40], check=False)
        gb = other.logpdf_grad_batch(nodes[:40], noises[:40], check=False)
        if "switches" not in _REFS:
            _REFS["switches"] = GC.references(nodes[:40], noises[:40], ts, xs)
        for i in range(40):
            if ga[3][i] == 0:
                sc = max(1.0, np.abs(ga[1][i]).max(), abs(ga[2][i]))
                assert np.abs(ga[1][i] - gb[1][i]).max() <= 1e-9 * sc and abs(ga[2][i] - gb[2][i]) <= 1e-9 * sc
                GC.assert_grad_components(ga[1][i], ga[2][i], _REFS["switches"][i], against=(gb[1][i], gb[2][i]), particle_wide=False, ctx=(env, i))
    finally:
        other.close()


@pytest.mark.parametrize("n,P", [(1500, 9), (1300, 70), (900, 300), (2048, 48)])
def test_dataflow_schedule_vs_oracle(pkg, n, P, monkeypatch):
    """The single-launch dataflow schedule (k_chol_flow: persistent workgroups, tiles handed out by ticket, per-tile
    ready flags) — the default for medium populations — forced on (AGP_FLOW=1) and off (AGP_FLOW=0): both against the
    oracle on every particle, against each other to rounding, bitwise reproducible run to run, with tiles evaluated
    in-kernel and prebuilt (AGP_FUSE=0), on the regular-grid path and on the general one (AGP_LAG=0)."""
    from oracle import fast as F
    ts, xs = pkg.prior.synthetic_series(n, seed=n + P, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n + P), P, max_depth=4, max_size=31)
    progs = pkg.encode_batch(nodes)
    ref, rinfo = F.gp_logpdf_many(progs, noises, ts, xs)
    res = {}
    for name, env in (("cols", {"AGP_FLOW": "0"}), ("flow", {"AGP_FLOW": "1"}),
                      ("flow_prebuilt", {"AGP_FLOW": "1", "AGP_FUSE": "0"}),
                      ("flow_general", {"AGP_FLOW": "1", "AGP_LAG": "0"}),
                      ("flow_prebuilt_general", {"AGP_FLOW": "1", "AGP_FUSE": "0", "AGP_LAG": "0"}),
                      ("auto", {})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = pkg.GPEngine(0)
        for k in env:
            monkeypatch.delenv(k)
        try:
            eng.set_data(ts, xs)
            lp, info = eng.logpdf_batch(None, noises, check=False, programs=progs)
            lp2, info2 = eng.logpdf_batch(None, noises, check=False, programs=progs)
            assert np.array_equal(lp, lp2, equal_nan=True) and np.array_equal(info, info2), name
            ok = (info == 0) & (rinfo == 0)
            assert ok.sum() >= P - 2 and np.array_equal(info > 0, rinfo > 0)
            assert lp_err(lp[ok], ref[ok]).max() <= LP_TOL, name
            res[name] = lp
        finally:
            eng.close()
    for name in res:
        ok = np.isfinite(res[name]) & np.isfinite(res["cols"])
        assert lp_err(res[name][ok], res["cols"][ok]).max() <= 1e-10, name


def test_config1_se_plus_linear(pkg, engine):
    """BASELINE config 1: n=256, 8 particles, fixed SE+Linear kernel."""
    G = pkg
    ts, xs = pkg.prior.synthetic_series(256, seed=161)
    rng = np.random.default_rng(161)
    nodes = [G.SquaredExponential(*np.exp(-1.5 + rng.standard_normal(2))) + G.Linear(*np.exp(-1.5 + rng.standard_normal(3)))
             for _ in range(8)]
    noises = np.exp(-1.5 + rng.standard_normal(8)) + 1e-5
    engine.set_data(ts, xs)
    lp, info = engine.logpdf_batch(nodes, noises)
    ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), ts, xs) for nd, nz in zip(nodes, noises)])
    assert (info == 0).all() and lp_err(lp, ref).max() <= LP_TOL
    tp = np.concatenate([ts, np.linspace(1.0, 1.2, 44)])
    mean, var, _, _ = engine.predict_batch(nodes, noises, tp)
    for i in range(8):
        mu, cov = O.predict_mvn(nodes[i].to_tuple(), float(noises[i]), ts, xs, tp)
        assert np.abs(mean[i] - mu).max() <= LP_TOL * max(1.0, np.abs(mu).max())
        assert np.abs(var[i] - np.diag(cov)).max() <= LP_TOL * max(1.0, np.abs(cov).max())


def test_annealing_prefixes_and_n0(pkg, engine):
    """Data-annealing evaluates on ts[1:step] of the resident data (src/inference_smc_anneal_data.jl:206-217);
    n = 0 returns 0 (ibid. :185-187)."""
    ts, xs = pkg.prior.synthetic_series(600, seed=9, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(9), 6, max_depth=3)
    engine.set_data(ts, xs)
    for n in [0] + pkg.schedule.linear_schedule(600, 0.2):
        lp, info = engine.logpdf_batch(nodes, noises, n=n)
        ref = np.array([O.gp_logpdf(nd.to_tuple(), float(nz), ts[:n], xs[:n]) for nd, nz in zip(nodes, noises)])
        assert lp_err(lp, ref).max() <= LP_TOL, n
    with pytest.raises(pkg.AGPError):
        engine.logpdf_batch(nodes, noises, n=601)


def test_predictive_shapes_and_mean_function(pkg, engine):
    """m > n with queries duplicating the training times (the usual API call, src/api.jl:497-522),
    m < n, n = 0, noise_pred = 0 and a non-zero mean function (test/test_api.jl:62-69)."""
    G = pkg
    k = G.Linear(0.3, 0.2, 0.5) + G.Periodic(0.4, 0.25, 0.6) * G.SquaredExponential(0.5, 1.0)
    for n, tp in ((50, np.linspace(0, 1.2, 30)), (128, None), (200, None), (0, np.linspace(0, 1, 40)), (300, np.array([0.5]))):
        ts, xs = pkg.prior.synthetic_series(max(n, 2), seed=5 + n)
        ts, xs = ts[:n], xs[:n]
        if tp is None:
            tp = np.concatenate([ts, np.linspace(1.0, 1.3, n // 2 + 7)])
        engine.set_data(ts, xs)
        for npred, meanf in ((None, None), (0.0, None), (None, lambda t: 0.3 + 0.1 * t)):
            mt = None if meanf is None else np.array([meanf(t) for t in ts])
            mp_ = None if meanf is None else np.array([meanf(t) for t in tp])
            mean, var, cov, info = engine.predict_batch([k], [0.08], tp, noise_pred=npred, mean_train=mt, mean_pred=mp_,
                                                        want_cov=True)
            mu, cv = O.predict_mvn(k.to_tuple(), 0.08, ts, xs, tp, noise_pred=npred, mean=meanf)
            sc = max(1.0, np.abs(cv).max())
            assert np.abs(mean[0] - mu).max() <= LP_TOL * max(1.0, np.abs(mu).max())
            assert np.abs(cov[0] - cv).max() <= LP_TOL * sc
            assert np.array_equal(cov[0], cov[0].T) and np.array_equal(np.diag(cov[0]), var[0])
    # module-level mirror of Distributions.MvNormal(node, ...) + quantile (src/GP.jl:731-758, 1006-1012)
    ts, xs = pkg.prior.synthetic_series(80, seed=1)
    d = G.MvNormal(k, 0.08, ts, xs, np.linspace(0, 1.1, 9), engine=engine)
    mu, cv = O.predict_mvn(k.to_tuple(), 0.08, ts, xs, np.linspace(0, 1.1, 9))
    assert np.allclose(G.quantile(d, [0.1, 0.5, 0.9]), O.quantile(mu, cv, [0.1, 0.5, 0.9]), atol=1e-8)


def test_predictive_likelihood_identity_on_gpu(pkg, engine):
    """logpdf(joint) - logpdf(obs) = logpdf(predictive, xs_test) with every term from the GPU
    (test/experiment_hmc.jl:111-132)."""
    G = pkg
    rng = np.random.default_rng(3)
    ts, xs = pkg.prior.synthetic_series(500, seed=77, shuffle=True)
    n_obs = 380
    for k in [G.SquaredExponential(0.2, 1.0), G.Linear(0.5) + G.Periodic(0.3, 0.25, 1.0),
              G.ChangePoint(G.Linear(0.5), G.Linear(1.5), 0.5, 0.001)]:
        engine.set_data(ts, xs)
        lj = engine.logpdf(k, 0.1)
        lo = engine.logpdf(k, 0.1, n=n_obs)
        mean, var, cov, _ = engine.predict_batch([k], [0.1], ts[n_obs:], n=n_obs, want_cov=True)
        lpred = O.mvnormal_logpdf(xs[n_obs:], cov[0], mean[0])
        assert abs((lj - lo) - lpred) <= 1e-7 * max(1.0, abs(lpred))


GRAD_TOL = 1e-7     # |g_gpu - g_ref| <= GRAD_TOL * max(1, |g_ref|_inf): both sides form K^-1 in fp64
# (and per component, |g_k - ref_k| <= GRAD_TOL * S_k with the 80-bit arbiter deciding misses: oracle/gradcheck.py)


def test_logpdf_gradient(pkg, engine):
    """d logpdf / d theta and d / d noise against the analytic oracle (itself pinned by finite
    differences and mpmath in tests/test_oracle.py): fixture kernels, composites, ChangePoints, a duplicate
    time point, n not a multiple of the tile, and a batch large enough for the fused build."""
    G = pkg
    base = base_kernels(G)
    kernels = list(base) + [base[2] + base[5], base[3] * base[4], G.ChangePoint(base[2], base[5], 0.5, 0.05),
                            G.ChangePoint(base[3] + base[4], base[2] * base[5], 0.3, 0.2),
                            (base[2] + base[3]) * (base[4] + base[5]) + G.ChangePoint(base[1], base[0], 0.6, 0.1)]
    rng = np.random.default_rng(23)
    for n in (40, 200, 300):
        ts = np.sort(rng.random(n)); ts[n // 2] = ts[n // 2 - 1]; xs = 0.4 * rng.standard_normal(n)
        engine.set_data(ts, xs)
        noises = np.full(len(kernels), 0.2)
        lp, grads, gn, info = engine.logpdf_grad_batch(kernels, noises)
        lp2, _ = engine.logpdf_batch(kernels, noises)
        assert (info == 0).all() and np.array_equal(lp, lp2)
        for k, g, gnz in zip(kernels, grads, gn):
            lpo, go, gno = O.gp_logpdf_grad(k.to_tuple(), 0.2, ts, xs)
            sc = max(1.0, np.abs(go).max(), abs(gno))
            assert g.shape == go.shape
            assert np.abs(g - go).max() <= GRAD_TOL * sc, (n, k, g, go)
            assert abs(gnz - gno) <= GRAD_TOL * sc, (n, k)
            GC.assert_grad_components(g, gnz, GC.reference(k.to_tuple(), 0.2, ts, xs), ctx=(n, k))
    # prior-sampled population, P >= 256 (fused build + cost sorting + scatter back to caller order)
    ts, xs = pkg.prior.synthetic_series(256, seed=5, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(5), 260, max_depth=4, max_size=15)
    engine.set_data(ts, xs)
    lp, grads, gn, info = engine.logpdf_grad_batch(nodes, noises, check=False)
    for i in list(range(0, 260, 13)) + [259]:
        if info[i] != 0:
            continue
        lpo, go, gno = O.gp_logpdf_grad(nodes[i].to_tuple(), float(noises[i]), ts, xs)
        assert abs(lp[i] - lpo) <= LP_TOL * max(1.0, abs(lpo))
        GC.assert_grad_components(grads[i], gn[i], GC.reference(nodes[i].to_tuple(), float(noises[i]), ts, xs), ctx=(i, nodes[i]))
    # n = 0: zero gradient
    lp, grads, gn, info = engine.logpdf_grad_batch(kernels[:3], [0.1] * 3, n=0)
    assert (lp == 0).all() and all((g == 0).all() for g in grads) and (gn == 0).all()


def test_logpdf_gradient_large_trees_and_chunks(pkg, engine):
    """Trees above 16 nodes take the 64-node kernel variant (mixed with small ones in one batch); a tight
    workspace limit forces several chunks; trees above 64 nodes are rejected, not mis-evaluated."""
    G = pkg
    leafs = base_kernels(G)[1:]

    def full(d, i=0):
        if d == 1:
            return leafs[i % 5]
        l, r = full(d - 1, 2 * i + 1), full(d - 1, 2 * i + 2)
        return G.ChangePoint(l, r, 0.3 + 0.05 * d, 0.05 * d) if d == 5 else (l + r if (d + i) % 2 else l * r)
    big = full(5)                      # 31 nodes, 16 leaves, one ChangePoint at the root
    mid = full(4, 3)                   # 15 nodes
    chain = leafs[0]
    for i in range(1, 12):             # right-deep chain, 23 nodes
        chain = (leafs[i % 5] + chain) if i % 2 else (leafs[i % 5] * chain)
    kernels = [leafs[1], big, mid, chain, leafs[3] * leafs[4], big + leafs[2]]
    assert big.size() == 31 and (big + leafs[2]).size() == 33
    rng = np.random.default_rng(31)
    n = 200
    ts = np.sort(rng.random(n)); xs = 0.4 * rng.standard_normal(n)
    engine.set_data(ts, xs)
    noises = np.full(len(kernels), 0.3)
    lp, grads, gn, info = engine.logpdf_grad_batch(kernels, noises)
    refs = [O.gp_logpdf_grad(k.to_tuple(), 0.3, ts, xs) for k in kernels]
    for k, g, gnz, (lpo, go, gno) in zip(kernels, grads, gn, refs):
        GC.assert_grad_components(g, gnz, GC.reference(k.to_tuple(), 0.3, ts, xs), ctx=k)
    # chunked workspace: L + Z for two particles at a time (nt = 2 -> 3 tiles)
    engine.set_workspace_limit(2 * 2 * 3 * 128 * 128 * 8)
    try:
        lp2, grads2, gn2, _ = engine.logpdf_grad_batch(kernels, noises)
    finally:
        engine.set_workspace_limit(0)
    assert np.array_equal(lp, lp2) and np.array_equal(gn, gn2) and all(np.array_equal(a, b) for a, b in zip(grads, grads2))
    with pytest.raises(pkg.AGPError, match="64 nodes"):
        engine.logpdf_grad_batch([full(7)], [0.3])             # 127 nodes


def test_infer_gp_sum(pkg, engine):
    """GP.infer_gp_sum (src/GP.jl:904-993) against the oracle restatement, plus the reference's own
    relational checks (test/test_GP.jl:150-240): the observable block equals the single-kernel
    predictive of the summed kernel, and with noise_pred = 0 the latent covariances add up to it."""
    G = pkg
    rng = np.random.default_rng(9)
    k1, k2, k3 = G.SquaredExponential(0.3, 0.8), G.Periodic(0.5, 0.2, 0.4), G.Linear(0.2, 0.1, 0.6) * G.GammaExponential(0.4, 1.3, 0.7)
    for n, p, kernels in ((30, 9, [k1, k2]), (150, 40, [k1, k2, k3]), (200, 130, [k3, G.ChangePoint(k1, k2, 0.5, 0.02)]), (64, 5, [k2])):
        ts = np.sort(rng.random(n)); xs = 0.3 * rng.standard_normal(n); tp = np.linspace(0, 1.2, p)
        engine.set_data(ts, xs)
        for npred in (None, 0.0):
            mean, cov, iF, iX = engine.infer_gp_sum(kernels, 0.1, tp, noise_pred=npred)
            mu_o, S_o, iF_o, iX_o = O.infer_gp_sum([k.to_tuple() for k in kernels], 0.1, ts, xs, tp, noise_pred=npred)
            assert iX == iX_o and iF == iF_o
            assert np.abs(mean - mu_o).max() <= LP_TOL * max(1.0, np.abs(mu_o).max())
            assert np.abs(cov - S_o).max() <= LP_TOL * max(1.0, np.abs(S_o).max())
            assert np.array_equal(cov, cov.T)
        # observable block == predictive MvNormal of the summed kernel (+ the 1e-8 jitter of infer_gp_sum)
        ksum = kernels[0]
        for k in kernels[1:]:
            ksum = ksum + k
        mean, cov, iF, iX = engine.infer_gp_sum(kernels, 0.1, tp)
        pm, pv, pc, _ = engine.predict_batch([ksum], [0.1], tp, want_cov=True)
        assert np.abs(mean[iX] - pm[0]).max() <= 1e-8
        assert np.abs(cov[iX, iX] - (pc[0] + 1e-8 * np.eye(p))).max() <= 1e-8
        # sum of latent covariances = observable covariance when noise_pred = 0 (test/test_GP.jl:228-237)
        mean0, cov0, iF, iX = engine.infer_gp_sum(kernels, 0.1, tp, noise_pred=0.0)
        lat = sum(cov0[a, b] for a in iF for b in iF)
        M = len(kernels)
        assert np.abs(lat - (cov0[iX, iX] + (M * M - 1) * 0 * np.eye(p))).max() <= 1e-6
        assert np.abs(sum(mean0[a] for a in iF) - mean0[iX]).max() <= 1e-8
    # module-level mirror
    mean, cov, idx = G.infer_gp_sum([k1, k2], 0.1, ts, xs, tp, engine=engine)
    assert mean.shape == (3 * 5,) and idx["X"] == slice(10, 15)


def test_debug_cholesky_and_nonpd(pkg, engine):
    rng = np.random.default_rng(2)
    for n in (16, 100, 128, 200, 384, 1000):
        M = rng.standard_normal((n, n)); K = M @ M.T / n + 0.5 * np.eye(n)
        L, info = engine.debug_cholesky(K)
        assert info == 0
        Lr = sla.cholesky(K, lower=True)
        assert np.abs(L - Lr).max() <= 1e-12 * np.abs(Lr).max()
        assert np.array_equal(L, np.tril(L))
    K = np.eye(300); K[150, 150] = -1.0
    _, info = engine.debug_cholesky(K)
    assert info == 151                                      # LAPACK dpotrf convention
    # through the likelihood entry: PosDefException like the reference (no try/catch upstream)
    ts = np.array([0.1, 0.1, 0.5]); xs = np.zeros(3)
    engine.set_data(ts, xs)
    k = pkg.Constant(1.0) * pkg.Linear(0.0, -5.0, 0.0)       # negative "bias" makes K indefinite
    lp, info = engine.logpdf_batch([k, pkg.Constant(1.0)], [1e-5, 0.1], check=False)
    assert info[0] > 0 and np.isnan(lp[0]) and info[1] == 0 and np.isfinite(lp[1])
    with pytest.raises(pkg.PosDefException):
        engine.logpdf_batch([k], [1e-5])


def test_bad_programs_are_rejected(pkg, engine):
    lib, ctx = engine._lib, engine._ctx
    ts, xs = pkg.prior.synthetic_series(10, seed=1)
    engine.set_data(ts, xs)
    out = ctypes.c_double(); info = ctypes.c_int32()

    def call(ops, prm):
        ops = np.asarray(ops, dtype=np.uint8); prm = np.asarray(prm, dtype=np.float64)
        return lib.agp_logpdf(ctx, 10, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ops.size,
                              prm.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), prm.size, 0.1,
                              ctypes.byref(out), ctypes.byref(info))
    assert call([1], [0.5]) == 0
    assert call([6], [0.5]) == -3                    # operator without operands
    assert call([1, 1], [0.5, 0.5]) == -3            # two kernels left on the stack
    assert call([1], [0.5, 0.7]) == -3               # parameter count mismatch
    assert call([42], [0.5]) == -3                   # unknown opcode
    assert b"particle 0" in lib.agp_last_error(ctx)
    # a chain of 75 ChangePoints needs 75 per-point tables: more than 160 KiB of LDS can hold next to the program -> a
    # clear program error, not an opaque launch failure (74 still run)
    def chain(ncp):
        ops, prm = [1], [0.5]
        for _ in range(ncp):
            ops += [1, 8]; prm += [0.5, 0.3, 0.05]
        return ops, prm
    assert call(*chain(74)) == 0 and np.isfinite(out.value), lib.agp_last_error(ctx)
    assert call(*chain(75)) == -3 and b"LDS" in lib.agp_last_error(ctx)


def test_resampled_population_is_evaluated_once(pkg, engine):
    """A resampled SMC population (src/inference_smc_anneal_data.jl:198-204) holds copies: the host-output sweeps
    evaluate each distinct (kernel, noise) once and every copy gets bit-identical value, info and gradient;
    particles that differ only in noise or in one parameter bit are NOT merged."""
    G = pkg
    ts, xs = pkg.prior.synthetic_series(200, seed=11, shuffle=True)
    engine.set_data(ts, xs)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(11), 12, max_depth=3, max_size=15)
    idx = np.random.default_rng(12).integers(0, 12, size=300)          # multinomial resampling
    pop = [nodes[i] for i in idx]; pnz = noises[idx].copy()
    pop += [nodes[0], nodes[0], G.SquaredExponential(0.3, 1.0), G.SquaredExponential(np.nextafter(0.3, 1.0), 1.0)]
    pnz = np.concatenate([pnz, [noises[0], noises[0] * 1.5, 0.2, 0.2]])
    s0 = engine.dedup_stats()
    lp, info = engine.logpdf_batch(pop, pnz, check=False)
    s1 = engine.dedup_stats()
    n_unique = len(set(idx.tolist())) + 3            # + nodes[0] at another noise + the two SE kernels
    assert s1[0] - s0[0] == len(pop) and s1[1] - s0[1] == n_unique
    ref, rinfo = engine.logpdf_batch(nodes, noises, check=False)
    assert np.array_equal(lp[:300], ref[idx]) and np.array_equal(info[:300], rinfo[idx])
    assert lp[300] == ref[0] and lp[301] != ref[0]
    for i in (0, 150, 301, 303):
        if info[i] == 0:
            lpo = O.gp_logpdf(pop[i].to_tuple(), float(pnz[i]), ts, xs)
            assert abs(lp[i] - lpo) <= LP_TOL * max(1.0, abs(lpo))
    lpg, grads, gn, ginfo = engine.logpdf_grad_batch(pop, pnz, check=False)
    rlp, rgrads, rgn, _ = engine.logpdf_grad_batch(nodes, noises, check=False)
    # (the value sweep of this regularly spaced series runs on the sorted copy with lag tables, the gradient sweep in the
    # caller's order: equal to rounding, not bit for bit)
    okg = (ginfo == 0) & (info == 0)
    assert np.array_equal(ginfo == 0, info == 0) and lp_err(lpg[okg], lp[okg]).max() <= 1e-11
    for j, i in enumerate(idx):
        assert np.array_equal(grads[j], rgrads[i]) and gn[j] == rgn[i]


def test_predict_evaluates_duplicates_once(pkg, engine):
    """agp_predict_batch on a resampled population (copies of a few survivors): same mean / variance / covariance / info
    per copy as the particle evaluated on its own, whatever noise_pred the copies carry."""
    ts, xs = pkg.prior.synthetic_series(260, seed=8)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(8), 5, max_depth=3)
    engine.set_data(ts, xs)
    tp = np.linspace(0.0, 1.2, 33)
    parents = np.array([0, 3, 3, 1, 0, 0, 4, 3, 2, 2, 0])
    pop = [nodes[i] for i in parents]; nz = noises[parents]
    npred = np.where(np.arange(len(parents)) % 2 == 0, 0.05, 0.2)          # copies may differ in noise_pred
    mean, var, cov, info = engine.predict_batch(pop, nz, tp, noise_pred=npred, want_cov=True)
    for j, i in enumerate(parents):
        m1, v1, c1, _ = engine.predict_batch([nodes[i]], noises[i:i + 1], tp, noise_pred=npred[j], want_cov=True)
        assert np.array_equal(mean[j], m1[0]) and np.array_equal(var[j], v1[0]) and np.array_equal(cov[j], c1[0])
    assert (info == 0).all()


def test_workspace_chunking_is_invisible(pkg, engine):
    ts, xs = pkg.prior.synthetic_series(300, seed=8)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(8), 13, max_depth=3)
    engine.set_data(ts, xs)
    a, _ = engine.logpdf_batch(nodes, noises)
    engine.set_workspace_limit(3 * 6 * 128 * 128 * 8)      # room for 3 particles per chunk (nt=3 -> 6 tiles)
    try:
        b, _ = engine.logpdf_batch(nodes, noises)
        tp = np.linspace(0, 1.1, 20)
        m1, v1, _, _ = engine.predict_batch(nodes, noises, tp)
    finally:
        engine.set_workspace_limit(0)
    m2, v2, _, _ = engine.predict_batch(nodes, noises, tp)
    assert np.array_equal(a, b) and np.array_equal(m1, m2) and np.array_equal(v1, v2)


def test_concurrent_callers(pkg, engine):
    """P host threads calling the single-particle entry at once — the reference's call pattern
    (Threads.@threads over particles, src/inference_smc_anneal_data.jl:133-135)."""
    ts, xs = pkg.prior.synthetic_series(400, seed=12)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(12), 24, max_depth=3)
    engine.set_data(ts, xs)
    ref, _ = engine.logpdf_batch(nodes, noises)
    for cache in (True, False):          # through the factor store (default): to rounding; plain sweeps: bit for bit
        engine.set_factor_cache(cache)
        try:
            out = np.zeros(24)

            def work(i):
                for _ in range(3):
                    out[i] = engine.logpdf(nodes[i], float(noises[i]))
            th = [threading.Thread(target=work, args=(i,)) for i in range(24)]
            [t.start() for t in th]; [t.join() for t in th]
            assert np.array_equal(out, ref) if not cache else lp_err(out, ref).max() <= 1e-12
        finally:
            engine.set_factor_cache(True)


def test_coalescing_of_single_particle_callers(pkg, engine):
    """Concurrent agp_logpdf callers are merged into batched sweeps inside the library; callers with a
    different n (an annealing step change mid-flight) are served by a later batch; a malformed program
    only fails its own caller."""
    ts, xs = pkg.prior.synthetic_series(300, seed=21)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(21), 32, max_depth=3)
    engine.set_data(ts, xs)
    ref_a, _ = engine.logpdf_batch(nodes, noises, n=300)
    ref_b, _ = engine.logpdf_batch(nodes, noises, n=170)
    engine.set_coalesce_window(20000)
    engine.set_factor_cache(False)         # plain sweeps: the callers get the batch entry's values bit for bit
    c0, b0 = engine.coalesce_stats()
    out = np.zeros(32); errs = []
    barrier = threading.Barrier(33)

    def work(i):
        barrier.wait()
        try:
            out[i] = engine.logpdf(nodes[i], float(noises[i]), n=300 if i % 2 == 0 else 170)
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    def bad():
        barrier.wait()
        ops = np.array([6], dtype=np.uint8); prm = np.zeros(1)
        o = ctypes.c_double(); inf = ctypes.c_int32()
        rc = engine._lib.agp_logpdf(engine._ctx, 300, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 1,
                                    prm.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0, 0.1, ctypes.byref(o), ctypes.byref(inf))
        if rc != -3:
            errs.append(AssertionError(f"bad program returned {rc}"))
    th = [threading.Thread(target=work, args=(i,)) for i in range(32)] + [threading.Thread(target=bad)]
    [t.start() for t in th]; [t.join() for t in th]
    engine.set_coalesce_window(300)
    engine.set_factor_cache(True)
    assert not errs, errs
    exp = np.where(np.arange(32) % 2 == 0, ref_a, ref_b)
    assert np.array_equal(out, exp)
    c1, b1 = engine.coalesce_stats()
    assert c1 - c0 == 33 and b1 - b0 <= 12, (c1 - c0, b1 - b0)     # 33 calls served by a handful of sweeps


def test_coalescing_of_single_particle_gradient_callers(pkg, engine):
    """agp_logpdf_grad from many threads (one trace per thread, as Gen.choice_gradients is driven): the library
    forms batched gradient sweeps; every caller gets exactly what the batch entry returns for its particle, and
    value-only callers running at the same time are batched separately."""
    ts, xs = pkg.prior.synthetic_series(300, seed=21, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(21), 24, max_depth=3, max_size=15)
    engine.set_data(ts, xs)
    ref = engine.logpdf_grad_batch(nodes, noises, check=False)
    for cache in (False, True):
        # plain sweeps: bit for bit.  Through the factor store (default) a gradient caller may find the factor its
        # value-calling twin has just left there: to rounding.
        engine.set_factor_cache(cache)
        try:
            out = [None] * 48
            def work(i):
                j = i % 24
                if i < 24:
                    out[i] = engine.logpdf_grad(nodes[j], float(noises[j]), check=False)
                else:
                    out[i] = engine.logpdf(nodes[j], float(noises[j]), check=False)
            th = [threading.Thread(target=work, args=(i,)) for i in range(48)]
            for t in th: t.start()
            for t in th: t.join()
        finally:
            engine.set_factor_cache(True)
        for i in range(24):
            if ref[3][i] != 0:
                continue
            lp, g, gn = out[i]
            if not cache:
                assert lp == ref[0][i] and gn == ref[2][i] and np.array_equal(g, ref[1][i])
                # (value-only callers of a regular grid take the sorted lag-table sweep: equal to rounding)
                assert abs(out[24 + i] - ref[0][i]) <= 1e-11 * max(1.0, abs(ref[0][i]))
            else:
                assert abs(lp - ref[0][i]) <= 1e-12 * max(1.0, abs(ref[0][i])) and abs(gn - ref[2][i]) <= 1e-9 * max(1.0, abs(ref[2][i]))
                assert np.all(np.abs(g - ref[1][i]) <= 1e-9 * np.maximum(1.0, np.abs(ref[1][i])))
                assert abs(out[24 + i] - ref[0][i]) <= 1e-12 * max(1.0, abs(ref[0][i]))


def test_randomised_soak(pkg, engine):
    """tools/gpu_fuzz.py: random (n, P, depth) configurations straddling every schedule threshold — oracle parity,
    run-to-run bitwise reproducibility, value agreement between the logpdf and gradient sweeps."""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("gpu_fuzz", Path(__file__).resolve().parent.parent / "tools" / "gpu_fuzz.py")
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    msg = mod.run(pkg, engine, cases=40, seed=5)
    assert msg.startswith("fuzz ok"), msg


def test_device_output_entry(pkg, engine):
    """agp_logpdf_batch_device leaves results in caller-provided device memory on the caller's stream."""
    import torch
    ts, xs = pkg.prior.synthetic_series(256, seed=3)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(3), 9, max_depth=3)
    engine.set_data(ts, xs)
    ref, _ = engine.logpdf_batch(nodes, noises)
    d_lp = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda:0")
    d_info = torch.full((9,), -7, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    engine.logpdf_batch_device(pkg.encode_batch(nodes), noises, 256, d_lp.data_ptr(), d_info.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(d_lp.cpu().numpy(), ref) and (d_info.cpu().numpy() == 0).all()


# ---- full-size, size-independent properties (n = 2048: no oracle run needed for most) -------------
def test_full_size_properties(pkg, engine):
    """BASELINE config 3 size (n=2048).  (1) spot parity vs the oracle on 3 particles;
    (2) invariance of the logpdf under a permutation of the observations; (3) joint/marginal/
    predictive identity; (4) batch composition does not change a particle's value."""
    n = 2048
    ts, xs = pkg.prior.synthetic_series(n, seed=2048)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(2048), 24, max_depth=4, max_size=31)
    engine.set_data(ts, xs)
    lp, info = engine.logpdf_batch(nodes, noises, check=False)
    ok = info == 0
    assert ok.sum() >= 20
    for i in np.flatnonzero(ok)[:3]:
        ref = O.gp_logpdf(nodes[i].to_tuple(), float(noises[i]), ts, xs)
        assert abs(lp[i] - ref) <= LP_TOL * max(1.0, abs(ref))
    perm = np.random.default_rng(1).permutation(n)
    engine.set_data(ts[perm], xs[perm])
    lp2, info2 = engine.logpdf_batch(nodes, noises, check=False)
    assert np.array_equal(info2 == 0, ok)
    assert lp_err(lp2[ok], lp[ok]).max() <= LP_TOL
    sub = [int(i) for i in np.flatnonzero(ok)[:5]]
    lp3, _ = engine.logpdf_batch([nodes[i] for i in sub[::-1]], noises[sub[::-1]])
    # (5 particles take the right-looking schedule, 24 the dataflow one: same value to rounding, not bit for bit)
    assert lp_err(lp3[::-1], lp2[sub]).max() <= 1e-11
    sub8 = [int(i) for i in np.flatnonzero(ok)[:12]]
    lp4, _ = engine.logpdf_batch([nodes[i] for i in sub8[::-1]], noises[sub8[::-1]])
    assert np.array_equal(lp4[::-1], lp2[sub8])          # same schedule, other batch composition: the same bits


def test_engine_against_scikit_learn(pkg, engine):
    """The engine against a THIRD PARTY's implementation, no oracle in between: scikit-learn's GaussianProcessRegressor
    (log marginal likelihood, posterior mean / covariance) on kernels both define, n = 700 (six tile rows, partial last tile),
    through agp_logpdf_batch / agp_predict_batch.  Tolerances as for the oracle: 1e-8."""
    pytest.importorskip("sklearn")
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process import kernels as K
    from test_oracle import _sk_kernel
    G = pkg
    ts, xs = pkg.prior.synthetic_series(700, seed=41, shuffle=True)
    engine.set_data(ts, xs)
    ks = [G.SquaredExponential(0.21, 0.9),
          G.Periodic(0.96, 0.21, 1.1),
          G.GammaExponential(0.33, 1.0, 0.8),
          G.SquaredExponential(0.3, 0.5) + G.Periodic(0.7, 0.15, 0.9) * G.SquaredExponential(0.47, 0.8),
          (G.GammaExponential(0.5, 1.0, 1.2) + G.Constant(0.1)) * (G.Periodic(1.3, 0.4, 0.6) + G.SquaredExponential(0.1, 0.3))]
    nz = np.array([0.07, 0.05, 0.1, 0.08, 0.06])
    tp = np.concatenate([ts[::9], np.linspace(1.0, 1.3, 20)])
    lp, info = engine.logpdf_batch(ks, nz)
    mean, var, cov, _ = engine.predict_batch(ks, nz, tp, want_cov=True)
    assert (info == 0).all()
    for i, k in enumerate(ks):
        kern = _sk_kernel(k.to_tuple()) + K.WhiteKernel(noise_level=float(nz[i]), noise_level_bounds="fixed")
        gpr = GaussianProcessRegressor(kernel=kern, alpha=0.0, optimizer=None).fit(ts[:, None], xs)
        ref = gpr.log_marginal_likelihood()
        assert abs(lp[i] - ref) <= LP_TOL * max(1.0, abs(ref)), (i, lp[i], ref)
        mu_sk, cov_sk = gpr.predict(tp[:, None], return_cov=True)
        assert np.abs(mean[i] - mu_sk).max() <= 1e-8 * max(1.0, np.abs(mu_sk).max())
        assert np.abs(cov[i] - cov_sk).max() <= 1e-8 * max(1.0, np.abs(cov_sk).max())
    # gradients: sklearn differentiates w.r.t. log-parameters (d/dlog p = p d/dp), order = hyperparameter order of the kernel
    cases = [(G.SquaredExponential(0.21, 0.9), 0.07,
              lambda: K.ConstantKernel(0.9) * K.RBF(0.21) + K.WhiteKernel(0.07), ("amp", "len", "noise")),
             (G.Periodic(0.96, 0.21, 1.1), 0.05,
              lambda: K.ConstantKernel(1.1) * K.ExpSineSquared(length_scale=0.96, periodicity=0.21) + K.WhiteKernel(0.05),
              ("amp", "len", "per", "noise"))]
    for k, z, mk, names in cases:
        gpr = GaussianProcessRegressor(kernel=mk(), alpha=0.0, optimizer=None).fit(ts[:, None], xs)
        ref, gsk = gpr.log_marginal_likelihood(gpr.kernel_.theta, eval_gradient=True)
        lpg, g, gn = engine.logpdf_grad(k, z)
        prm = pkg.encode(k)[1]
        mine = {"noise": gn * z}
        if len(names) == 3:
            mine.update(len=g[0] * prm[0], amp=g[1] * prm[1])
        else:
            mine.update(len=g[0] * prm[0], per=g[1] * prm[1], amp=g[2] * prm[2])
        assert abs(lpg - ref) <= LP_TOL * max(1.0, abs(ref))
        for nm, want in zip(names, gsk):
            assert abs(mine[nm] - want) <= 1e-7 * max(1.0, abs(want)), (nm, mine[nm], want)


def test_reference_arithmetic_is_call_order_stable(pkg):
    """agp_set_reference_arithmetic: a particle's results depend on (program, parameters, noise, data, n) alone — the same BITS from a
    batch of 1, of 6 and of 300, from the single-particle entry (coalesced), from the extension entry, from the value part of a
    gradient call, before and after other calls left state behind, on a regular grid (where the default engine would pick among
    lag tables, Toeplitz sweeps and lag-domain contractions) — and they meet the oracle at the stated tolerances."""
    n = 600
    ts, xs = pkg.prior.synthetic_series(n, seed=8, shuffle=True)          # a regular grid: every structured path would apply
    G = pkg
    mine = [G.SquaredExponential(0.2, 0.8) + G.Linear(0.3, 0.2, 0.5), G.Periodic(0.7, 0.21, 1.1) * G.SquaredExponential(0.5, 0.9),
            G.GammaExponential(0.3, 1.2, 0.7) + G.WhiteNoise(0.05), G.ChangePoint(G.Periodic(0.5, 0.1, 1.0), G.SquaredExponential(0.2, 0.6), 0.45, 0.01),
            G.Linear(0.1, 0.3, 0.7), G.Linear(0.2, 0.1, 0.6) * G.Periodic(1.0, 0.3, 0.8) + G.Constant(0.3)]
    nz = np.linspace(0.05, 0.2, len(mine))
    others, onz = pkg.prior.sample_particles(np.random.default_rng(4), 294, max_depth=3)
    tq = np.concatenate([ts[:50], np.linspace(1.0, 1.2, 30)])
    eng = pkg.GPEngine(0)
    try:
        eng.set_reference_arithmetic()
        eng.set_data(ts, xs)
        assert eng.lag_stats() == (False, 0) and eng.lattice_stats()["kind"] == 0
        lp6, i6 = eng.logpdf_batch(mine, nz, check=False)
        assert (i6 == 0).all()
        lp1 = np.array([eng.logpdf_batch([k], [z], check=False)[0][0] for k, z in zip(mine, nz)])
        lps = np.array([eng.logpdf(k, float(z)) for k, z in zip(mine, nz)])          # agp_logpdf (coalescing queue)
        big, _ = eng.logpdf_batch(list(others[:150]) + mine + list(others[150:]), np.concatenate([onz[:150], nz, onz[150:]]), check=False)
        ext, _ = eng.logpdf_batch_extend(mine, nz, check=False)
        ext_prefix, _ = eng.logpdf_batch_extend(mine, nz, n=300, check=False)
        ext2, _ = eng.logpdf_batch_extend(mine, nz, check=False)                      # (would be an extension sweep by default)
        glp, grads, gn, gi = eng.logpdf_grad_batch(mine, nz, check=False)
        glp_big, grads_big, gn_big, _ = eng.logpdf_grad_batch(list(others[:280]) + mine, np.concatenate([onz[:280], nz]), check=False)
        for other in (lp1, lps, big[150:156], ext, ext2, glp, glp_big[280:]):
            assert np.array_equal(lp6, other)
        for a_, b_ in zip(grads, grads_big[280:]):
            assert np.array_equal(a_, b_)
        assert np.array_equal(gn, gn_big[280:])
        assert eng.extend_stats()["tile_rows_reused"] == 0 and eng.grad_lag_domain_particles() == 0 and eng.grad_structured_particles() == 0
        m6, v6, _, _ = eng.predict_batch(mine, nz, tq, check=False)
        m1 = np.array([eng.predict_batch([k], [z], tq, check=False)[0][0] for k, z in zip(mine, nz)])
        mb, vb, _, _ = eng.predict_batch(list(others[:60]) + mine, np.concatenate([onz[:60], nz]), tq, check=False)
        assert np.array_equal(m6, m1) and np.array_equal(m6, mb[60:]) and np.array_equal(v6, vb[60:])
        assert eng.predict_structured_particles() == 0 and eng.lag_predict_passes() == 0
        for i, (k, z) in enumerate(zip(mine, nz)):
            lpo, go, gno = O.gp_logpdf_grad(k.to_tuple(), float(z), ts, xs)
            sc = max(1.0, np.abs(go).max(), abs(gno))
            assert abs(lp6[i] - lpo) <= LP_TOL * max(1.0, abs(lpo))
            assert np.abs(grads[i] - go).max() <= GRAD_TOL * sc and abs(gn[i] - gno) <= GRAD_TOL * sc
            GC.assert_grad_components(grads[i], gn[i], GC.reference(k.to_tuple(), float(z), ts, xs), ctx=(i, k))
            mu, cv = O.predict_mvn(k.to_tuple(), float(z), ts, xs, tq)
            assert np.abs(m6[i] - mu).max() <= 1e-8 * max(1.0, np.abs(mu).max())
            assert np.abs(v6[i] - np.diag(cv)).max() <= 1e-8 * max(1.0, np.abs(cv).max())
        assert np.abs(ext_prefix - eng.logpdf_batch(mine, nz, n=300, check=False)[0]).max() == 0.0
        # the switch cannot be undone piecemeal: every setter that would re-enable a state-dependent path is refused ...
        for setter in (eng.set_lag_tables, eng.set_lag_rank_tables, eng.set_lattice, eng.set_grad_lag_domain, eng.set_factor_cache):
            with pytest.raises(pkg.AGPError, match="reference arithmetic"):
                setter(1)
            setter(0)                                        # (switching OFF what is off already is harmless)
        eng.set_data(ts, xs)
        assert np.array_equal(eng.logpdf_batch(mine, nz, check=False)[0], lp6) and eng.lag_stats() == (False, 0)
    finally:
        eng.close()
    # ... and the one-process multi-device entry with resident factors honours it too (plain sweeps, nothing resident)
    multi = pkg.GPEngineMulti([0])
    try:
        multi.engines[0].set_reference_arithmetic()
        multi.set_data(ts, xs)
        a1, _ = multi.logpdf_batch(mine, nz, check=False, extend=True)
        a2, _ = multi.logpdf_batch(mine, nz, n=300, check=False, extend=True)
        a3, _ = multi.logpdf_batch(mine, nz, check=False, extend=True)
        assert np.array_equal(a1, lp6) and np.array_equal(a3, lp6) and np.array_equal(a2, ext_prefix)
        assert multi.engines[0].extend_stats()["tile_rows_reused"] == 0
    finally:
        multi.close()
