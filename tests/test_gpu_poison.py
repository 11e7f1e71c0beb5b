"""NaN-poison checks (AGP_POISON=1, include/autogp_hip.h agp_get_poison_stats).

The fast paths leave memory unwritten on purpose: the padding steps of a ragged last tile, the store's resident rows, flags
cleared only on the paths that raise them, slot workspaces shared by every entry point.  A kernel that READS such memory
sees a stale finite number today — masked or multiplied by an exact zero, so every result is still right — and a NaN for
a valid particle as soon as the stale number is not finite (after a non-positive-definite particle, or in a fresh
allocation).  A poisoned engine fills every value buffer with NaN bits on allocation, when a workspace slot is claimed and,
in a store sweep, in the rows the sweep recomputes; so:

  * the same call sequence on a poisoned and on a clean engine gives BITWISE equal results (no tolerance: any difference is
    a read of memory the call did not write);
  * every result with info == 0 is finite;
  * the poisoned engine did poison something (poison_stats()["bytes"] > 0), and the path counter the case targets moved.

The second half checks the clean engine against the oracle at the ragged shapes those paths are about.
"""
import threading

import numpy as np
import pytest

from oracle import fast as F
from oracle import gradcheck as GC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LP_TOL = 1e-8
GRAD_TOL = 1e-7

# every class of the last tile's rows (1, 2, 16 | 17, 113 | 127, 128 | 129, 143 .. 145, 240, 256 | 257) and the reference's
# tutorial sizes (135 .. 442 points)
SHAPES = [1, 2, 16, 17, 113, 127, 128, 129, 143, 144, 145, 240, 256, 257, 442]


def lp_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def engines(pkg, monkeypatch, env=None):
    """(poisoned, clean) engines built under the same switches."""
    env = dict(env or {})
    out = []
    for poison in ("1", "0"):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("AGP_POISON", poison)
        out.append(pkg.GPEngine(0))
        for k in list(env) + ["AGP_POISON"]:
            monkeypatch.delenv(k, raising=False)
    return out


def close(*engs):
    for e in engs:
        e.close()


def same(a, b, what):
    """Bitwise equality of two results (arrays, lists of arrays, scalars, tuples of them)."""
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, (what, i))
        return
    if a is None:
        assert b is None, what
        return
    x, y = np.asarray(a), np.asarray(b)
    assert x.shape == y.shape and x.dtype == y.dtype, what
    x, y = np.ascontiguousarray(x).reshape(-1), np.ascontiguousarray(y).reshape(-1)
    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, x, y)


def finite_where_ok(vals, info, what):
    ok = np.asarray(info) == 0
    for v in vals:
        v = np.asarray(v)
        assert np.isfinite(v[ok]).all(), (what, v[ok])


def both(pz, cl, f, what):
    """f(engine) on both engines; the results must be bitwise equal, and the call on the poisoned engine must itself have
    poisoned memory (its slot's value buffers when it claimed the slot, fresh allocations, store rows it recomputes) —
    not only an earlier call or agp_set_data."""
    f0 = pz.poison_stats()["fills"]
    a = f(pz)
    assert pz.poison_stats()["fills"] > f0, ("nothing poisoned by", what)
    b = f(cl)
    same(a, b, what)
    return a


def poisoned(pz):
    st = pz.poison_stats()
    assert st["bytes"] > 0 and st["fills"] > 0, st
    return st


def irregular(n, seed):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.random(max(n, 1))); xs = 0.5 * rng.standard_normal(max(n, 1))
    return ts[:n], xs[:n]


# ---- 1. every entry at every ragged shape --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SHAPES)
def test_poison_entries_at_ragged_shapes(pkg, monkeypatch, n):
    """Values (batch of 5 and 12, single-particle, device output), gradients and a dense predictive pass with covariance, on a
    regular grid (lag paths) and on an irregular series, poisoned vs clean: bitwise."""
    import torch
    pz, cl = engines(pkg, monkeypatch)
    try:
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(100 + n), 12, max_depth=3, max_size=15)
        for kind, (ts, xs) in (("grid", pkg.prior.synthetic_series(max(n, 2), seed=n, shuffle=True)), ("irregular", irregular(n, n))):
            ts, xs = ts[:n], xs[:n]
            for e in (pz, cl):
                e.set_data(ts, xs)
            for P in (5, 12):
                lp, info = both(pz, cl, lambda e: e.logpdf_batch(nodes[:P], noises[:P], check=False), (n, kind, "batch", P))
                finite_where_ok([lp], info, (n, kind, P))
                assert (info == 0).sum() >= P - 2
            one = both(pz, cl, lambda e: e.logpdf(nodes[0], float(noises[0]), check=False), (n, kind, "logpdf"))
            assert np.isfinite(one)

            def dev(e):
                d_lp = torch.zeros(5, dtype=torch.float64, device="cuda:0")
                d_info = torch.zeros(5, dtype=torch.int32, device="cuda:0")
                e.logpdf_batch_device(pkg.encode_batch(nodes[:5]), noises[:5], n, d_lp.data_ptr(), d_info.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                return d_lp.cpu().numpy(), d_info.cpu().numpy()
            lpd, infod = both(pz, cl, dev, (n, kind, "device"))
            finite_where_ok([lpd], infod, (n, kind, "device"))
            g = both(pz, cl, lambda e: e.logpdf_grad_batch(nodes[:6], noises[:6], check=False), (n, kind, "grad"))
            finite_where_ok([g[0], g[2]], g[3], (n, kind, "grad"))
            for i in range(6):
                if g[3][i] == 0:
                    assert np.isfinite(g[1][i]).all(), (n, kind, i)
            tq = np.concatenate([np.linspace(-0.1, 1.1, 7), ts[: min(n, 3)]])
            pr = both(pz, cl, lambda e: e.predict_batch(nodes[:4], noises[:4], tq, want_cov=True, check=False), (n, kind, "predict"))
            for i in range(4):
                if pr[3][i] == 0:
                    assert np.isfinite(pr[0][i]).all() and np.isfinite(pr[1][i]).all() and np.isfinite(pr[2][i]).all(), (n, kind, i)
            if kind == "grid" and n >= 2:
                assert pz.lag_stats()[1] > 0          # (the regular grid's whole-series sweeps took the lag path)
        poisoned(pz)
    finally:
        close(pz, cl)


# ---- 2. populations across the schedule thresholds, schedule switches ----------------------------------------------------

SCHEDULES = [{}, {"AGP_FLOW": "0"}, {"AGP_FLOW": "1"}, {"AGP_SPLIT_DIAG": "1"}, {"AGP_RIGHT_LOOKING": "1"}, {"AGP_FUSE": "0"},
             {"AGP_LAG": "0"}, {"AGP_LAG": "3"}, {"AGP_REFERENCE_ARITHMETIC": "1"}]


@pytest.mark.parametrize("env", SCHEDULES, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_poison_schedules_and_populations(pkg, monkeypatch, env):
    """Populations of 5 (right-looking), 12 (mixed launch), 70 (dataflow) and 260 (split diagonal launch, in-kernel
    evaluation) at ragged n, value and gradient sweeps, under every schedule switch: poisoned vs clean, bitwise.
    (The product library counts no schedule — which factorisation schedule, launch split or fusion a sweep took is not
    observable outside the measurement build — so only AGP_LAG=3 (toeplitz_particles) and the lag-table switches
    (lag_stats) are checked by a counter here; the schedule cases rely on the switches' documented effect.)"""
    pz, cl = engines(pkg, monkeypatch, env)
    try:
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(7), 260, max_depth=4, max_size=15)
        for n in (145, 257):
            ts, xs = pkg.prior.synthetic_series(n, seed=n + 3, shuffle=True)
            for e in (pz, cl):
                e.set_data(ts, xs)
            for P in (5, 12, 70, 260):
                lp, info = both(pz, cl, lambda e: e.logpdf_batch(nodes[:P], noises[:P], check=False), (env, n, P))
                finite_where_ok([lp], info, (env, n, P))
                assert (info == 0).sum() >= P - 3
            g = both(pz, cl, lambda e: e.logpdf_grad_batch(nodes[:24], noises[:24], check=False), (env, n, "grad"))
            finite_where_ok([g[0], g[2]], g[3], (env, n, "grad"))
        poisoned(pz)
        if env.get("AGP_LAG") == "3":
            assert pz.toeplitz_particles() > 0
        lag_on = env.get("AGP_LAG") != "0" and "AGP_REFERENCE_ARITHMETIC" not in env
        assert (pz.lag_stats()[1] > 0) == lag_on, pz.lag_stats()
    finally:
        close(pz, cl)


@pytest.mark.parametrize("n,P", [(1300, 70), (2048, 48)])
def test_poison_large_dataflow(pkg, monkeypatch, n, P):
    """The dataflow schedule at the sizes test_dataflow_schedule_vs_oracle uses: poisoned vs clean, bitwise."""
    pz, cl = engines(pkg, monkeypatch)
    try:
        ts, xs = pkg.prior.synthetic_series(n, seed=n, shuffle=True)
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n), P, max_depth=3, max_size=15)
        for e in (pz, cl):
            e.set_data(ts, xs)
        for m in (n, n - 77):
            lp, info = both(pz, cl, lambda e: e.logpdf_batch(nodes, noises, n=m, check=False), (n, m))
            finite_where_ok([lp], info, (n, m))
        poisoned(pz)
    finally:
        close(pz, cl)


# ---- 3. the factor store: extensions, growth, gradients and predictions from resident factors ------------------------------

def test_poison_store_extension_chain(pkg, monkeypatch):
    """Extension sweeps along 100 -> 128 -> 129 -> 144 -> 145 -> 256 -> 257 -> 300 -> 442 the way add_data! grows a series: the
    store is sized for the resident 300 points, then the series grows to 442 (agp_set_data keeps the store: the old series is a
    prefix) and the store is RESIZED while it holds factors — their prefix is copied, the remainder of every slot is fresh
    memory.  On the way, predictive passes at observed points keep and then extend the resident L^-T (zrows), and a gradient
    and a predictive pass start from the grown factors: poisoned vs clean, bitwise; the counters show extensions, the growth
    copy and reuse, not scratch sweeps."""
    pz, cl = engines(pkg, monkeypatch)
    try:
        ts, xs = irregular(442, 21)          # (general path before and after the growth: the store survives it)
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(21), 12, max_depth=3, max_size=15)
        tobs = ts[:60]

        def step(n):
            lp, info = both(pz, cl, lambda e: e.logpdf_batch_extend(nodes, noises, n=n, check=False), ("extend", n))
            finite_where_ok([lp], info, ("extend", n))

        def at_observed(n):
            r0 = pz.predict_reuse_stats()["reused"]
            pr = both(pz, cl, lambda e: e.predict_batch(nodes, noises, tobs, n=n, check=False), ("observed", n))
            finite_where_ok([pr[0], pr[1]], pr[3], ("observed", n))
            assert pz.predict_reuse_stats()["reused"] > r0
        for e in (pz, cl):
            e.set_data(ts[:300], xs[:300])
            e.extend_reserve(150, 12)
        for n in (100, 128, 129, 144, 145, 256):
            step(n)
        at_observed(256)                     # L^-T of the first two tile columns stays resident
        for n in (257, 300):
            step(n)
        at_observed(300)                     # ... and is extended from column 2
        s1 = pz.extend_stats()
        assert s1["capacity_tile_rows"] == 3 and s1["occupied"] > 0, s1
        for e in (pz, cl):
            e.set_data(ts, xs)
        step(442)
        s2 = pz.extend_stats()
        assert s2["capacity_tile_rows"] == 4 and s2["growth_copies"] > s1["growth_copies"], (s1, s2)
        assert s2["from_scratch"] == s1["from_scratch"] and s2["extended"] > s1["extended"], (s1, s2)
        assert s2["tile_rows_reused"] > s1["tile_rows_reused"]
        g = both(pz, cl, lambda e: e.logpdf_grad_batch(nodes, noises, n=442, check=False), "grad from store")
        finite_where_ok([g[0], g[2]], g[3], "grad from store")
        assert pz.grad_reuse_stats()["reused"] > 0
        tq = np.linspace(1.0, 1.2, 9)
        r0 = pz.predict_reuse_stats()["reused"]
        pr = both(pz, cl, lambda e: e.predict_batch(nodes, noises, tq, n=442, check=False), "predict from store")
        finite_where_ok([pr[0], pr[1]], pr[3], "predict from store")
        assert pz.predict_reuse_stats()["reused"] > r0
        poisoned(pz)
    finally:
        close(pz, cl)


# ---- 4. gradient paths -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env,counter", [({"AGP_LAG": "0"}, None), ({"AGP_GRAD_FFT": "1"}, "grad_lag_domain_particles"),
                                         ({"AGP_GRAD_FFT": "2"}, "grad_toeplitz_particles"),
                                         ({"AGP_GRAD_FFT": "4"}, "grad_structured_particles")])
def test_poison_gradient_paths(pkg, monkeypatch, env, counter):
    """Element-wise, lag-domain (power spectrum), Toeplitz and structured gradient sweeps at ragged n: bitwise."""
    G = pkg
    pz, cl = engines(pkg, monkeypatch, env)
    try:
        se, per, ge = G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.21, 1.1), G.GammaExponential(0.4, 1.3, 0.6)
        ks = [se, per, ge, se + per, per * se + ge, G.Linear(0.3, 0.2, 0.7) + se, G.ChangePoint(se, per, 0.5, 0.05)] * 2
        nz = np.linspace(0.02, 0.3, len(ks))
        for n in (129, 257, 442):
            ts, xs = pkg.prior.synthetic_series(n, seed=n + 11, shuffle=True)
            for e in (pz, cl):
                e.set_data(ts, xs)
                e.extend_reset()
            g = both(pz, cl, lambda e: e.logpdf_grad_batch(ks, nz, check=False), (env, n))
            finite_where_ok([g[0], g[2]], g[3], (env, n))
            assert (g[3] == 0).all()
        poisoned(pz)
        if counter is None:
            assert pz.grad_lag_domain_particles() == 0
        else:
            assert getattr(pz, counter)() > 0, counter
    finally:
        close(pz, cl)


# ---- 5. predictive paths -----------------------------------------------------------------------------------------------

def test_poison_predictive_paths(pkg, monkeypatch):
    """Lattice queries, training-point queries, mean functions, the structured pass (Toeplitz class, no dense factor) and the
    dense off-lattice pass with covariance: poisoned vs clean, bitwise.  Lattice passes and the structured pass are counted
    (lag_predict_passes, predict_structured_particles); the training-point, off-lattice and mean-function cases have no counter
    in the product library — the off-lattice case is checked by the lattice counter NOT moving."""
    G = pkg
    pz, cl = engines(pkg, monkeypatch)
    try:
        n = 257
        grid = np.linspace(0.0, 1.0, n); h = grid[1] - grid[0]
        perm = np.random.default_rng(5).permutation(n)
        ts = grid[perm]; xs = np.sin(7 * ts) + 0.1 * np.random.default_rng(5).standard_normal(n)
        for e in (pz, cl):
            e.set_data(ts, xs)
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(55), 9, max_depth=3, max_size=15)
        fut = 1.0 + h * np.arange(1, 40)
        cases = {"lattice": fut, "train": ts[:100], "offgrid": np.linspace(-0.05, 1.05, 33) + 0.3 * h}
        for name, tq in cases.items():
            k0 = pz.lag_predict_passes()
            pr = both(pz, cl, lambda e: e.predict_batch(nodes, noises, tq, want_cov=(name == "offgrid"), check=False), name)
            finite_where_ok([pr[0], pr[1]], pr[3], name)
            if name == "lattice":
                assert pz.lag_predict_passes() > k0
            if name == "offgrid":
                assert pz.lag_predict_passes() == k0
        mt = 0.3 * np.cos(5 * ts); mp_ = 0.3 * np.cos(5 * fut)
        pr = both(pz, cl, lambda e: e.predict_batch(nodes, noises, fut, mean_train=mt, mean_pred=mp_, check=False), "mean")
        finite_where_ok([pr[0], pr[1]], pr[3], "mean")
        se, per = G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.21, 1.1)
        cls = [se, per, se + per, per * se] * 10
        pr = both(pz, cl, lambda e: e.predict_batch(cls, np.linspace(0.01, 0.2, 40), fut, check=False), "structured")
        finite_where_ok([pr[0], pr[1]], pr[3], "structured")
        assert pz.predict_structured_particles() > 0
        poisoned(pz)
    finally:
        close(pz, cl)


# ---- 6. calendar series, the sum-of-GPs posterior, matrix assembly -------------------------------------------------------

@pytest.mark.parametrize("freq,n,kind", [("B", 300, 2), ("M", 300, 3)])
def test_poison_calendar_series(pkg, monkeypatch, freq, n, kind):
    pz, cl = engines(pkg, monkeypatch)
    try:
        ts, xs = pkg.prior.calendar_series(n, freq, seed=n, shuffle=True)
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n), 40, max_depth=3, max_size=15)
        for e in (pz, cl):
            e.set_data(ts, xs)
        assert pz.lattice_stats()["kind"] == kind
        for m in (n, n - 45):
            lp, info = both(pz, cl, lambda e: e.logpdf_batch(nodes, noises, n=m, check=False), (freq, m))
            finite_where_ok([lp], info, (freq, m))
        lpe, infoe = both(pz, cl, lambda e: e.logpdf_batch_extend(nodes[:12], noises[:12], n=n, check=False), (freq, "extend"))
        finite_where_ok([lpe], infoe, (freq, "extend"))
        if kind == 3:
            assert pz.compact_stats()["sweeps"] > 0
        poisoned(pz)
    finally:
        close(pz, cl)


def test_poison_infer_gp_sum_and_cov_matrix(pkg, monkeypatch):
    G = pkg
    pz, cl = engines(pkg, monkeypatch)
    try:
        ts, xs = irregular(145, 3)
        for e in (pz, cl):
            e.set_data(ts, xs)
        parts = [G.SquaredExponential(0.3, 0.8), G.Periodic(0.7, 0.21, 1.1), G.Linear(0.3, 0.2, 0.7)]
        tq = np.linspace(0.9, 1.2, 17)
        r = both(pz, cl, lambda e: e.infer_gp_sum(parts, 0.1, tq)[:2], "infer_gp_sum")
        assert np.isfinite(r[0]).all() and np.isfinite(r[1]).all()
        for m in (1, 17, 129):
            K = both(pz, cl, lambda e: e.cov_matrix(parts[0] + parts[1], 0.1, ts[:m]), ("cov", m))
            assert np.isfinite(K).all()
        poisoned(pz)
    finally:
        close(pz, cl)


# ---- 7. call order: one long-lived poisoned engine, a shuffled history with a singular particle -------------------------

def _history(pkg):
    """Steps (n, population) of a shuffled history: a large n, a smaller ragged n, a population with a singular particle (the
    recipe of test_lag_path_non_positive_definite_info: a smooth kernel without noise), then valid populations."""
    G = pkg
    rng = np.random.default_rng(31)
    steps = []
    for n, P in ((442, 12), (145, 5), (256, 12), (129, 70), (17, 5), (300, 12)):
        nodes, noises = pkg.prior.sample_particles(rng, P, max_depth=3, max_size=15)
        steps.append((n, list(nodes), np.asarray(noises, dtype=np.float64)))
    sing = [G.SquaredExponential(5.0, 1.0), G.SquaredExponential(0.1, 1.0) + G.Linear(0.2, 0.1, 1.0)]
    n, nodes, noises = steps[2]
    steps[2] = (n, sing + nodes[2:], np.concatenate([[0.0, 0.05], noises[2:]]))
    order = [0, 1, 2] + list(3 + rng.permutation(len(steps) - 3))
    return [steps[i] for i in order]


@pytest.mark.parametrize("mode", ["reference_arithmetic", "no_store"])
def test_poison_call_order_against_fresh_engines(pkg, monkeypatch, mode):
    """Reference arithmetic promises one arithmetic whatever the call order and the store's state, and without the store every
    sweep starts from scratch: so each call of a long poisoned history — NaNs left behind by a singular particle included —
    equals BITWISE the same call on a fresh clean engine with the same switches."""
    env = {"AGP_REFERENCE_ARITHMETIC": "1"} if mode == "reference_arithmetic" else {}
    pz, _unused = engines(pkg, monkeypatch, env)
    _unused.close()
    if mode == "no_store":
        pz.set_factor_cache(False)
    ts_all, xs_all = pkg.prior.synthetic_series(442, seed=77, shuffle=True)
    try:
        singular_seen = False
        for n, nodes, noises in _history(pkg):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            fresh = pkg.GPEngine(0)
            for k in env:
                monkeypatch.delenv(k)
            try:
                if mode == "no_store":
                    fresh.set_factor_cache(False)
                for e in (pz, fresh):
                    e.set_data(ts_all[:n], xs_all[:n])
                lp, info = both(pz, fresh, lambda e: e.logpdf_batch(nodes, noises, check=False), (mode, n, "batch"))
                finite_where_ok([lp], info, (mode, n))
                singular_seen |= bool((info > 0).any())
                g = both(pz, fresh, lambda e: e.logpdf_grad_batch(nodes[:5], noises[:5], check=False), (mode, n, "grad"))
                finite_where_ok([g[0], g[2]], g[3], (mode, n, "grad"))
                one = both(pz, fresh, lambda e: e.logpdf(nodes[-1], float(noises[-1]), check=False), (mode, n, "logpdf"))
                assert np.isfinite(one)
                tq = np.linspace(0.95, 1.1, 6)
                pr = both(pz, fresh, lambda e: e.predict_batch(nodes[-3:], noises[-3:], tq, check=False), (mode, n, "predict"))
                finite_where_ok([pr[0], pr[1]], pr[3], (mode, n, "predict"))
            finally:
                fresh.close()
        assert singular_seen
        poisoned(pz)
    finally:
        pz.close()


def test_poison_threaded_callers(pkg, monkeypatch):
    """Concurrent single-particle callers on a poisoned engine (test_coalescing_of_single_particle_gradient_callers' pattern and
    bounds).  Plain sweeps (store off): every caller gets the batch entry's result bit for bit.  Through the factor store the
    batches the coalescer forms depend on arrival times — a gradient caller may start from the factor its value-calling twin
    has just left — so only the existing rounding bounds hold there; every result must be finite either way."""
    pz, cl = engines(pkg, monkeypatch)
    cl.close()
    try:
        ts, xs = pkg.prior.synthetic_series(300, seed=21, shuffle=True)
        pz.set_data(ts, xs)
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(21), 24, max_depth=3, max_size=15)
        ref = pz.logpdf_grad_batch(nodes, noises, check=False)
        for cache in (False, True):
            pz.set_factor_cache(cache)
            f0 = pz.poison_stats()["fills"]
            out, errs = [None] * 48, []

            def work(i):
                j = i % 24
                try:
                    if i < 24:
                        out[i] = pz.logpdf_grad(nodes[j], float(noises[j]), check=False)
                    else:
                        out[i] = pz.logpdf(nodes[j], float(noises[j]), check=False)
                except Exception as ex:      # (reported below)
                    errs.append(ex)
            th = [threading.Thread(target=work, args=(i,)) for i in range(48)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            pz.set_factor_cache(True)
            assert not errs, errs
            assert pz.poison_stats()["fills"] > f0
            for i in range(24):
                if ref[3][i] != 0:
                    continue
                lp, g, gn = out[i]
                assert np.isfinite(lp) and np.isfinite(gn) and np.isfinite(g).all() and np.isfinite(out[24 + i]), i
                if not cache:
                    assert lp == ref[0][i] and gn == ref[2][i] and np.array_equal(g, ref[1][i]), i
                    # (value-only callers of a regular grid take the sorted lag-table sweep: equal to rounding)
                    assert abs(out[24 + i] - ref[0][i]) <= 1e-11 * max(1.0, abs(ref[0][i])), i
                else:
                    assert abs(lp - ref[0][i]) <= 1e-12 * max(1.0, abs(ref[0][i])) and abs(gn - ref[2][i]) <= 1e-9 * max(1.0, abs(ref[2][i])), i
                    assert np.all(np.abs(g - ref[1][i]) <= 1e-9 * np.maximum(1.0, np.abs(ref[1][i]))), i
                    assert abs(out[24 + i] - ref[0][i]) <= 1e-12 * max(1.0, abs(ref[0][i])), i
        poisoned(pz)
    finally:
        pz.close()


# ---- 8. the clean engine against the oracle at the ragged shapes ---------------------------------------------------------

# (test_logpdf_batch_vs_oracle already checks the value entry at 1, 2, 17, 127, 128, 129 and 256 points)
VALUE_SHAPES = [n for n in SHAPES if n not in (1, 2, 17, 127, 128, 129, 256)]


@pytest.mark.parametrize("n", SHAPES)
def test_ragged_shapes_vs_oracle(pkg, engine, n):
    """Value (where no existing test covers the shape), gradient and predictive pass of the clean engine against the oracle:
    LP_TOL, gradcheck.assert_grad_components (GRAD_TOL of the particle's scale and of every component's own), 1e-8.  n <= 17: well-conditioned particles also against the 60-digit oracle."""
    ts, xs = pkg.prior.synthetic_series(max(n, 2), seed=500 + n, shuffle=True)
    ts, xs = ts[:n], xs[:n]
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(500 + n), 12, max_depth=3, max_size=15)
    engine.set_data(ts, xs)
    progs = pkg.encode_batch(nodes)
    lp, info = engine.logpdf_batch(nodes, noises, check=False)
    ok = info == 0
    assert ok.sum() >= 8
    if n in VALUE_SHAPES:
        ref, rinfo = F.gp_logpdf_many(progs, noises, ts, xs)
        good = ok & (np.asarray(rinfo) == 0)
        assert lp_err(lp[good], np.asarray(ref)[good]).max() <= LP_TOL
    glp, grads, gn, ginfo = engine.logpdf_grad_batch(nodes[:6], noises[:6], check=False)
    for i in range(6):
        if ginfo[i] != 0:
            continue
        ref = GC.reference(nodes[i].to_tuple(), float(noises[i]), ts, xs)
        assert abs(glp[i] - ref.lp) <= LP_TOL * max(1.0, abs(ref.lp))
        GC.assert_grad_components(grads[i], gn[i], ref, tau=GRAD_TOL, ctx=(n, i))
    # (predictions: fixed, well-conditioned kernels — the oracle's LU solves carry cond(K) eps of their own)
    G = pkg
    pk = [G.Linear(0.3, 0.2, 0.5) + G.Periodic(0.4, 0.25, 0.6) * G.SquaredExponential(0.5, 1.0),
          G.SquaredExponential(0.2, 1.0) + G.GammaExponential(0.3, 1.2, 0.5), G.ChangePoint(G.Periodic(0.4, 0.25, 0.6), G.Constant(0.7), 0.5, 0.05),
          G.Linear(0.3, 0.2, 0.5)]
    pn = np.array([0.08, 0.1, 0.05, 0.2])
    tq = np.concatenate([np.linspace(-0.1, 1.1, 5), ts[: min(n, 2)]])
    mean, var, _, pinfo = engine.predict_batch(pk, pn, tq, check=False)
    assert (pinfo == 0).all()
    for i in range(4):
        mo, co = O.predict_mvn(pk[i].to_tuple(), float(pn[i]), ts, xs, tq)
        sc_m = max(1.0, np.abs(mo).max()); vo = np.diag(co); sc_v = max(1.0, np.abs(vo).max())
        assert np.abs(mean[i] - mo).max() <= 1e-8 * sc_m, (n, i)
        assert np.abs(var[i] - vo).max() <= 1e-8 * sc_v, (n, i)
    if n <= 17:
        from oracle import oracle_mp as M
        ops_off, ops, prm_off, prm = progs
        checked = 0
        for i in range(len(nodes)):
            if not ok[i]:
                continue
            pinfo_i, ratio = F.gp_pivot_ratio(ops[ops_off[i]:ops_off[i + 1]], prm[prm_off[i]:prm_off[i + 1]], float(noises[i]), ts)
            if pinfo_i != 0 or ratio <= 1e-8:
                continue
            ref = float(M.gp_logpdf_mp(nodes[i].to_tuple(), float(noises[i]), ts, xs))
            assert abs(lp[i] - ref) <= 1e-12 * max(1.0, abs(ref)), (n, i, lp[i], ref, ratio)
            checked += 1
        assert checked >= 3
