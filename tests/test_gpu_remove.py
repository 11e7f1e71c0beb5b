"""GPU tests of remove_data (agp_remove_data; remove_data!, src/api.jl:449-468): observations leave the resident series and the
resident factors are updated on the device instead of being refactored.  Particles: the test/test_GP.jl:24-33 kernels and
prior-sampled trees of depth <= 3, noise >= 1e-2 so that the oracle factors every case (asserted, nothing is skipped).
Tolerance, from the project: |dlogpdf| <= 1e-8 max(1, |logpdf|) against the oracle on the reduced series AND against a fresh
context given the reduced series; predictive mean / variance 1e-8 max(1, |.|_inf).

The admission rule measured on the hardware (remove_admits, profiles/remove_data_perf.txt) updates by default only single runs of at
most 8 rows with at least 2040 trailing rows; everywhere else the default drops the factors.  So that the update's arithmetic is
checked at EVERY size and removal the cases below name, they run with set_remove_update(2) — the update whatever the rule says —
and assert that every factor was updated and none dropped; test_default_rule_follows_the_measurement checks the rule in force.
Run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from oracle import fast as F
from oracle import gradcheck as GC

pytestmark = pytest.mark.gpu
LP_TOL = 1e-8


def lp_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def pred_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def population(pkg, seed, extra=5):
    G = pkg
    nodes = [G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
             G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1),
             G.Plus(G.SquaredExponential(0.47, 0.13), G.Periodic(0.96, 0.21, 1.1))]      # test/test_GP.jl:24-33 and a composite
    more, nz = pkg.prior.sample_particles(np.random.default_rng(seed), extra, max_depth=3, max_size=15)
    nodes = nodes + list(more)
    noises = np.concatenate([np.linspace(0.05, 0.3, 6), np.maximum(nz, 1e-2)])
    return nodes, noises


def series(pkg, kind, n, seed):
    if kind == "irregular":
        rng = np.random.default_rng(seed)
        ts = np.sort(rng.uniform(0.0, 1.0, n))
        _, xs = pkg.prior.synthetic_series(n, seed=seed)
        return np.ascontiguousarray(ts), xs
    if kind == "grid":
        return pkg.prior.synthetic_series(n, seed=seed, shuffle=True)
    return pkg.prior.calendar_series(n, freq="B", seed=seed)


def removal(name, n):
    if name == "front":
        return [0]
    if name == "back":
        return [n - 1]
    if name == "boundary":      # a run across the first tile boundary (or the middle of a short series)
        a = 126 if n > 130 else max(0, n // 2 - 1)
        return list(range(a, min(a + 3, n - 1)))
    if name == "scattered":
        return sorted(np.random.default_rng(n).choice(n, size=min(3, n - 1), replace=False).tolist())
    if name == "tile":          # r a multiple of 128
        return list(range(1, 129))
    return list(range(1, n))    # all but one point


def oracle_lp(pkg, nodes, noises, ts, xs):
    ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(nodes), noises, ts, xs)
    assert (rinfo == 0).all(), "the oracle must factor every case"
    return ref


@pytest.fixture()
def eng(pkg):
    e = pkg.GPEngine(0)
    e.set_remove_update(2)
    yield e
    e.close()


CASES = [(2, "irregular", "front"), (2, "irregular", "back"), (17, "grid", "scattered"), (17, "irregular", "all"),
         (129, "irregular", "front"), (129, "bday", "back"), (129, "grid", "boundary"),
         (300, "irregular", "front"), (300, "grid", "scattered"), (300, "bday", "boundary"), (300, "irregular", "tile"),
         (300, "irregular", "back"), (300, "grid", "all"),
         (1024, "irregular", "front"), (1024, "grid", "boundary"), (1024, "bday", "scattered"), (1024, "irregular", "tile"),
         (2048, "irregular", "front"), (2048, "grid", "scattered"), (2048, "irregular", "boundary"), (2048, "bday", "back"),
         (2048, "irregular", "tile"), (2048, "irregular", "all")]


@pytest.mark.parametrize("n,kind,what", CASES)
def test_remove_parity(pkg, eng, n, kind, what):
    """Score, remove, score again at the new n: equal to the oracle on the reduced series and to a fresh context given the reduced
    series.  Every factor must have been UPDATED (wide runs in several passes, scattered positions run by run): this fails without
    the feature."""
    ts, xs = series(pkg, kind, n, seed=n + len(what))
    nodes, noises = population(pkg, seed=n)
    idx = removal(what, n)
    keep = np.setdiff1d(np.arange(n), idx)
    eng.set_data(ts, xs)
    lp0, info0 = eng.logpdf_batch_extend(nodes, noises, check=False)
    assert (info0 == 0).all()
    assert eng.remove_data(idx) == len(keep) == eng.n_max
    st = eng.remove_stats()
    assert st["updated"] == len(nodes) and st["dropped"] == 0 and st["rows_removed"] == len(idx)
    # (a removal at the very end that leaves whole tile rows touches no tile: the factor stays as it is)
    assert st["panel_steps"] > 0 or (what == "back" and keep.size % 128 == 0)
    x0 = eng.extend_stats()
    lp, info = eng.logpdf_batch_extend(nodes, noises, check=False)
    x1 = eng.extend_stats()
    assert x1["extended"] - x0["extended"] == st["updated"] and x1["from_scratch"] - x0["from_scratch"] == st["dropped"]
    ref = oracle_lp(pkg, nodes, noises, ts[keep], xs[keep])
    print("remove parity", n, kind, what, "updated", st["updated"], "max err vs oracle", lp_err(lp, ref).max())
    assert (info == 0).all() and lp_err(lp, ref).max() <= LP_TOL
    fresh = pkg.GPEngine(0)
    try:
        fresh.set_data(ts[keep], xs[keep])
        lpf, inff = fresh.logpdf_batch_extend(nodes, noises, check=False)
    finally:
        fresh.close()
    assert (inff == 0).all() and lp_err(lp, lpf).max() <= LP_TOL


@pytest.mark.parametrize("n,what", [(300, "front"), (1024, "boundary"), (2048, "scattered")])
def test_switch_off_drops_the_factors_with_the_same_results(pkg, eng, n, what):
    ts, xs = series(pkg, "irregular", n, seed=7)
    nodes, noises = population(pkg, seed=n + 1)
    idx = removal(what, n)
    keep = np.setdiff1d(np.arange(n), idx)
    res = []
    for on in (2, 0):
        eng.set_data(ts, xs)
        eng.extend_reset()
        eng.set_remove_update(on)
        eng.logpdf_batch_extend(nodes, noises, check=False)
        s0 = eng.remove_stats()
        eng.remove_data(idx)
        s1 = eng.remove_stats()
        d = {k: s1[k] - s0[k] for k in s1}
        if on:
            assert d["updated"] == len(nodes) and d["dropped"] == 0
        else:
            assert d["updated"] == 0 and d["dropped"] == len(nodes) and d["panel_steps"] == 0
        res.append(eng.logpdf_batch_extend(nodes, noises, check=False))
    assert same(res[0][1], res[1][1]) and lp_err(res[0][0], res[1][0]).max() <= LP_TOL
    assert lp_err(res[0][0], oracle_lp(pkg, nodes, noises, ts[keep], xs[keep])).max() <= LP_TOL


def test_updated_slot_is_a_first_class_factor(pkg, eng):
    """After an update: an add_data-style extension starts from the slot, predict_batch reuses it, logpdf_grad_batch starts from
    it — each equal to the oracle."""
    import oracle.oracle as O
    n, n0 = 700, 600
    ts, xs = series(pkg, "irregular", n, seed=31)
    perm = np.random.default_rng(31).permutation(n)
    ts, xs = np.ascontiguousarray(ts[perm]), np.ascontiguousarray(xs[perm])
    nodes, noises = population(pkg, seed=31)
    idx = [5, 130, 131]
    keep = np.setdiff1d(np.arange(n0), idx)
    eng.set_data(ts[:n0], xs[:n0])
    eng.logpdf_batch_extend(nodes, noises, check=False)
    eng.remove_data(idx)
    assert eng.remove_stats()["updated"] == len(nodes)
    t1, x1 = ts[keep], xs[keep]
    # predictive pass on the updated factor
    tp = np.concatenate([t1[::50], np.linspace(1.0, 1.2, 40)])
    r0 = eng.predict_reuse_stats()["reused"]
    mean, var, _, info = eng.predict_batch(nodes, noises, tp, check=False)
    assert eng.predict_reuse_stats()["reused"] - r0 == len(nodes) and (info == 0).all()
    for i in range(len(nodes)):
        mu, cov = O.predict_mvn(nodes[i].to_tuple(), float(noises[i]), t1, x1, tp)
        assert pred_err(mean[i], mu) <= 1e-8 and pred_err(var[i], np.diag(cov)) <= 1e-8, i
    # gradient sweep starting from it
    g0 = eng.grad_reuse_stats()["reused"]
    got = eng.logpdf_grad_batch(nodes, noises, check=False)
    assert eng.grad_reuse_stats()["reused"] - g0 == len(nodes)
    refs = GC.references(nodes, noises, t1, x1)
    for i in range(len(nodes)):
        assert refs[i] is not None
        GC.assert_grad_components(got[1][i], got[2][i], refs[i], ctx=i)
    # add_data!: the reduced series is a prefix of the longer one, the sweep extends the updated factors
    t2, x2 = np.concatenate([t1, ts[n0:]]), np.concatenate([x1, xs[n0:]])
    eng.set_data(t2, x2)
    x0 = eng.extend_stats()
    lp, info = eng.logpdf_batch_extend(nodes, noises, check=False)
    xs1 = eng.extend_stats()
    assert xs1["extended"] - x0["extended"] == len(nodes) and xs1["from_scratch"] == x0["from_scratch"]
    assert (info == 0).all() and lp_err(lp, oracle_lp(pkg, nodes, noises, t2, x2)).max() <= LP_TOL


def test_updated_slot_predicts_on_its_own_error_scale(pkg, eng):
    """The updated factors end to end, output by output: the nine kernels of tests/_predict_cases.py at noise 1e-5, 1e-3 and 0.1 on
    300 irregular times, [0, 130, 131] removed (the first tile column's panel and applies, a run across the tile boundary), then
    predict_batch from the updated slots — every mean and variance within the resident route's own multiple of the reference
    routes' distance from the 80-bit values (oracle/predcheck.py; the multiples of tests/test_gpu_predict_components.py)."""
    import _predict_cases as PCS
    import test_gpu_predict_components as TPC
    n, idx = 300, [0, 130, 131]
    ts, xs = PCS.irregular_series(n, seed=431)
    keep = np.setdiff1d(np.arange(n), idx)
    c = PCS.Case("removed_300", ts[keep].copy(), xs[keep].copy(), keep.size, PCS.general_queries(ts[keep]))
    eng.set_data(ts, xs)
    _, info = eng.logpdf_batch_extend(c.nodes, c.noises, check=False)
    assert (info == 0).all()
    assert eng.remove_data(idx) == c.n
    st = eng.remove_stats()
    assert st["updated"] == len(c.nodes) and st["dropped"] == 0 and st["panel_steps"] > 0
    r0 = eng.predict_reuse_stats()["reused"]
    res = TPC.predict(eng, c)
    assert eng.predict_reuse_stats()["reused"] - r0 == len(c.nodes), eng.predict_reuse_stats()
    TPC.check_all("resident after remove_data", res, c, key="resident joint_300")


def test_sliding_window_of_40_steps(pkg, eng):
    """Remove the oldest point, append one, re-score: 40 steps at n = 300; every step within the tolerance of the oracle (no drift
    beyond it), every step an update followed by an extension."""
    n, steps = 300, 40
    ts, xs = series(pkg, "irregular", n + steps, seed=300)
    nodes, noises = population(pkg, seed=300)
    eng.set_data(ts[:n], xs[:n])
    eng.logpdf_batch_extend(nodes, noises, check=False)
    worst = 0.0
    for k in range(steps):
        eng.remove_data([0])
        lp_mid, info_mid = eng.logpdf_batch_extend(nodes, noises, check=False)      # the reference's smc_step! after deleteat!
        eng.set_data(ts[k + 1:n + k + 1], xs[k + 1:n + k + 1])                        # add_data!: one point appended
        lp, info = eng.logpdf_batch_extend(nodes, noises, check=False)
        ref_mid = oracle_lp(pkg, nodes, noises, ts[k + 1:n + k], xs[k + 1:n + k])
        ref = oracle_lp(pkg, nodes, noises, ts[k + 1:n + k + 1], xs[k + 1:n + k + 1])
        assert (info == 0).all() and (info_mid == 0).all()
        e = max(lp_err(lp, ref).max(), lp_err(lp_mid, ref_mid).max())
        worst = max(worst, e)
        assert e <= LP_TOL, (k, e)
    st, xt = eng.remove_stats(), eng.extend_stats()
    print("sliding window: worst error over", steps, "steps", worst)
    assert st["updated"] == steps * len(nodes) and st["dropped"] == 0
    assert xt["from_scratch"] == len(nodes)


def test_partially_covered_factors(pkg, eng):
    """A factor resident on a shorter prefix sees only the removed positions below its own length."""
    n = 300
    ts, xs = series(pkg, "irregular", n, seed=9)
    perm = np.random.default_rng(9).permutation(n)
    ts, xs = np.ascontiguousarray(ts[perm]), np.ascontiguousarray(xs[perm])
    nodes, noises = population(pkg, seed=9)
    eng.set_data(ts, xs)
    lp200, _ = eng.logpdf_batch_extend(nodes, noises, n=200, check=False)
    # beyond the prefix: untouched, same bits
    eng.remove_data([250])
    s = eng.remove_stats()
    assert s["updated"] == 0 and s["dropped"] == 0
    x0 = eng.extend_stats()
    again, _ = eng.logpdf_batch_extend(nodes, noises, n=200, check=False)
    assert same(again, lp200) and eng.extend_stats()["from_scratch"] == x0["from_scratch"]
    # partly below: prefix 200 loses position 150 only
    eng.remove_data([150, 260])
    s = eng.remove_stats()
    assert s["updated"] == len(nodes) and s["dropped"] == 0
    x0 = eng.extend_stats()
    lp, info = eng.logpdf_batch_extend(nodes, noises, n=199, check=False)
    x1 = eng.extend_stats()
    assert x1["from_scratch"] == x0["from_scratch"] and x1["tile_rows_reused"] - x0["tile_rows_reused"] == 2 * len(nodes)
    keep = np.setdiff1d(np.arange(200), [150])
    assert (info == 0).all() and lp_err(lp, oracle_lp(pkg, nodes, noises, ts[keep], xs[keep])).max() <= LP_TOL
    # and the whole reduced series extends from it
    keep_all = np.setdiff1d(np.arange(n), [150, 250, 261])
    lp, info = eng.logpdf_batch_extend(nodes, noises, check=False)
    assert eng.extend_stats()["from_scratch"] == x0["from_scratch"]
    assert lp_err(lp, oracle_lp(pkg, nodes, noises, ts[keep_all], xs[keep_all])).max() <= LP_TOL


def test_error_codes(pkg, eng):
    lib, ctx = eng._lib, eng._ctx

    def call(v):
        a = (C.c_int64 * max(1, len(v)))(*v)
        return lib.agp_remove_data(ctx, a, len(v))

    assert call([0]) == -4                                  # AGP_ERR_NODATA before agp_set_data
    ts, xs = series(pkg, "irregular", 50, seed=1)
    eng.set_data(ts, xs)
    for bad in ([], [3, 1], [2, 2], [-1], [50], [0, 50]):
        assert call(bad) == -1, bad                          # AGP_ERR_ARG
    assert lib.agp_remove_data(ctx, None, 1) == -1
    assert eng.n_max == 50 and call([49]) == 0
    out = (C.c_int64 * 4)()
    assert lib.agp_get_remove_stats(ctx, out, 4) == 0 and out[2] == 1
    assert lib.agp_get_remove_stats(ctx, None, 4) == -1


def test_poison_mode_is_bit_identical(pkg, monkeypatch):
    n = 300
    ts, xs = series(pkg, "irregular", n, seed=5)
    nodes, noises = population(pkg, seed=5)
    res = []
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        try:
            e.set_remove_update(2)
            e.set_data(ts, xs)
            e.logpdf_batch_extend(nodes, noises, check=False)
            e.remove_data([0, 1, 127, 200])
            assert e.remove_stats()["updated"] == len(nodes)
            res.append(e.logpdf_batch_extend(nodes, noises, check=False))
            e.remove_data(list(range(10, 50)))
            res.append(e.logpdf_batch_extend(nodes, noises, check=False))
        finally:
            e.close()
    assert same(res[0][0], res[2][0]) and same(res[1][0], res[3][0]) and np.isfinite(res[2][0]).all() and np.isfinite(res[3][0]).all()


def test_reference_arithmetic_only_edits_the_series(pkg, monkeypatch):
    monkeypatch.setenv("AGP_REFERENCE_ARITHMETIC", "1")
    n = 300
    ts, xs = series(pkg, "grid", n, seed=6)
    nodes, noises = population(pkg, seed=6)
    idx = [0, 5, 128, 129]
    keep = np.setdiff1d(np.arange(n), idx)
    a, b = pkg.GPEngine(0), pkg.GPEngine(0)
    try:
        a.set_data(ts, xs)
        a.logpdf_batch_extend(nodes, noises, check=False)
        a.remove_data(idx)
        s = a.remove_stats()
        assert s["updated"] == 0 and s["dropped"] == 0 and s["rows_removed"] == 4
        b.set_data(ts[keep], xs[keep])
        ra, rb = a.logpdf_batch_extend(nodes, noises, check=False), b.logpdf_batch_extend(nodes, noises, check=False)
        assert same(ra[0], rb[0]) and same(ra[1], rb[1])
    finally:
        a.close(); b.close()


def test_not_positive_definite_factor_is_dropped(pkg, eng):
    """0.1 I - 0.01 t t' fails at the 196th leading minor: its failed factor cannot be updated — the slot is gone after the removal
    and the next sweep reports the particle's info on the reduced series, as LAPACK does."""
    G = pkg
    ts = np.linspace(0, 1, 500); xs = np.sin(7 * ts)
    eng.set_data(ts, xs)
    bad, good = G.Linear(0.0, 0.0, -0.01), G.SquaredExponential(0.2, 1.0)
    nz = np.array([0.1, 0.1])
    _, info = eng.logpdf_batch_extend([bad, good], nz, check=False)
    assert info[0] == 196 and info[1] == 0
    occ = eng.extend_stats()["occupied"]
    eng.remove_data([3])
    s = eng.remove_stats()
    assert s["updated"] == 1 and s["dropped"] == 1 and eng.extend_stats()["occupied"] == occ - 1
    lp, info = eng.logpdf_batch_extend([bad, good], nz, check=False)
    keep = np.setdiff1d(np.arange(500), [3])
    ref, rinfo = F.gp_logpdf_many(pkg.encode_batch([bad, good]), nz, ts[keep], xs[keep])
    assert info[0] == rinfo[0] > 0 and np.isnan(lp[0]) and info[1] == 0 and lp_err(lp[1], ref[1]) <= LP_TOL


@pytest.mark.parametrize("n,idx,updates", [(2048, [0], True), (2060, list(range(8)), True), (2048, list(range(9)), False),
                                           (2048, [0, 2], False), (2048, [100], False), (300, [0], False)])
def test_default_rule_follows_the_measurement(pkg, n, idx, updates):
    """The rule in force (no switch set): single runs of at most 8 rows with at least 2040 trailing rows are updated, everything else
    is dropped and refactored by the next sweep — the same results either way."""
    ts, xs = series(pkg, "irregular", n, seed=n)
    nodes, noises = population(pkg, seed=n + 2)
    keep = np.setdiff1d(np.arange(n), idx)
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        e.logpdf_batch_extend(nodes, noises, check=False)
        e.remove_data(idx)
        st = e.remove_stats()
        assert (st["updated"], st["dropped"]) == ((len(nodes), 0) if updates else (0, len(nodes)))
        lp, info = e.logpdf_batch_extend(nodes, noises, check=False)
        assert (info == 0).all() and lp_err(lp, oracle_lp(pkg, nodes, noises, ts[keep], xs[keep])).max() <= LP_TOL
    finally:
        e.close()
