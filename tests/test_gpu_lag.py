"""GPU tests of the regular-grid path (include/autogp_hip.h "Regular time grids"; csrc/agp_cov_kernel.hpp lag tables): value
sweeps over the whole of a regularly spaced series run on a sorted copy and read stationary leaves from per-tile lag tables.
Checked against the oracle (1e-8, BASELINE.json's tolerance), against the general path of the same engine (1e-10: the two differ
by the rounding of t_i - t_j and by the pivot order) in every schedule regime, and that everything which must NOT take the path —
prefixes, irregular series, jittered grids — does not."""
import numpy as np
import pytest

from oracle import fast as F
from oracle import gradcheck as GC
from oracle.predcheck import predict_80bit

import _sweep_cases as SWEEP_CASES

pytestmark = pytest.mark.gpu
LP_TOL = 1e-8


def lp_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def both_paths(pkg, nodes, noises, ts, xs, n=None):
    """(lag-path values, general-path values, lag sweeps counted) from two contexts over the same data."""
    a = pkg.GPEngine(0); b = pkg.GPEngine(0)
    try:
        b.set_lag_tables(False)
        a.set_data(ts, xs); b.set_data(ts, xs)
        before = a.lag_stats()[1]
        la, ia = a.logpdf_batch(nodes, noises, n=n, check=False)
        took = a.lag_stats()[1] - before
        lb, ib = b.logpdf_batch(nodes, noises, n=n, check=False)
        assert b.lag_stats() == (False, 0)
        return la, ia, lb, ib, took, a.lag_stats()[0]
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n,P,depth", [(640, 300, 3),      # >= 256 particles: per-column launches, tiles evaluated in-kernel
                                        (768, 40, 3),       # dataflow schedule
                                        (700, 3, 3),        # right-looking schedule, tiles prebuilt by k_cov_tiles (n not a tile multiple)
                                        (128, 9, 2), (129, 9, 2), (2, 4, 2),
                                        (1024, 24, 6)])     # deep trees: depth-8 evaluation stack, many tables
def test_lag_path_vs_oracle_and_general_path(pkg, n, P, depth):
    ts, xs = pkg.prior.synthetic_series(n, seed=900 + n, shuffle=True)
    kw = dict(max_depth=depth) if depth < 6 else dict(max_depth=6, min_depth=5, max_size=63)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n + P), P, **kw)
    la, ia, lb, ib, took, regular = both_paths(pkg, nodes, noises, ts, xs)
    assert regular and took >= 1, "the sweep did not take the lag-table path"
    assert np.array_equal(ia == 0, ib == 0) or (np.sum((ia == 0) != (ib == 0)) <= 1)
    ok = (ia == 0) & (ib == 0)
    assert ok.mean() >= 0.9
    assert lp_err(la[ok], lb[ok]).max() <= 1e-10
    ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(nodes), noises, ts, xs)
    both = ok & (rinfo == 0)
    assert lp_err(la[both], ref[both]).max() <= LP_TOL
    # rejected particles carry LAPACK's info of the CALLER's order (repaired by a second factorisation in that order)
    bad = (ia > 0) & (ib > 0)
    assert np.array_equal(ia[bad], ib[bad])


def test_lag_path_fixture_kernels_and_changepoints(pkg):
    """Every leaf kind and combinator (test/test_GP.jl:24-33 kernels and their composites), incl. WhiteNoise (the identity
    survives the sort), ChangePoint with its per-point tables next to the lag tables, and an unsorted regular grid with an offset
    and a negative range."""
    G = pkg
    base = [G.WhiteNoise(0.3), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
            G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1)]
    ks = list(base[2:])
    for x in base:
        for y in base[3:]:
            ks += [x + y, x * y, G.ChangePoint(x, y, 0.5, 0.05), G.ChangePoint(y, x * y, 0.3, 0.001)]
    nz = np.full(len(ks), 0.07)
    for t0, t1, n in ((0.0, 1.0, 300), (-3.0, 2.0, 257), (5.0, 5.5, 128)):
        ts = np.linspace(t0, t1, n)
        rng = np.random.default_rng(n)
        perm = rng.permutation(n)
        ts = ts[perm]; xs = np.sin(5 * ts) + 0.1 * rng.standard_normal(n)
        la, ia, lb, ib, took, regular = both_paths(pkg, ks, nz, ts, xs)
        assert regular and took >= 1
        assert (ia == 0).all() and (ib == 0).all()
        assert lp_err(la, lb).max() <= 1e-10
        ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(ks), nz, ts, xs)
        assert (rinfo == 0).all() and lp_err(la, ref).max() <= LP_TOL


def test_what_must_not_take_the_lag_path(pkg):
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(5), 12, max_depth=3)
    eng = pkg.GPEngine(0)
    try:
        # prefixes of a shuffled grid are not grids
        ts, xs = pkg.prior.synthetic_series(512, seed=4, shuffle=True)
        eng.set_data(ts, xs)
        assert eng.lag_stats() == (True, 0)
        lp, info = eng.logpdf_batch(nodes, noises, n=300, check=False)
        assert eng.lag_stats() == (True, 0)
        ref, _ = F.gp_logpdf_many(pkg.encode_batch(nodes), noises, ts[:300], xs[:300])
        ok = info == 0
        assert lp_err(lp[ok], ref[ok]).max() <= LP_TOL
        assert eng.lag_rank_sweeps() == 1            # (the prefix sweep read its stationary leaves from rank tables instead)
        eng.logpdf_batch(nodes, noises, check=False)
        assert eng.lag_stats() == (True, 1) and eng.lag_rank_sweeps() == 1
        # gradient, extension and predictive entries keep the caller's order (the gradient sweep's factorisation: rank tables)
        eng.logpdf_grad_batch(nodes, noises, check=False)
        assert eng.lag_rank_sweeps() == 2
        eng.logpdf_batch_extend(nodes, noises, check=False)
        eng.predict_batch(nodes[:2], noises[:2], np.linspace(0, 1.1, 20), check=False)
        assert eng.lag_stats() == (True, 1) and eng.lag_rank_sweeps() == 2
        # a grid jittered by 1e-9 (relative), by 1e-13 (inside the former 16-ulp-of-|t| bound, 4e-11 spacings), a random series, a grid
        # with one point missing and with a duplicate
        rng = np.random.default_rng(0)
        grid = np.linspace(0.0, 1.0, 400)
        for bad in (grid * (1 + 1e-9 * rng.standard_normal(400)), grid + 1e-13 * np.cos(np.arange(400.0)) * (grid > 0) * (grid < 1),
                    np.sort(rng.random(400)), np.delete(grid, 17),
                    np.concatenate([grid[:200], grid[199:]])):
            eng.set_data(bad, np.cos(3 * bad))
            assert eng.lag_stats()[0] is False
            lp, info = eng.logpdf_batch(nodes[:4], noises[:4], check=False)
            ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(nodes[:4]), noises[:4], bad, np.cos(3 * bad))
            ok = (info == 0) & (rinfo == 0)
            assert lp_err(lp[ok], ref[ok]).max() <= LP_TOL
        # (the grid with one point missing is a lattice with a gap: not a regular grid, but its sweep reads rank tables — tests/test_gpu_calendar.py)
        assert eng.lag_stats()[1] == 1 and eng.lag_rank_sweeps() == 3
    finally:
        eng.close()


def _short_scale_population(pkg, rng, span):
    """Kernels whose values move fastest with the time differences: lengthscales ~0.01 of the series' span, periods ~0.015 of it
    (the reference's raw-space calls, test/test_GP.jl:35-68, use parameters in the units of the time axis)."""
    G = pkg
    l, p = 0.01 * span, 0.015 * span
    ks = [G.SquaredExponential(l, 0.9), G.Periodic(0.5, p, 1.1), G.GammaExponential(l, 1.0, 0.7), G.GammaExponential(2 * l, 1.9, 0.6),
          G.Periodic(0.8, p, 1.0) * G.SquaredExponential(20 * l, 0.8), G.SquaredExponential(l, 0.5) + G.Periodic(0.6, 1.3 * p, 0.4),
          G.GammaExponential(l, 0.6, 0.5) + G.Constant(0.2), G.Periodic(1.2, 0.7 * p, 0.9) + G.WhiteNoise(0.01)]
    nz = 0.02 + 0.2 * rng.random(len(ks))
    return ks, nz


@pytest.mark.parametrize("case", ["offset_1e3", "offset_1e5", "appended", "inside", "outside", "unit"])
def test_regular_grid_admission_is_tied_to_the_spacing(pkg, case):
    """agp_set_data admits a series to the lag path when every sorted point sits within 1e-11 SPACINGS of t_0 + g h, one ulp of |t|max included (the tables
    replace t_i - t_j by t_sorted[g] - t_sorted[0]: the admitted relative error of the smallest lag is ~1e-11).  Grids with a
    large offset (add_data! keeps the old transform, src/api.jl:434; raw-space calls as in test/test_GP.jl:35-68) and grids
    jittered below the former 16-ulp-of-|t| bound must be REFUSED; what is admitted must meet 1e-8 against the oracle and 1e-10
    against the general path with short-lengthscale kernels at n = 2048."""
    n = 2048
    rng = np.random.default_rng(12)
    base = np.linspace(0.0, 1.0, n)
    h = base[1] - base[0]
    if case == "offset_1e3":   tg, expect = np.linspace(1000.0, 1001.0, n), False        # ulp(1000) / h = 4.6e-10
    elif case == "offset_1e5": tg, expect = np.linspace(1e5, 1e5 + 1.0, n), False        # ulp(1e5) / h = 3e-8
    elif case == "appended":   tg, expect = np.concatenate([base, 1.0 + h * np.arange(1, 1025)]), None      # add_data!: [0, 1.5]
    elif case == "inside":     tg, expect = base + 1e-15 * np.sign(np.sin(7.0 * np.arange(n))) * (np.arange(n) % 5 != 0), True     # 2.7e-12 h
    elif case == "outside":    tg, expect = base + 8e-15 * np.sign(np.sin(7.0 * np.arange(n))) * (np.arange(n) % 5 != 0), False    # 1.7e-11 h
    else:                      tg, expect = base, True
    tg = np.asarray(tg, dtype=np.float64)
    if case in ("inside", "outside"): tg[0], tg[-1] = base[0], base[-1]      # (end points define the grid)
    span = tg.max() - tg.min()
    ks, nz = _short_scale_population(pkg, rng, span)
    perm = rng.permutation(len(tg))
    ts = tg[perm]
    xs = np.sin(40.0 * (ts - tg.min()) / span) + 0.3 * rng.standard_normal(len(ts))
    la, ia, lb, ib, took, regular = both_paths(pkg, ks, nz, ts, xs)
    if expect is not None: assert regular is expect, (case, regular)
    assert (took >= 1) == bool(regular)
    assert (ia == 0).all() and (ib == 0).all()
    assert lp_err(la, lb).max() <= 1e-10, (case, lp_err(la, lb).max())
    ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(ks), nz, ts, xs)
    assert (rinfo == 0).all() and lp_err(la, ref).max() <= LP_TOL, (case, lp_err(la, ref).max())
    # rank tables (an annealing prefix in the caller's order) and the lag-domain gradient follow the same admission
    eng = pkg.GPEngine(0)
    try:
        eng.set_data(ts, xs)
        m = len(ts) - 200
        lp, info = eng.logpdf_batch(ks, nz, n=m, check=False)
        assert (eng.lag_rank_sweeps() == 1) == bool(regular) or len(ts) > 4096
        refm, _ = F.gp_logpdf_many(pkg.encode_batch(ks), nz, ts[:m], xs[:m])
        assert (info == 0).all() and lp_err(lp, refm).max() <= LP_TOL
    finally:
        eng.close()


@pytest.mark.parametrize("n_max,n,P,depth", [(640, 500, 300, 3),     # per-column launches
                                              (768, 700, 40, 3),      # dataflow schedule
                                              (700, 650, 3, 3),       # right-looking schedule, tiles prebuilt
                                              (300, 129, 9, 2), (300, 2, 4, 2),
                                              (1024, 900, 24, 6),     # deep trees: many tables, most tiles prebuilt
                                              (2048, 1845, 64, -1),   # an annealing prefix of config 3, one GPU's share
                                              (4096, 3000, 6, 3)])    # 32 KiB tables
def test_rank_lag_tables_prefix_sweeps(pkg, monkeypatch, n_max, n, P, depth):
    """Prefix sweeps of a shuffled regular grid keep the caller's order and read stationary subtrees from rank tables
    (table[|rank_a - rank_b|]): against the general path of a second context (1e-10), the oracle (1e-8), and LAPACK's info."""
    ts, xs = pkg.prior.synthetic_series(n_max, seed=300 + n_max, shuffle=True)
    kw = dict(max_depth=depth) if 0 < depth < 6 else (dict(max_depth=6, min_depth=5, max_size=63) if depth == 6 else dict(max_depth=-1, max_size=63))
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(n + P), P, **kw)
    a = pkg.GPEngine(0)
    monkeypatch.setenv("AGP_LAG_RANK", "0")
    b = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_LAG_RANK")
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        la, ia = a.logpdf_batch(nodes, noises, n=n, check=False)
        lb, ib = b.logpdf_batch(nodes, noises, n=n, check=False)
        assert a.lag_rank_sweeps() == 1 and b.lag_rank_sweeps() == 0 and a.lag_stats()[1] == 0
        assert np.sum((ia == 0) != (ib == 0)) <= 1
        ok = (ia == 0) & (ib == 0)
        assert ok.mean() >= 0.9 and lp_err(la[ok], lb[ok]).max() <= 1e-10
        bad = (ia > 0) & (ib > 0)
        assert np.array_equal(ia[bad], ib[bad])
        if n <= 2048:
            ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(nodes), noises, ts[:n], xs[:n])
            both = ok & (rinfo == 0)
            assert lp_err(la[both], ref[both]).max() <= LP_TOL
        # the value a gradient sweep reports comes from the same factorisation
        if P <= 64 and n <= 1024:
            lg, _, _, ig = a.logpdf_grad_batch(nodes, noises, n=n, check=False)
            assert np.array_equal(ig, ia) and lp_err(lg[ok], la[ok]).max() <= 1e-11
        a.set_lag_rank_tables(False)
        lc, ic = a.logpdf_batch(nodes, noises, n=n, check=False)
        assert a.lag_rank_sweeps() <= 2 and np.array_equal(lc[ok], lb[ok])
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("case", ["duplicates", "future", "interleaved", "backcast", "prefix", "off_grid", "too_long", "many"])
def test_predictive_pass_on_lattice_query_points(pkg, case):
    """agp_predict_batch with query points on the series' own lattice (scripts/online.jl:41-43: ds_query = vcat(model.ds, ds_next,
    ds_test); src/GP.jl:743) reads the stationary subtrees from rank tables: duplicates of training times, future-only points,
    both interleaved, points before the series, a prefix n < n_max; one off-lattice point or more than 4096 lags -> general path.
    Mean, variance and covariance against the oracle (1e-8) and against a context without lag tables (1e-10 of the scale)."""
    from oracle import oracle as O
    G = pkg
    n_max, n = 300, 300
    grid = np.linspace(0.0, 1.0, n_max)
    h = grid[1] - grid[0]
    rng = np.random.default_rng(17)
    perm = rng.permutation(n_max)
    ts = grid[perm]; xs = np.sin(7 * ts) + 0.2 * rng.standard_normal(n_max)
    fut = grid[0] + h * np.arange(n_max, n_max + 40)
    if case == "duplicates":    tq, on = ts[rng.permutation(n_max)[:200]], True
    elif case == "future":      tq, on = fut, True
    elif case == "interleaved": tq, on = np.concatenate([ts[:150], fut[:25], ts[150:], fut[25:]]), True
    elif case == "backcast":    tq, on = np.concatenate([grid[0] - h * np.arange(1, 30), ts[:20], fut[:5]]), True
    elif case == "prefix":      tq, on, n = np.concatenate([ts, fut]), True, 170          # (the rest of the series is "ds_next")
    elif case == "off_grid":    tq, on = np.concatenate([ts[:50], [grid[10] + 0.3 * h], fut[:5]]), False
    elif case == "too_long":    tq, on = grid[0] + h * np.arange(0, 5000, 100), False      # ranks up to 4900 > 4096 lags (the LDS budget of a rank table)
    else:                       tq, on = np.concatenate([ts, fut]), True
    ks = [G.SquaredExponential(0.1, 0.8), G.Periodic(0.7, 0.21, 1.1) * G.SquaredExponential(0.5, 0.9) + G.Linear(0.3, 0.2, 0.5),
          G.GammaExponential(0.3, 1.2, 0.7) + G.WhiteNoise(0.05), G.ChangePoint(G.Periodic(0.5, 0.1, 1.0), G.SquaredExponential(0.2, 0.6), 0.45, 0.01),
          G.Linear(0.1, 0.3, 0.7), G.Constant(0.3) + G.GammaExponential(0.15, 0.8, 0.5) * G.Periodic(1.0, 0.3, 0.8)]
    nz = np.linspace(0.05, 0.2, len(ks))
    if case == "many":      # a population on the dataflow / per-column schedules, duplicates among the particles
        nodes, nzs = pkg.prior.sample_particles(np.random.default_rng(3), 70, max_depth=3)
        ks = list(nodes) + ks + [ks[0]]; nz = np.concatenate([nzs, nz, nz[:1]])
    a = pkg.GPEngine(0); b = pkg.GPEngine(0)
    try:
        b.set_lag_tables(False)
        a.set_data(ts, xs); b.set_data(ts, xs)
        for want_cov in (False, True):
            k0 = a.lag_predict_passes()
            ma, va, ca, ia = a.predict_batch(ks, nz, tq, n=n, want_cov=want_cov, check=False)
            assert (a.lag_predict_passes() - k0 == 1) == on, case
            mb, vb, cb, ib = b.predict_batch(ks, nz, tq, n=n, want_cov=want_cov, check=False)
            assert b.lag_predict_passes() == 0 and np.array_equal(ia, ib)
            ok = ia == 0
            assert ok.mean() >= 0.9
            sc = np.maximum(1.0, np.abs(mb[ok]).max(axis=1))[:, None]
            assert (np.abs(ma[ok] - mb[ok]) / sc).max() <= 1e-10 and (np.abs(va[ok] - vb[ok]) / np.maximum(1.0, vb[ok])).max() <= 1e-10
            if want_cov:
                assert np.abs(ca[ok] - cb[ok]).max() <= 1e-10 * max(1.0, np.abs(cb[ok]).max())
        for i in range(len(ks) - 6 - (case == "many"), len(ks) - (case == "many")):          # the hand-written kernels against the oracle
            mu, cv = O.predict_mvn(ks[i].to_tuple(), float(nz[i]), ts[:n], xs[:n], tq)
            assert np.abs(ma[i] - mu).max() <= LP_TOL * max(1.0, np.abs(mu).max()), (case, i)
            assert np.abs(ca[i] - cv).max() <= LP_TOL * max(1.0, np.abs(cv).max()), (case, i)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("case", ["train_only", "train_future", "scattered", "means", "general_times", "reuse", "population", "below_threshold"])
def test_predictive_pass_on_training_point_queries(pkg, case):
    """Query points that are training points (scripts/online.jl:41-43: ds_query starts with model.ds) and no covariance request:
    mean and marginal variance come from alpha and diag(K11^-1) (row sums of squares of L^-T), the remaining queries from the
    joint matrix.  Against the oracle (src/GP.jl:739-757 restated) and against the same call with the covariance requested,
    which never takes this route."""
    from oracle import oracle as O
    G = pkg
    rng = np.random.default_rng(5)
    n_max, n = 420, 390
    if case == "general_times":
        ts = np.sort(rng.uniform(0.0, 1.0, n_max)); ts[7] = 0.0          # (+0.0 / -0.0 compare equal)
    else:
        ts = np.linspace(0.0, 1.0, n_max)[rng.permutation(n_max)]
    xs = np.cos(9 * ts) + 0.3 * ts + 0.1 * rng.standard_normal(n_max)
    h = 1.0 / (n_max - 1)
    fut = 1.0 + h * np.arange(1, 61)
    if case == "train_only":        tq = ts[:n].copy()
    elif case == "scattered":       tq = np.concatenate([fut[:7], ts[rng.permutation(n)[:300]], [0.3337], ts[:40], fut[7:]])    # repeats among the queries
    elif case == "below_threshold": tq = np.concatenate([ts[:100], fut])          # too few duplicates: joint path
    else:                           tq = np.concatenate([ts[:n_max], fut])
    if case == "general_times":     tq[7] = -0.0
    ks = [G.SquaredExponential(0.1, 0.8), G.Periodic(0.7, 0.21, 1.1) * G.SquaredExponential(0.5, 0.9) + G.Linear(0.3, 0.2, 0.5),
          G.GammaExponential(0.3, 1.2, 0.7) + G.WhiteNoise(0.05), G.ChangePoint(G.Periodic(0.5, 0.1, 1.0), G.SquaredExponential(0.2, 0.6), 0.45, 0.01),
          G.Linear(0.1, 0.3, 0.7), G.Constant(0.3) + G.GammaExponential(0.15, 0.8, 0.5) * G.Periodic(1.0, 0.3, 0.8)]
    nz = np.linspace(0.01, 0.2, len(ks)); npred = np.linspace(0.3, 0.02, len(ks))
    n_or = len(ks)
    if case == "population":
        nodes, nzs = pkg.prior.sample_particles(np.random.default_rng(3), 90, max_depth=3)
        ks = ks + list(nodes); nz = np.concatenate([nz, nzs]); npred = np.concatenate([npred, 0.5 * nzs])
    kw = {}
    mean_fn = None
    if case == "means":
        mean_fn = lambda t: 0.4 - 1.3 * t
        kw = dict(mean_train=np.array([mean_fn(t) for t in ts[:n]]), mean_pred=np.array([mean_fn(t) for t in tq]))
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        if case == "reuse":         # factors of exactly this prefix are resident
            e.logpdf_batch_extend(ks, nz, n=n, check=False)
        r0 = e.predict_reuse_stats()["reused"]
        m1, v1, _, i1 = e.predict_batch(ks, nz, tq, n=n, noise_pred=npred, want_cov=False, check=False, **kw)
        assert (e.predict_reuse_stats()["reused"] - r0 > 0) == (case == "reuse")
        m2, v2, c2, i2 = e.predict_batch(ks, nz, tq, n=n, noise_pred=npred, want_cov=True, check=False, **kw)
        assert np.array_equal(i1, i2)
        ok = i1 == 0
        assert ok[:n_or].all() and ok.mean() >= 0.9
        assert np.isnan(m1[~ok]).all() and np.isnan(v1[~ok]).all()
        sc = np.maximum(1.0, np.abs(m2[ok]).max(axis=1))[:, None]
        assert (np.abs(m1[ok] - m2[ok]) / sc).max() <= 1e-9
        assert (np.abs(v1[ok] - v2[ok]) / np.maximum(1.0, v2[ok])).max() <= 1e-9
        assert np.allclose(np.diagonal(c2[ok], axis1=1, axis2=2), v2[ok], rtol=0, atol=1e-12)
        for i in range(n_or):
            mu, cv = O.predict_mvn(ks[i].to_tuple(), float(nz[i]), ts[:n], xs[:n], tq, noise_pred=float(npred[i]), mean=mean_fn)
            assert np.abs(m1[i] - mu).max() <= LP_TOL * max(1.0, np.abs(mu).max()), (case, i)
            assert np.abs(v1[i] - np.diag(cv)).max() <= LP_TOL * max(1.0, np.abs(cv).max()), (case, i)
    finally:
        e.close()


@pytest.mark.parametrize("case", ["train_and_future", "means", "future_only", "train_only", "prefix_in_time_order", "population_2048", "backcast", "refused", "linear_far_centre"])
def test_predictive_pass_structured(pkg, monkeypatch, case):
    """Predictive pass WITHOUT a dense factor for the Toeplitz + rank-2 class (csrc/agp_predict.hip toeplitz_predict_sweep: joint
    Schur recursion, backward substitution, Gohberg-Semencul diagonal, Bayesian linear model for the Linear leaves): training points
    consecutive on the grid, queries = any of them and / or grid points after them (scripts/online.jl:41-43).  Against the dense pass
    (AGP_GRAD_FFT=2: 1e-9 of the scale) and the oracle (src/GP.jl:739-757 restated); a point before the series, or a matrix that is
    not positive definite, goes to the dense path."""
    from oracle import oracle as O
    G = pkg
    rng = np.random.default_rng(3)
    covered, elementwise, n_poly = _grad_shapes(G)
    base = covered[:len(covered) - n_poly]
    ks = base * 3 + elementwise
    nz = np.linspace(0.01, 0.25, len(ks)); npred = np.linspace(0.3, 0.02, len(ks))
    n_max = 420
    grid = np.linspace(0.0, 1.0, n_max); h = grid[1] - grid[0]
    perm = rng.permutation(n_max)
    ts = grid[perm]; n = n_max
    fut = 1.0 + h * np.arange(1, 90)
    n_cls = 3 * len(base)
    if case == "future_only":      tq = fut[rng.permutation(fut.size)]
    elif case == "train_only":     tq = ts[rng.permutation(n_max)[:300]]
    elif case == "backcast":       tq = np.concatenate([ts[:50], [grid[0] - h], fut[:5]]); n_cls = 0
    elif case == "prefix_in_time_order":
        ts = grid.copy(); n = 333
        tq = np.concatenate([ts[:n][::-1], grid[n:], fut])          # (the rest of the series are "future" points here)
    elif case == "population_2048":
        n_max = n = 2048
        ts, _ = pkg.prior.synthetic_series(n_max, seed=13, shuffle=True)
        gs = np.sort(ts); h = gs[1] - gs[0]
        ks, nz = pkg.prior.sample_particles(np.random.default_rng(31), 96, max_depth=-1, max_size=31)
        npred = 0.5 * nz
        tq = np.concatenate([ts, gs[-1] + h * np.arange(1, 513)]); n_cls = None
    else:                          tq = np.concatenate([fut[:7], ts[rng.permutation(n_max)[:200]], ts[:40], fut[7:]])
    if case == "linear_far_centre":
        # Linear leaves centred far from the data and a small noise: (I + N C) is of the order 1e5..1e7 — the future-point mean must not
        # be formed as a difference of near-equal terms (h' C (U'a - N S U'a) lost 1e-7 of the scale; h' S U'a is the same quantity)
        ks = [G.Linear(c0, b0, a0) for c0 in (7.0, 15.0, -9.0, 0.24) for b0 in (0.04, 0.5) for a0 in (0.5, 1.0, 2.2, 4.0, 9.0)]
        nz = np.full(len(ks), 0.02); npred = np.full(len(ks), 0.02); n_cls = len(ks)
    if case == "refused":
        ks = [G.SquaredExponential(5.0, 1.0)] + ks; nz = np.concatenate([[0.0], nz]); npred = np.concatenate([[0.1], npred]); n_cls = n_cls  # particle 0: singular
    xs = np.cos(9 * ts) + 0.3 * ts + 0.1 * rng.standard_normal(ts.size)
    kw = {}; mean_fn = None
    if case == "means":
        mean_fn = lambda t: 0.4 - 1.3 * t
        kw = dict(mean_train=np.array([mean_fn(t) for t in ts[:n]]), mean_pred=np.array([mean_fn(t) for t in tq]))
    a = pkg.GPEngine(0)
    monkeypatch.setenv("AGP_GRAD_FFT", "2")
    b = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_FFT")
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        m1, v1, _, i1 = a.predict_batch(ks, nz, tq, n=n, noise_pred=npred, check=False, **kw)
        m2, v2, _, i2 = b.predict_batch(ks, nz, tq, n=n, noise_pred=npred, check=False, **kw)
        k = a.predict_structured_particles()
        assert b.predict_structured_particles() == 0
        if n_cls is None: assert k >= len(ks) // 2
        else: assert k == n_cls, (case, k)
        assert np.array_equal(i1 > 0, i2 > 0)
        if case == "refused": assert i1[0] > 0 and np.isnan(m1[0]).all()
        ok = i1 == 0
        sc = np.maximum(1.0, np.abs(m2[ok]).max(axis=1))[:, None]
        far = case == "linear_far_centre"      # (conditioning 1e7..1e8: the dense pass and the oracle keep 1e-9; an 80-bit factorisation is the judge)
        assert (np.abs(m1[ok] - m2[ok]) / sc).max() <= (1e-7 if far else 1e-9)
        assert (np.abs(v1[ok] - v2[ok]) / np.maximum(1.0, v2[ok])).max() <= 1e-9
        if far:
            for i in range(0, len(ks), 3):
                ml, vl = predict_80bit(ks[i].to_tuple(), float(nz[i]), ts[:n], xs[:n], tq, float(npred[i]))
                assert np.abs(m1[i] - ml).max() <= 1e-9 * max(1.0, np.abs(ml).max()), (case, i)   # (the entries of K are rounded to double: 1e-16 x conditioning)
                assert np.abs(v1[i] - vl).max() <= 1e-9 * max(1.0, np.abs(vl).max()), (case, i)
        elif case == "population_2048":
            # at the size the bench quotes (n = 2048, 2560 query points): the oracle's full-size predictive restatement on worker
            # processes (oracle/fast.py: predict_marginal_many, pinned against oracle.predict_mvn in tests/test_oracle.py)
            sel = np.flatnonzero(ok)[:24]
            mo, vo, io = F.predict_marginal_many(pkg.encode_batch(ks), nz, ts[:n], xs[:n], tq, sel)
            # (noise_pred differs from noise here: predict_marginal_many adds the training noise; correct for it)
            vo = vo - np.asarray(nz)[sel][:, None] + np.asarray(npred)[sel][:, None]
            for r, i in enumerate(sel):
                if io[r] != 0:
                    continue
                assert np.abs(m1[i] - mo[r]).max() <= LP_TOL * max(1.0, np.abs(mo[r]).max()), (case, i)
                assert np.abs(v1[i] - vo[r]).max() <= LP_TOL * max(1.0, np.abs(vo[r]).max()), (case, i)
        elif n <= 420:
            for i in list(range(1 if case == "refused" else 0, 6)) + [len(ks) - 1]:
                mu, cv = O.predict_mvn(ks[i].to_tuple(), float(nz[i]), ts[:n], xs[:n], tq, noise_pred=float(npred[i]), mean=mean_fn)
                assert np.abs(m1[i] - mu).max() <= LP_TOL * max(1.0, np.abs(mu).max()), (case, i)
                assert np.abs(v1[i] - np.diag(cv)).max() <= LP_TOL * max(1.0, np.abs(cv).max()), (case, i)
        if case == "train_and_future":
            a.set_workspace_limit(5 * n * (n + 1) // 2 * 8 + 1)          # five particles per chunk of the structured pass
            try:
                m3, v3, _, i3 = a.predict_batch(ks, nz, tq, n=n, noise_pred=npred, check=False)
            finally:
                a.set_workspace_limit(0)
            assert np.array_equal(i1, i3) and np.array_equal(m1[ok], m3[ok]) and np.array_equal(v1[ok], v3[ok])
    finally:
        a.close(); b.close()


def test_predictive_lattice_pass_reuses_resident_factors(pkg):
    """The per-step callback of the streaming workload (scripts/online.jl:43,59): factors left by the reweight sweep (rank
    tables) are reused by a predictive pass on lattice query points; same result as a pass that factors itself."""
    n_max, n = 512, 384
    ts, xs = pkg.prior.synthetic_series(n_max, seed=21, shuffle=True)
    nodes, nz = pkg.prior.sample_particles(np.random.default_rng(9), 40, max_depth=3)
    grid = np.sort(ts); h = grid[1] - grid[0]
    tq = np.concatenate([ts[:n + 64], grid[0] + h * np.arange(n_max, n_max + 50)])
    a = pkg.GPEngine(0); b = pkg.GPEngine(0)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        a.logpdf_batch_extend(nodes, nz, n=n, check=False)
        m1, v1, _, i1 = a.predict_batch(nodes, nz, tq, n=n, check=False)
        assert a.predict_reuse_stats()["reused"] > 0 and a.lag_predict_passes() == 1
        m2, v2, _, i2 = b.predict_batch(nodes, nz, tq, n=n, check=False)
        assert b.predict_reuse_stats()["reused"] == 0 and b.lag_predict_passes() == 1
        ok = (i1 == 0) & (i2 == 0)
        assert np.array_equal(i1, i2) and ok.mean() >= 0.9
        sc = np.maximum(1.0, np.abs(m2[ok]).max(axis=1))[:, None]
        assert (np.abs(m1[ok] - m2[ok]) / sc).max() <= 1e-10 and (np.abs(v1[ok] - v2[ok]) / np.maximum(1.0, v2[ok])).max() <= 1e-10
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("case", ["population_2048", "shapes_300", "n4096", "refused", "irregular", "prefix", "prefix_in_time_order", "window_in_time_order"])
def test_structured_value_sweep(pkg, case):
    """Opt-in structured value sweep (agp_set_lag_tables(ctx, 2) / AGP_LAG=2; csrc/agp_toep_kernel.hpp): on a regular grid the
    particles whose kernel is a sum of stationary subtrees and Linear leaves are scored by the Schur algorithm on T + U C U'
    (no factorisation), the others densely in the same call.  Against the dense engine (1e-10 of |logpdf|) and the oracle
    (src/Model.jl:134-136 restated, 1e-8); a matrix that is not positive definite is refused and handed to the dense path, whose
    info (LAPACK's, caller's order) the call returns; irregular series and prefixes take the dense path."""
    G = pkg
    level = 3
    if case == "population_2048":
        n_max = n = 2048; level = 2          # (the class is large enough for the heuristic)
        nodes, nz = pkg.prior.sample_particles(np.random.default_rng(31), 160, max_depth=-1, max_size=31)
        ts, xs = pkg.prior.synthetic_series(n_max, seed=13, shuffle=True)
    elif case == "n4096":
        n_max = n = 4096
        nodes, nz = pkg.prior.sample_particles(np.random.default_rng(32), 24, max_depth=3)
        ts, xs = pkg.prior.synthetic_series(n_max, seed=14, shuffle=False)
    else:
        n_max = n = 300
        covered, elementwise, n_poly = _grad_shapes(G)
        nodes = covered + elementwise; nz = np.linspace(0.02, 0.3, len(nodes))
        ts, xs = pkg.prior.synthetic_series(n_max, seed=15, shuffle=True)
        if case == "refused":
            nodes = [G.SquaredExponential(5.0, 1.0), G.SquaredExponential(0.1, 1.0) + G.Linear(0.2, 0.1, 1.0), G.Linear(0.3, 0.2, 0.5)]
            nz = np.array([0.0, 0.05, 0.1]); n_max = n = 256
            ts, xs = pkg.prior.synthetic_series(n_max, seed=11, shuffle=True)
        elif case == "irregular":
            ts = ts.copy(); ts[7] += 3e-4
        elif case == "prefix":
            n = 250
        elif case == "prefix_in_time_order":         # (scripts/online.jl, fit_smc!(shuffle = false): the first n points ARE consecutive grid points)
            order = np.argsort(ts); ts, xs = ts[order], xs[order]; n = 250
        elif case == "window_in_time_order":         # ... consecutive, but not starting at the series' first point
            order = np.argsort(ts); order = np.concatenate([order[40:], order[:40]]); ts, xs = ts[order], xs[order]; n = 260
    a = G.GPEngine(0); b = G.GPEngine(0)
    try:
        a.set_lag_tables(level)
        a.set_data(ts, xs); b.set_data(ts, xs)
        la, ia = a.logpdf_batch(nodes, nz, n=n, check=False)
        lb, ib = b.logpdf_batch(nodes, nz, n=n, check=False)
        k = a.toeplitz_particles()
        assert b.toeplitz_particles() == 0
        if case in ("irregular", "prefix"):
            assert k == 0
        elif case == "refused":
            assert k == 2 and ia[0] > 0 and np.isnan(la[0])          # (particle 0 went to the dense path)
        elif case in ("shapes_300", "prefix_in_time_order", "window_in_time_order"):
            assert k == len(covered) - n_poly
        else:
            assert k >= len(nodes) // 2
        assert np.array_equal(ia, ib)
        ok = ia == 0
        assert lp_err(la[ok], lb[ok]).max() <= 1e-10
        if True:          # (n = 4096 too: 24 particles x 23 GF on the host's worker processes)
            sel = np.flatnonzero(ok)[:48]
            ref, rinfo = F.gp_logpdf_many(pkg.encode_batch([nodes[i] for i in sel]), np.asarray(nz)[sel], ts[:n], xs[:n])
            both = rinfo == 0
            assert lp_err(la[sel][both], ref[both]).max() <= LP_TOL
        # the same call again: nothing is cached, same bits
        la2, ia2 = a.logpdf_batch(nodes, nz, n=n, check=False)
        assert np.array_equal(la[ok], la2[ok]) and np.array_equal(ia, ia2)
    finally:
        a.close(); b.close()


def test_lag_path_non_positive_definite_info(pkg):
    """A matrix that is not positive definite: the lag sweep flags it, and the info it hands back is LAPACK's for the caller's
    order of the observations (the reference raises PosDefException(info) with that index)."""
    n = 256
    ts, xs = pkg.prior.synthetic_series(n, seed=11, shuffle=True)
    ks, nz = SWEEP_CASES.non_positive_definite_pair(pkg)   # smooth kernel, noise 0: singular to rounding
    la, ia, lb, ib, took, regular = both_paths(pkg, ks, nz, ts, xs)
    assert regular and took >= 1
    assert ia[0] > 0 and ib[0] > 0 and ia[0] == ib[0] and np.isnan(la[0])
    assert ia[1] == 0 and ib[1] == 0 and lp_err(la[1:], lb[1:]).max() <= 1e-10
    _, rinfo = F.gp_logpdf_many(pkg.encode_batch(ks), nz, ts, xs)
    assert rinfo[0] > 0


# ---- gradient sweeps: lag-domain contraction (include/autogp_hip.h agp_set_grad_lag_domain; csrc/agp_grad_kernel.hpp) ----

_grad_shapes = SWEEP_CASES.grad_shapes          # (shared with tools/gpu_sweep_refactor_ab.py)


@pytest.mark.parametrize("n_max,n,fft", [(300, 300, 1), (300, 250, 1), (128, 128, 1), (640, 513, 1), (17, 17, 1), (2, 2, 1),
                                          (300, 300, 0), (300, 250, 0), (129, 129, 0), (17, 17, 0),
                                          (300, 300, 2), (300, 250, 2), (640, 640, 2), (257, 257, 2), (128, 128, 2)])
def test_gradient_lag_domain_vs_elementwise_and_oracle(pkg, monkeypatch, n_max, n, fft):
    """A sum of stationary subtrees and Linear leaves on a (shuffled) regular grid is contracted over n lags instead of n^2
    elements: same gradient as the element-wise contraction (1e-10 of the gradient's scale) and as the oracle (1e-7), on the
    whole series and on a prefix of it; kernels outside the class keep the element-wise contraction in the same batch.  Both
    sources of the lag sums: the power spectrum of Z's columns (fft = 1: series of up to 2048 points) and the histogram of the
    K^-1 tiles (fft = 0: what longer series use)."""
    from oracle import oracle as O
    G = pkg
    covered, elementwise, n_poly = _grad_shapes(G)
    kernels = covered + elementwise
    ts, xs = pkg.prior.synthetic_series(n_max, seed=77 + n_max, shuffle=True)
    noises = np.linspace(0.05, 0.3, len(kernels))
    monkeypatch.setenv("AGP_GRAD_FFT", str(fft))
    eng = pkg.GPEngine(0)
    try:
        eng.set_data(ts, xs)
        assert eng.lag_stats()[0]
        k0 = eng.grad_lag_domain_particles()
        lp, g, gn, info = eng.logpdf_grad_batch(kernels, noises, n=n)
        assert eng.grad_lag_domain_particles() - k0 == len(covered)
        # (fft = 2: consecutive grid points -> the Toeplitz solves; a prefix of the shuffled grid is not such a set)
        assert eng.grad_toeplitz_particles() == (len(covered) - n_poly if fft == 2 and n == n_max and n >= 256 else 0)
        lp_r, g_r, gn_r, _ = eng.logpdf_grad_batch(kernels, noises, n=n)          # reproducible sums
        assert np.array_equal(gn, gn_r) and all(np.array_equal(a, b) for a, b in zip(g, g_r))
        eng.set_grad_lag_domain(False)
        lp2, g2, gn2, info2 = eng.logpdf_grad_batch(kernels, noises, n=n)
        assert eng.grad_lag_domain_particles() - k0 == 2 * len(covered)
        assert (info == 0).all() and (info2 == 0).all() and np.array_equal(lp, lp2)
        for i, k in enumerate(kernels):
            sc = max(1.0, np.abs(g2[i]).max(), abs(gn2[i]))
            assert np.abs(g[i] - g2[i]).max() <= 1e-10 * sc and abs(gn[i] - gn2[i]) <= 1e-10 * sc, (i, k, g[i], g2[i])
            lpo, go, gno = O.gp_logpdf_grad(k.to_tuple(), float(noises[i]), ts[:n], xs[:n])
            sc = max(1.0, np.abs(go).max(), abs(gno))
            assert np.abs(g[i] - go).max() <= 1e-7 * sc and abs(gn[i] - gno) <= 1e-7 * sc, (i, k, g[i], go)
            ref = GC.reference(k.to_tuple(), float(noises[i]), ts[:n], xs[:n])
            GC.assert_grad_components(g[i], gn[i], ref, ctx=(i, k))
            GC.assert_grad_components(g[i], gn[i], ref, against=(g2[i], gn2[i]), particle_wide=False, ctx=(i, k))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["prefix_in_time_order", "resident_factor", "population_2048", "offset_grid"])
def test_gradient_toeplitz_lag_sums(pkg, case):
    """Lag sums of K^-1 from four solves with L (Gohberg-Semencul + the Linear leaves' 2x2 Woodbury term; k_toep_solve) where the
    sweep's points are consecutive grid points: a prefix of a series in time order (data annealing, src/inference_smc_anneal_data.jl:
    206-217), factors read in place from the store (update -> choice_gradients, :63-67), a prior-sampled population at n = 2048,
    a grid away from the origin.  Against the element-wise contraction (1e-9 of the gradient's scale) and, small cases, the oracle."""
    from oracle import oracle as O
    G = pkg
    covered, elementwise, n_poly = _grad_shapes(G)
    # a Linear leaf that dominates its stationary neighbour: the downdate T^-1 = K^-1 + V Q V' is refused on the device and the
    # particle repeated with the explicit inverse
    dominated = SWEEP_CASES.dominated_linear(G)
    kernels = covered + elementwise + [dominated]
    n_refused = 1
    noises = np.linspace(0.02, 0.3, len(kernels))
    oracle_check = True
    if case == "prefix_in_time_order":
        ts, xs = pkg.prior.synthetic_series(600, seed=5, shuffle=False); n = 400
    elif case == "resident_factor":
        ts, xs = pkg.prior.synthetic_series(384, seed=6, shuffle=True); n = 384
    elif case == "offset_grid":
        ts, xs = pkg.prior.synthetic_series(320, seed=7, shuffle=True); ts = ts + 40.0; n = 320
        # (products of Linear leaves are ~1e6 here and the problem itself loses 6 digits: both contractions and the oracle agree to 1e-6
        # only, tools say; the polynomial class is compared on [0, 1], where the reference puts its data, src/api.jl:98-102)
        covered = covered[:len(covered) - n_poly]; n_poly = 0
        kernels = covered + elementwise[:1] + [dominated]; noises = noises[:len(kernels)]
    else:
        ts, xs = pkg.prior.synthetic_series(2048, seed=8, shuffle=True); n = 2048
        kernels, noises = pkg.prior.sample_particles(np.random.default_rng(12), 64, max_depth=-1, max_size=31)
        oracle_check = False; n_refused = None
    a = pkg.GPEngine(0); b = pkg.GPEngine(0)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        b.set_grad_lag_domain(False)
        if case == "resident_factor":
            a.logpdf_batch_extend(kernels, noises, n=n, check=False)
        lp, g, gn, info = a.logpdf_grad_batch(kernels, noises, n=n, check=False)
        if n_refused is None:
            assert 0 < a.grad_toeplitz_particles() <= a.grad_lag_domain_particles()
        else:
            # (away from the origin the cross term -amp (c - t_ref)(t + t') of every Linear leaf is large: more particles are refused)
            refused = a.grad_lag_domain_particles() - n_poly - a.grad_toeplitz_particles()
            assert a.grad_lag_domain_particles() == len(covered) + 1 and (refused == n_refused or (case == "offset_grid" and 1 <= refused <= 4))
        if case == "resident_factor":
            assert a.grad_reuse_stats()["reused"] > 0
        lp2, g2, gn2, info2 = b.logpdf_grad_batch(kernels, noises, n=n, check=False)
        assert np.array_equal(info, info2) and (info == 0).mean() >= 0.9
        refs = GC.references(kernels, noises, ts[:n], xs[:n])
        for i in np.flatnonzero(info == 0):
            sc = max(1.0, np.abs(g2[i]).max(), abs(gn2[i]))
            assert np.abs(g[i] - g2[i]).max() <= 1e-9 * sc and abs(gn[i] - gn2[i]) <= 1e-9 * sc, (case, i, kernels[i], g[i], g2[i])
            GC.assert_grad_components(g[i], gn[i], refs[i], against=(g2[i], gn2[i]), particle_wide=False, ctx=(case, i, kernels[i]))
            # (every case against the oracle per component, population_2048 included; the particle-wide check where it was)
            GC.assert_grad_components(g[i], gn[i], refs[i], particle_wide=oracle_check, ctx=(case, i, kernels[i]))
            if oracle_check:
                lpo, go, gno = O.gp_logpdf_grad(kernels[i].to_tuple(), float(noises[i]), ts[:n], xs[:n])
                sc = max(1.0, np.abs(go).max(), abs(gno))
                assert np.abs(g[i] - go).max() <= 1e-7 * sc and abs(gn[i] - gno) <= 1e-7 * sc, (case, i, kernels[i], g[i], go)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("case", ["shapes_full", "shapes_prefix_in_time_order", "population_2048", "refused", "store_present"])
def test_gradient_structured_sweep(pkg, monkeypatch, case):
    """Gradient sweeps of the Toeplitz class WITHOUT a dense factor (AGP_GRAD_FFT >= 3: Schur recursion on T with the columns of L
    stored, backward substitution, K^-1 = T^-1 - W S W' in the update direction; csrc/agp_toep_kernel.hpp, toeplitz_grad_sweep):
    value, gradient and noise gradient against the element-wise contraction of a dense sweep (1e-9 of the gradient's scale, 1e-10 of
    |logpdf|) and the oracle; a matrix that is not positive definite goes to the dense path; nothing changes while factors can be
    resident (HMC's update -> choice_gradients pairs, src/inference_smc_anneal_data.jl:63-67, keep reading them)."""
    from oracle import oracle as O
    G = pkg
    covered, elementwise, n_poly = _grad_shapes(G)
    n_cls = len(covered) - n_poly
    kernels = covered + elementwise
    noises = np.linspace(0.02, 0.3, len(kernels))
    oracle_check = True
    force = "4"
    if case == "shapes_prefix_in_time_order":
        ts, xs = pkg.prior.synthetic_series(600, seed=5, shuffle=False); n = 400
    elif case == "population_2048":
        ts, xs = pkg.prior.synthetic_series(2048, seed=8, shuffle=True); n = 2048
        kernels, noises = pkg.prior.sample_particles(np.random.default_rng(12), 320, max_depth=-1, max_size=31)
        oracle_check = False; force = "3"; n_cls = None          # (the default: the class is large enough to pay)
    elif case == "refused":
        ts, xs = pkg.prior.synthetic_series(256, seed=11, shuffle=True); n = 256
        kernels = [G.SquaredExponential(5.0, 1.0), G.SquaredExponential(0.1, 1.0) + G.Linear(0.2, 0.1, 1.0), G.Linear(0.3, 0.2, 0.5)]
        noises = np.array([0.0, 0.05, 0.1]); n_cls = 3
    else:
        ts, xs = pkg.prior.synthetic_series(384, seed=6, shuffle=True); n = 384
    monkeypatch.setenv("AGP_GRAD_FFT", force)
    a = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_FFT")
    b = pkg.GPEngine(0)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        b.set_grad_lag_domain(False)
        if case == "store_present":
            a.logpdf_batch_extend(kernels[:2], noises[:2], n=n, check=False)
        lp, g, gn, info = a.logpdf_grad_batch(kernels, noises, n=n, check=False)
        k = a.grad_structured_particles()
        if case == "store_present":
            assert k == 0
        elif case == "refused":
            assert k == 2 and info[0] > 0
        elif n_cls is None:
            assert k >= len(kernels) // 2
        else:
            assert k == n_cls and a.grad_lag_domain_particles() == len(covered)
        lp2, g2, gn2, info2 = b.logpdf_grad_batch(kernels, noises, n=n, check=False)
        assert np.array_equal(info, info2)
        ok = info == 0
        assert lp_err(lp[ok], lp2[ok]).max() <= 1e-10
        refs = GC.references(kernels, noises, ts[:n], xs[:n])
        for i in np.flatnonzero(ok):
            GC.assert_grad_components(g[i], gn[i], refs[i], particle_wide=False, ctx=(case, i, kernels[i]))
            GC.assert_grad_components(g[i], gn[i], refs[i], against=(g2[i], gn2[i]), particle_wide=False, ctx=(case, i, kernels[i]))
            sc = max(1.0, np.abs(g2[i]).max(), abs(gn2[i]))
            # (prior-sampled kernels at n = 2048 include periods / length scales of a few grid spacings: both contractions carry ~1e-8
            # there — tools/gpu_grad_toeplitz_check.py prints the population's worst case for every variant)
            tol = 1e-8 if case == "population_2048" else 1e-9
            assert np.abs(g[i] - g2[i]).max() <= tol * sc and abs(gn[i] - gn2[i]) <= tol * sc, (case, i, kernels[i], g[i], g2[i])
            if oracle_check:
                lpo, go, gno = O.gp_logpdf_grad(kernels[i].to_tuple(), float(noises[i]), ts[:n], xs[:n])
                sc = max(1.0, np.abs(go).max(), abs(gno))
                assert np.abs(g[i] - go).max() <= 1e-7 * sc and abs(gn[i] - gno) <= 1e-7 * sc and abs(lp[i] - lpo) <= LP_TOL * max(1.0, abs(lpo))
        lp_r, g_r, gn_r, _ = a.logpdf_grad_batch(kernels, noises, n=n, check=False)          # reproducible
        assert np.array_equal(gn[ok], gn_r[ok]) and all(np.array_equal(g[i], g_r[i]) for i in np.flatnonzero(ok))
        if case == "shapes_full":
            # a small workspace: the structured sweep runs its particles a few at a time, same bits
            a.set_workspace_limit(3 * n * (n + 1) // 2 * 8 + 1)
            try:
                lp_c, g_c, gn_c, _ = a.logpdf_grad_batch(kernels, noises, n=n, check=False)
            finally:
                a.set_workspace_limit(0)
            assert np.array_equal(lp[ok], lp_c[ok]) and np.array_equal(gn[ok], gn_c[ok]) and all(np.array_equal(g[i], g_c[i]) for i in np.flatnonzero(ok))
    finally:
        a.close(); b.close()


def test_gradient_lag_domain_population_and_switches(pkg, monkeypatch):
    """Prior-sampled population at n=1024 (several launch classes of the element-wise contraction beside the lag-domain particles,
    chunked workspace), the environment switch, and an irregular series (nothing contracted in the lag domain)."""
    ts, xs = pkg.prior.synthetic_series(1024, seed=4, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(8), 96, max_depth=-1, max_size=31)
    a = pkg.GPEngine(0)
    monkeypatch.setenv("AGP_GRAD_LAGDOM", "0")
    b = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_LAGDOM")
    monkeypatch.setenv("AGP_GRAD_FFT", "0")
    h = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_FFT")
    try:
        a.set_data(ts, xs); b.set_data(ts, xs); h.set_data(ts, xs)
        lp, g, gn, info = a.logpdf_grad_batch(nodes, noises, check=False)
        lp2, g2, gn2, info2 = b.logpdf_grad_batch(nodes, noises, check=False)
        lp3, g3, gn3, info3 = h.logpdf_grad_batch(nodes, noises, check=False)
        assert a.grad_lag_domain_particles() >= 40 and b.grad_lag_domain_particles() == 0 and h.grad_lag_domain_particles() >= 40
        assert np.array_equal(info, info2) and np.array_equal(info, info3)
        refs = GC.references(nodes, noises, ts, xs)
        for i in np.flatnonzero(info == 0):
            GC.assert_grad_components(g[i], gn[i], refs[i], particle_wide=False, ctx=(i, nodes[i]))
            GC.assert_grad_components(g[i], gn[i], refs[i], against=(g2[i], gn2[i]), particle_wide=False, ctx=(i, nodes[i]))
            GC.assert_grad_components(g3[i], gn3[i], refs[i], against=(g2[i], gn2[i]), particle_wide=False, ctx=(i, nodes[i]))
            sc = max(1.0, np.abs(g2[i]).max(), abs(gn2[i]))
            assert np.abs(g[i] - g2[i]).max() <= 1e-9 * sc and abs(gn[i] - gn2[i]) <= 1e-9 * sc, (i, nodes[i])
            assert np.abs(g3[i] - g2[i]).max() <= 1e-9 * sc and abs(gn3[i] - gn2[i]) <= 1e-9 * sc, (i, nodes[i])
        a.set_workspace_limit(8 * 2 * 36 * 128 * 128 * 8)          # eight particles per chunk
        try:
            lp3, g3, gn3, _ = a.logpdf_grad_batch(nodes, noises, check=False)
        finally:
            a.set_workspace_limit(0)
        ok = info == 0
        assert np.array_equal(gn[ok], gn3[ok]) and all(np.array_equal(g[i], g3[i]) for i in np.flatnonzero(ok))
        tj = ts.copy(); tj[5] += 3e-4
        a.set_data(tj, xs)
        k0 = a.grad_lag_domain_particles()
        a.logpdf_grad_batch(nodes[:8], noises[:8], check=False)
        assert a.grad_lag_domain_particles() == k0 and not a.lag_stats()[0]
    finally:
        a.close(); b.close(); h.close()


@pytest.mark.parametrize("n_max", [2300, 3000, 4096])
def test_gradient_polynomial_class_above_2048_points(pkg, n_max):
    """Polynomial lag-domain class on long series: a particle of degree d keeps 2d+1 moment histograms of n_max lags in LDS and is
    admitted while they fit one tile (csrc/agp_engine.hip, (2d+1) n_max + 8 <= 128 x 128) — degree 3 up to 2339 points, degree 2 up
    to 3275, degree 1 up to 5458.  k_lag_grad's launch is sized by the largest ADMITTED degree (sized for degree 3 whatever the
    class held, it failed from 2926 points on; found by tools/gpu_fuzz_structured.py).  Against the element-wise contraction."""
    G = pkg
    ts, xs = pkg.prior.synthetic_series(n_max, seed=4, shuffle=True)
    se, per, lin = G.SquaredExponential(0.2, 0.8), G.Periodic(0.3, 0.25, 0.7), G.Linear(0.3, 0.2, 0.9)
    lin2, lin3 = G.Linear(0.6, 0.1, 0.5), G.Linear(-0.2, 0.3, 0.4)
    kernels = [lin * se, lin * per + se, lin * lin2 * se, lin * lin2 * lin3 * per, se + lin]
    noises = np.array([0.05, 0.1, 0.08, 0.12, 0.07])
    n_adm = sum((2 * d + 1) * n_max + 8 <= 128 * 128 for d in (1, 1, 2, 3))
    a = pkg.GPEngine(0); b = pkg.GPEngine(0)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        b.set_grad_lag_domain(False)
        lp, g, gn, info = a.logpdf_grad_batch(kernels, noises, check=False)
        assert a.grad_lag_domain_particles() == n_adm + 1
        lp2, g2, gn2, info2 = b.logpdf_grad_batch(kernels, noises, check=False)
        assert np.array_equal(info, info2) and (info == 0).all()
        assert lp_err(lp, lp2).max() <= 1e-10
        refs = GC.references(kernels, noises, ts, xs)
        for i in range(len(kernels)):
            sc = max(1.0, np.abs(g2[i]).max(), abs(gn2[i]))
            assert np.abs(g[i] - g2[i]).max() <= 1e-7 * sc and abs(gn[i] - gn2[i]) <= 1e-7 * sc, (n_max, i)
            GC.assert_grad_components(g[i], gn[i], refs[i], against=(g2[i], gn2[i]), particle_wide=False, ctx=(n_max, i))
    finally:
        a.close(); b.close()


def test_class_aware_leapfrog_pairs(pkg, monkeypatch):
    """Opt-in level AGP_LAG = 2 on the coalesced single-particle entries (Gen.hmc's update -> choice_gradients pairs,
    src/inference_smc_anneal_data.jl:63-67): value calls score the Toeplitz class by the Schur recursion and keep it OUT of the factor
    store, the others go through the store; the gradient calls that follow differentiate the class by the structured sweep and the
    others from their resident factors — no particle is factored twice, none of the class densely.  Results against the default
    engine (value 1e-10 of |logpdf|, gradient 1e-7 of its scale) and the oracle."""
    import threading
    from oracle import oracle as O
    n, T = 512, 160
    ts, xs = pkg.prior.synthetic_series(n, seed=77, shuffle=True)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(12), T, max_depth=3, max_size=15)
    cls = np.array([pkg.shard_plan(pkg.encode_batch([nd]), [z], n, 1, sweep=1, regular_grid=True)[1][0] < 3.0 for nd, z in zip(nodes, noises)])
    assert 0.5 * T <= cls.sum() < T
    ref = pkg.GPEngine(0)
    monkeypatch.setenv("AGP_GRAD_FFT", "4")      # structured gradient sweeps whatever the class's size ...
    eng = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_FFT")
    try:
        ref.set_data(ts, xs)
        r_lp, r_g, r_gn, r_info = ref.logpdf_grad_batch(nodes, noises, check=False)
        refs = GC.references(nodes, noises, ts, xs)
        eng.set_lag_tables(3)                    # ... and level 3 = level 2 whatever it is: the size heuristics are not under test
        eng.set_data(ts, xs)
        eng.extend_reserve(n, 2 * T)             # (Python threads arrive slowly: many small coalesced batches, the store must hold the population)

        def phase(fn):
            out = [None] * T
            def work(i):
                out[i] = fn(nodes[i], float(noises[i]), check=False)
            th = [threading.Thread(target=work, args=(i,)) for i in range(T)]
            for t in th: t.start()
            for t in th: t.join()
            return out
        for rep in range(2):                     # two leapfrog steps (the second at the same parameters: value calls hit the store / recompute the class)
            k_t0, k_s0, g0 = eng.toeplitz_particles(), eng.grad_structured_particles(), eng.grad_reuse_stats()
            vals = phase(eng.logpdf)
            k_t1 = eng.toeplitz_particles()
            grads = phase(eng.logpdf_grad)
            k_s1, g1 = eng.grad_structured_particles(), eng.grad_reuse_stats()
            ok = r_info == 0
            n_cls_ok = int((cls & ok).sum())
            # every accepted class particle: value from the recursion, gradient from the structured sweep
            assert k_t1 - k_t0 >= n_cls_ok - 2, (k_t1 - k_t0, n_cls_ok)
            assert k_s1 - k_s0 >= n_cls_ok - 2, (k_s1 - k_s0, n_cls_ok)
            # the others: gradient from the resident factor of the value call, nothing factored by a gradient sweep
            assert g1["reused"] - g0["reused"] >= int((~cls & ok).sum()) and g1["factored"] - g0["factored"] <= 2, (g0, g1)
            for i in range(T):
                if not ok[i]:
                    continue
                lp, g, gn = grads[i]
                sc = max(1.0, np.abs(r_g[i]).max() if len(r_g[i]) else 0.0, abs(r_gn[i]))
                assert abs(vals[i] - r_lp[i]) <= 1e-10 * max(1.0, abs(r_lp[i])), i
                assert abs(lp - r_lp[i]) <= 1e-10 * max(1.0, abs(r_lp[i])), i
                assert (np.abs(g - r_g[i]).max() if len(g) else 0.0) <= 1e-7 * sc and abs(gn - r_gn[i]) <= 1e-7 * sc, i
                GC.assert_grad_components(g, gn, refs[i], against=(r_g[i], r_gn[i]), particle_wide=False, ctx=i)
        for i in range(0, T, 23):
            if r_info[i] != 0:
                continue
            lpo, go, gno = O.gp_logpdf_grad(nodes[i].to_tuple(), float(noises[i]), ts, xs)
            sc = max(1.0, np.abs(go).max() if len(go) else 0.0, abs(gno))
            assert abs(grads[i][0] - lpo) <= LP_TOL * max(1.0, abs(lpo))
            assert (np.abs(grads[i][1] - go).max() if len(go) else 0.0) <= 1e-7 * sc and abs(grads[i][2] - gno) <= 1e-7 * sc
            GC.assert_grad_components(grads[i][1], grads[i][2], refs[i], ctx=i)
        # The annealing prefixes fit_smc! runs its HMC moves on (src/inference_smc_anneal_data.jl:240-252): a series handed over in TIME
        # ORDER, a prefix of it — n consecutive grid points, so the class stays structured — and no agp_extend_reserve (the store sizes
        # itself by the callers).  Same counters: the class is never factored densely, nobody is factored twice.
        ts2, xs2 = pkg.prior.synthetic_series(n, seed=78, shuffle=False)
        n_pre = 384
        ref.set_data(ts2, xs2); eng.extend_reset(release_memory=True); eng.set_data(ts2, xs2)
        p_lp, p_g, p_gn, p_info = ref.logpdf_grad_batch(nodes, noises, n=n_pre, check=False)
        p_refs = GC.references(nodes, noises, ts2[:n_pre], xs2[:n_pre])
        k_t0, k_s0, g0 = eng.toeplitz_particles(), eng.grad_structured_particles(), eng.grad_reuse_stats()
        vals = phase(lambda nd, z, check: eng.logpdf(nd, z, n=n_pre, check=check))
        k_t1 = eng.toeplitz_particles()
        grads = phase(lambda nd, z, check: eng.logpdf_grad(nd, z, n=n_pre, check=check))
        k_s1, g1 = eng.grad_structured_particles(), eng.grad_reuse_stats()
        ok = p_info == 0
        n_cls_ok = int((cls & ok).sum())
        assert k_t1 - k_t0 >= n_cls_ok - 2 and k_s1 - k_s0 >= n_cls_ok - 2, (k_t1 - k_t0, k_s1 - k_s0, n_cls_ok)
        st = eng.extend_stats()
        assert g1["reused"] - g0["reused"] >= int((~cls & ok).sum()) and g1["factored"] - g0["factored"] <= 2, (g0, g1, st, eng.coalesce_stats())
        assert st["evicted_before_reuse"] == 0 and st["slots"] >= int((~cls).sum()), st      # (no reservation: the store grew by what was waiting in it)
        for i in range(T):
            if not ok[i]:
                continue
            lp, g, gn = grads[i]
            sc = max(1.0, np.abs(p_g[i]).max() if len(p_g[i]) else 0.0, abs(p_gn[i]))
            assert abs(vals[i] - p_lp[i]) <= 1e-10 * max(1.0, abs(p_lp[i])) and abs(lp - p_lp[i]) <= 1e-10 * max(1.0, abs(p_lp[i])), i
            assert (np.abs(g - p_g[i]).max() if len(g) else 0.0) <= 1e-7 * sc and abs(gn - p_gn[i]) <= 1e-7 * sc, i
            GC.assert_grad_components(g, gn, p_refs[i], against=(p_g[i], p_gn[i]), particle_wide=False, ctx=i)
    finally:
        ref.close(); eng.close()
