"""Every gradient path of the engine checked COMPONENT BY COMPONENT against the fp64 oracle (oracle/gradcheck.py):
|g_k - ref_k| <= 1e-7 S_k, S_k = 1/2 sum_ab (|alpha_a alpha_b| + |K^-1_ab|) |dK_ab/dtheta_k| — the error scale of component k
itself, not of the particle's largest component — at the places where small components live: summands of amplitude 1e-3 .. 1e-6
of their neighbour's, GammaExponential exponents near 0.05 and 2, periods below the grid spacing and at hundreds of periods per
lag, Linear leaves inside products of degree 1 .. 4 and with their location outside [0, 1], ChangePoints at the prior's scale of
0.001 between two grid points and on one, WhiteNoise on duplicated times, noise from the model's jitter (1e-5) up to 1.

Paths (each case asserts through the engine's counters that it ran): the element-wise contraction on irregular times; the lag
domain on a shuffled regular grid with its lag sums from K^-1 tile histograms (AGP_GRAD_FFT=0), Z's power spectrum (=1, series
above 1024 points), the Gohberg-Semencul solves (=2, n >= 256 consecutive points) and the structured Schur sweep without a dense
factor (=4), each on the whole grid and on a prefix in time order; rank tables (business days) and compact tables (month starts)
on calendar lattices; gradients read from a resident factor; the coalesced single-particle entry from several threads; the
multi-context entry over two contexts of one device.  Shapes n = 2 .. 2049 (2049: past the spectral and structured paths'
2048-point bound), and prior populations of 64 particles at n = 2048.  Each path is also compared with the element-wise
contraction (lag domain off) at 1e-9 S_k.  Each test prints its worst |g_k - ref_k| / S_k (run with -s to see them).

Only the per-component bound is asserted here.  The particle-wide one does not hold for a period below the grid spacing: the
derivative by the period multiplies the rounding of its argument (pi / p) |t - t'| by |t - t'| / p^2, so one unit of rounding in
how t - t' is formed (a lag-domain path forms it as k h) moves the gradient by ~1e-6 .. 1e-4 of the particle's largest component
at n = 1000 .. 2048, while each component stays within 1e-7 of its own S_k.  (The oracle's derivative of the Periodic kernel first
formed its argument as pi |t - t'| / p, not as the reference's (pi / p) |t - t'|, and disagreed with the device there by 1e-5 of the
particle's scale on the element-wise path as well; eval_cov_grad now rounds the argument as the reference does.)"""
import threading

import numpy as np
import pytest

from oracle import gradcheck as GC

pytestmark = pytest.mark.gpu

SHAPES = [2, 17, 127, 128, 129, 255, 256, 257, 1000, 2048, 2049]
_REFS = {}


def references(key, trees, noises, ts, xs):
    """GradRef of every particle (cached by key: the FFT variants of one series share them); the oracle runs in threads (its
    large array operations release the GIL)."""
    if key not in _REFS:
        _REFS[key] = GC.references(trees, noises, ts, xs)
    return _REFS[key]


def report(name, worst):
    print(f"[grad-components] {name}: worst |g_k - ref_k| / S_k = {worst:.3e}")


def check_all(name, res, refs, against=None, tau=None):
    """Per-component check of every particle with info == 0; all failures reported together."""
    lp, g, gn, info = res
    fails, worst = [], 0.0
    for i, r in enumerate(refs):
        if info[i] != 0:
            continue
        try:
            ag = None if against is None else (against[1][i], against[2][i])
            worst = max(worst, GC.assert_grad_components(g[i], gn[i], r, tau=tau, against=ag, ctx=(name, i, r.tree, r.noise),
                                                         particle_wide=False))
        except AssertionError as e:
            fails.append(str(e))
    report(name, worst)
    assert not fails, "\n".join(fails)
    return worst


def small_kernels(G, ts, duplicates=False):
    """Kernels with small gradient components; the ChangePoint locations are placed on the series' own points."""
    u = np.unique(ts)
    h = (u[-1] - u[0]) / max(1, len(u) - 1) if len(u) > 1 else 1.0
    k = len(u) // 2
    mid = 0.5 * (u[max(k - 1, 0)] + u[k]) if len(u) > 1 else u[0] + 0.5
    lin, lin2, lin3 = G.Linear(0.3, 0.2, 0.7), G.Linear(0.6, 0.1, 0.5), G.Linear(0.1, 0.3, 0.4)
    out = [G.GammaExponential(0.2, 0.05, 0.9),                                           # gamma near 0.05 (noise 1e-5 goes here)
           G.SquaredExponential(0.3, 1.0) + G.SquaredExponential(0.05, 1e-3),            # a summand 1e-3 of its neighbour
           G.Periodic(0.8, 0.25, 1.0) + G.GammaExponential(0.1, 1.0, 1e-6),              # ... 1e-6
           G.GammaExponential(0.15, 1.97, 0.8) + G.SquaredExponential(0.4, 0.3),         # gamma near 2
           G.Periodic(1.2, 0.37 * h, 0.7) + G.SquaredExponential(0.2, 0.5),              # period below the grid spacing
           G.Periodic(0.9, 0.004, 0.6) + G.Constant(0.2),                                # |dt| / p up to 250
           lin * G.SquaredExponential(0.1, 1e-3) + G.SquaredExponential(0.3, 1.0),       # Linear in a product, degree 1 .. 3
           lin * lin2 * G.Periodic(0.7, 0.2, 0.5) + G.SquaredExponential(0.2, 0.4),
           lin * lin2 * lin3 * G.SquaredExponential(0.25, 0.8),
           G.Linear(1.7, 0.1, 0.5) * G.SquaredExponential(0.3, 1.0) + G.Linear(-0.6, 0.05, 0.2),     # locations outside [0, 1]
           G.Constant(0.4) + G.WhiteNoise(0.05),
           # (element-wise whatever the series: ChangePoints, degree 4)
           G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Periodic(0.5, 0.1, 0.8), float(mid), 0.001),   # between two points
           G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Linear(0.3, 0.2, 0.7), float(u[len(u) // 3]), 0.001),   # on a point
           lin * lin2 * lin3 * G.Linear(0.8, 0.2, 0.3) * G.SquaredExponential(0.3, 1.0)]
    if duplicates:
        out.append(G.WhiteNoise(0.05) + G.SquaredExponential(0.1, 0.5))                # WhiteNoise on duplicated times
    noises = np.geomspace(1e-5, 1.0, len(out))
    return out, noises


N_ELEMENTWISE_ONLY = 3       # the last three of small_kernels (four with duplicates) are never in the lag-domain class


def irregular_series(n, seed):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.random(n))
    if n > 3:
        ts[n // 2] = ts[n // 2 - 1]          # a duplicated time
    xs = 0.5 * rng.standard_normal(n) + np.sin(6 * ts)
    return ts, xs


def counters(e):
    return np.array([e.grad_lag_domain_particles(), e.grad_toeplitz_particles(), e.grad_structured_particles()])


@pytest.mark.parametrize("n", SHAPES)
def test_elementwise_irregular_times(pkg, n):
    """Irregular times with a duplicated point: nothing is contracted in the lag domain."""
    ts, xs = irregular_series(n, seed=1000 + n)
    kernels, noises = small_kernels(pkg, ts, duplicates=True)
    refs = references(("irregular", n), [k.to_tuple() for k in kernels], noises, ts, xs)
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        c0 = counters(e)
        res = e.logpdf_grad_batch(kernels, noises, check=False)
        assert n <= 2 or ((counters(e) == c0).all() and not e.lag_stats()[0])      # (two points are a regular grid)
        assert (res[3] == 0).sum() >= len(kernels) - 1
        check_all(f"elementwise n={n}", res, refs)
    finally:
        e.close()


def tau_vs_elementwise(fft, n):
    """TAU_PATHS, except the structured sweep above 1024 points: its Schur recursion and the downdate K^-1 = T^-1 - W S W' differ
    from the dense factor's K^-1 by up to 2.3e-9 S_k measured (the noise derivative of a particle with noise 6e-5 at n = 2048), as
    test_gpu_lag.py::test_gradient_structured_sweep[population_2048] allows 1e-8 of the particle's scale there.  Against the oracle
    the structured sweep meets 1e-7 S_k like every path."""
    return 1e-8 if fft == 4 and n > 1024 else GC.TAU_PATHS


def _grid_engines(pkg, monkeypatch, fft):
    monkeypatch.setenv("AGP_GRAD_FFT", str(fft))
    a = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_FFT")
    b = pkg.GPEngine(0)
    b.set_grad_lag_domain(False)
    return a, b


@pytest.mark.parametrize("fft", [1, 0, 2, 4])
@pytest.mark.parametrize("n", SHAPES)
def test_lag_domain_shuffled_grid(pkg, monkeypatch, n, fft):
    """Whole shuffled regular grid.  Which source of the lag sums runs: histograms (fft = 0, and fft = 1 up to 1024 points), the
    power spectrum (fft = 1 above 1024 points), the Toeplitz solves (fft = 2, n >= 256), the structured sweep (fft = 4,
    256 <= n <= 2048); at 2049 neither the spectrum, the solves nor the structured sweep may run."""
    ts, xs = pkg.prior.synthetic_series(n, seed=2000 + n, shuffle=True)
    kernels, noises = small_kernels(pkg, ts)
    refs = references(("grid", n), [k.to_tuple() for k in kernels], noises, ts, xs)
    a, b = _grid_engines(pkg, monkeypatch, fft)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        assert a.lag_stats()[0] or n <= 2
        c0 = counters(a)
        res = a.logpdf_grad_batch(kernels, noises, check=False)
        d = counters(a) - c0
        if n > 2:
            assert d[0] == len(kernels) - N_ELEMENTWISE_ONLY, d
            assert (d[2] > 0) == (fft == 4 and 256 <= n <= 2048), d            # structured sweep: no dense factor
            if fft != 4:
                assert (d[1] > 0) == (fft == 2 and 256 <= n <= 2048), d        # Gohberg-Semencul solves on the dense factor
        ref2 = b.logpdf_grad_batch(kernels, noises, check=False)
        assert np.array_equal(res[3], ref2[3])
        check_all(f"grid fft={fft} n={n}", res, refs)
        check_all(f"grid fft={fft} n={n} vs element-wise", res, refs, against=ref2, tau=tau_vs_elementwise(fft, n))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("fft", [1, 0, 2, 4])
@pytest.mark.parametrize("n", [17, 129, 256, 1000, 2047])
def test_lag_domain_prefix_in_time_order(pkg, monkeypatch, n, fft):
    """A prefix of a series in time order (data annealing): n consecutive grid points of a longer grid."""
    ts, xs = pkg.prior.synthetic_series(2048, seed=3000, shuffle=False)        # (2 n_max <= 4096: every source of the lag sums open)
    kernels, noises = small_kernels(pkg, ts[:n])
    refs = references(("prefix", n), [k.to_tuple() for k in kernels], noises, ts[:n], xs[:n])
    a, b = _grid_engines(pkg, monkeypatch, fft)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        c0 = counters(a)
        res = a.logpdf_grad_batch(kernels, noises, n=n, check=False)
        d = counters(a) - c0
        assert d[0] == len(kernels) - N_ELEMENTWISE_ONLY, d
        assert (d[2] > 0) == (fft == 4 and n >= 256), d
        if fft != 4:
            assert (d[1] > 0) == (fft == 2 and n >= 256), d
        ref2 = b.logpdf_grad_batch(kernels, noises, n=n, check=False)
        check_all(f"prefix fft={fft} n={n}", res, refs)
        check_all(f"prefix fft={fft} n={n} vs element-wise", res, refs, against=ref2, tau=tau_vs_elementwise(fft, n))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("freq,n", [("B", 520), ("M", 520)])
def test_calendar_lattices(pkg, freq, n):
    """Business days: rank tables and the lag-domain contraction over the lattice's lags; month starts (15 796 days): compact
    tables, element-wise contraction."""
    ts, xs = pkg.prior.calendar_series(n, freq, seed=11, shuffle=True)
    kernels, noises = small_kernels(pkg, ts)
    refs = references(("calendar", freq, n), [k.to_tuple() for k in kernels], noises, ts, xs)
    a = pkg.GPEngine(0); b = pkg.GPEngine(0)
    try:
        a.set_data(ts, xs); b.set_data(ts, xs)
        b.set_grad_lag_domain(False)
        kind = a.lattice_stats()["kind"]
        assert kind == (3 if freq == "M" else 2)
        c0, s0 = counters(a), a.compact_stats()["sweeps"]
        res = a.logpdf_grad_batch(kernels, noises, check=False)
        d = counters(a) - c0
        assert d[1] == 0 and d[2] == 0
        if kind == 2:
            assert d[0] == len(kernels) - N_ELEMENTWISE_ONLY, d
        else:
            assert d[0] == 0 and a.compact_stats()["sweeps"] == s0 + 1
        check_all(f"calendar {freq} n={n}", res, refs)
        check_all(f"calendar {freq} n={n} vs element-wise", res, refs, against=b.logpdf_grad_batch(kernels, noises, check=False))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("grid", [False, True])
def test_resident_factor(pkg, grid):
    """Gradients read from the factor store (logpdf_batch_extend first, as Gen.hmc's update -> choice_gradients)."""
    n = 384
    if grid:
        ts, xs = pkg.prior.synthetic_series(n, seed=4000, shuffle=True)
    else:
        ts, xs = irregular_series(n, seed=4001)
    kernels, noises = small_kernels(pkg, ts, duplicates=not grid)
    refs = references(("resident", grid), [k.to_tuple() for k in kernels], noises, ts, xs)
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        e.logpdf_batch_extend(kernels, noises, check=False)
        r0 = e.grad_reuse_stats()["reused"]
        res = e.logpdf_grad_batch(kernels, noises, check=False)
        assert e.grad_reuse_stats()["reused"] > r0
        check_all(f"resident factor grid={grid}", res, refs)
    finally:
        e.close()


@pytest.mark.parametrize("grid", [False, True])
def test_coalesced_threads(pkg, grid):
    """agp_logpdf_grad one particle per thread, coalesced by the library into batches."""
    n = 300
    if grid:
        ts, xs = pkg.prior.synthetic_series(n, seed=5000, shuffle=True)
    else:
        ts, xs = irregular_series(n, seed=5001)
    kernels, noises = small_kernels(pkg, ts, duplicates=not grid)
    refs = references(("threads", grid), [k.to_tuple() for k in kernels], noises, ts, xs)
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        out = [None] * len(kernels)
        barrier = threading.Barrier(len(kernels))

        def work(i):
            barrier.wait()
            out[i] = e.logpdf_grad(kernels[i], float(noises[i]), check=False)
        c0, _ = e.coalesce_stats()
        th = [threading.Thread(target=work, args=(i,)) for i in range(len(kernels))]
        for t in th: t.start()
        for t in th: t.join()
        assert e.coalesce_stats()[0] - c0 == len(kernels)
        lp = np.array([o[0] for o in out])
        res = (lp, [o[1] for o in out], np.array([o[2] for o in out]), np.where(np.isfinite(lp), 0, 1))
        assert (res[3] == 0).all()
        check_all(f"coalesced threads grid={grid}", res, refs)
    finally:
        e.close()


def test_multi_context(pkg):
    """agp_logpdf_grad_batch_multi over two contexts of one device; every particle of both contexts' shares checked."""
    n = 512
    ts, xs = pkg.prior.synthetic_series(n, seed=6000, shuffle=True)
    kernels, noises = small_kernels(pkg, ts)
    kernels = kernels * 3
    noises = np.concatenate([noises, noises[::-1], np.full(len(noises), 0.1)])
    refs = references(("multi",), [k.to_tuple() for k in kernels], noises, ts, xs)
    engines = [pkg.GPEngine(0), pkg.GPEngine(0)]
    try:
        for e in engines:
            e.set_data(ts, xs)
        lp, g, gn, info, owner = pkg.logpdf_grad_batch_multi(engines, kernels, noises, check=False, want_owner=True)
        assert set(np.unique(owner)) == {0, 1}, owner
        check_all("multi-context", (lp, g, gn, info), refs)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("grid", [False, True])
def test_prior_population_2048(pkg, grid):
    """64 prior particles at n = 2048 on irregular times (element-wise) and on the shuffled grid (the default engine's mix of the
    Toeplitz solves, the structured sweep and the element-wise contraction), every component against the oracle."""
    n = 2048
    if grid:
        ts, xs = pkg.prior.synthetic_series(n, seed=8, shuffle=True)
    else:
        ts, xs = irregular_series(n, seed=7000)
    nodes, noises = pkg.prior.sample_particles(np.random.default_rng(12), 64, max_depth=-1, max_size=31)
    refs = references(("population", grid), [k.to_tuple() for k in nodes], noises, ts, xs)
    e = pkg.GPEngine(0)
    try:
        e.set_data(ts, xs)
        c0 = counters(e)
        res = e.logpdf_grad_batch(nodes, noises, check=False)
        d = counters(e) - c0
        if grid:
            assert d[1] + d[2] > 0, d
        else:
            assert (d == 0).all(), d
        assert (res[3] == 0).mean() >= 0.9
        check_all(f"population n=2048 grid={grid}", res, refs)
    finally:
        e.close()
