"""Every predictive route of the engine checked OUTPUT BY OUTPUT against an 80-bit reference on the output's own error scale
(oracle/predcheck.py):

    |mean_j - m80_j| <= mult R_mean sigma_j + 4 eps S_mean_j,      |var_j - v80_j| <= mult R_var v80_j + 4 eps S_var_j,
    |cov_ij - c80_ij| <= mult R_cov sigma_i sigma_j + 4 eps S_cov_ij,      mult = 8 or the route's own multiple (below),

R the distance of three correct double-precision routes from the 80-bit values — at the places where small outputs live: noise at
the model's jitter (1e-5), a kernel of amplitude 1e-4, noise_pred = 0, queries ON training times (variance 1e-8 .. 1e-5), between
them and after the series.  The particle-wide criterion |d| <= 1e-8 max(1, max|ref|), which the helper asserts as well, lets an
error of 1 % .. 10 % of such a variance pass.

Routes (each case asserts through the engine's counters that it ran): the joint dense pass on irregular times with a duplicated
time (n = 17, 129, 300, marginals and full covariance, mean functions, noise_pred != 0); the training-point shortcut through
diag(K^-1) at its threshold and one query below it; the lattice pass on rank tables (shuffled regular grid, business-day
calendar); the structured pass without a dense factor and its dense twin; resident factors at n_max and at a prefix; a population
of 72 distinct particles beyond the small-batch schedule; the short-series kernel on one ragged call, and the resident-series path
on the same data.  Cases and references: tests/_predict_cases.py, built once per process; nothing is skipped: every particle must
come back with info == 0.  Each test prints its worst distance / R and the smallest multiple at which it would pass (run with -s);
the figures of one MI355X run are in profiles/predict_error_scale.txt.

Found by these tests and NOT fixed here (test_known_cancellation: strict expected failures of the bound alone, one per particle
that misses; every other assertion on those particles — info, counters, the old criterion, a cap on the miss — is made outside the
mark): at a query ON a training time the training-point shortcut and the structured pass form mean = x_u - noise alpha_u and
var = noise - noise^2 (K^-1)_uu; where the noise exceeds the kernel's amplitude by 10 .. 1e3 both are differences of near-equal terms."""
import numpy as np
import pytest

import _predict_cases as PCS
from oracle import predcheck as PC

pytestmark = pytest.mark.gpu

# A case's own multiple: twice the smallest multiple at which it passed on an MI355X, rounded up to a power of two, never above 64;
# a case that passed at 8 stays at 8 (profiles/predict_error_scale.txt has the figures, with the reference routes' LAPACK on one
# thread; R moves by some 20 % with LAPACK's summation order, and with it on all threads the same outputs measured up to 16.8).  Every
# miss of the dense, shortcut and resident routes at 8 was at noise 1e-5 and none at noise 0.1 — amplified rounding, not a wrong term
# — and on the particle on which a correct double-precision route misses too: the blocked 16 x 16 algorithm of
# tests/_series_predict_ref.py in NumPy, on the oracle's own entries, needs 9.0 R_mean for the ChangePoint at noise 1e-5 on 176
# irregular times.  The dense factorisation keeps the inverses of its 16 x 16 diagonal blocks and multiplies by them as that route
# does, and the device's exp / tanh / sin leave the entries of a ChangePoint or a Periodic further from the oracle's than the 2 ulp of
# R's third route.  The small-amplitude kernel runs at 8 on every route but one: on the business-day calendar, at noise 0.1, R_mean is
# 9e-16 — LAPACK's dot products of 300 terms came within 0.3 eps S_mean of the 80-bit value, closer than a sum of 300 terms in another
# order has to (sqrt(n) eps S_mean) — and the lattice pass is 4.3 eps S_mean away, 10.8 R_mean.
MULT_REST = {"joint_17": 32, "joint_129": 32, "joint_means_129": 32,      # measured 12.1, 13.3, 12.6: the ChangePoint / SE + SE at noise 1e-5
             "train_route_300": 32, "train_route_below_300": 32}          # measured 13.0, 11.3: the ChangePoint at noise 1e-5
MULT_SMALL = {"lattice_business_days_300": 32,          # measured 10.8 at noise 0.1
              "train_route_300": 32}                    # measured 11.1 at noise 1e-3: the cancellation below at its onset (noise = 10 x amplitude)
# The known cancellation (module docstring): (route, noise of Constant(1e-4) * SE) -> cap on the smallest passing multiple, twice the
# measured one rounded up to a power of two.  Above 64: test_known_cancellation.
KNOWN_MISS = {("train_route_300", PCS.NOISES[2]): 8192,                 # noise 0.1: measured 2476 (variance; the mean 57 R_mean)
              ("structured_420", PCS.STRUCTURED_NOISES[2]): 128,        # noise 1e-3: measured 59.5
              ("structured_420", PCS.STRUCTURED_NOISES[3]): 8192,       # noise 1e-2: measured 2076
              ("structured_420", PCS.STRUCTURED_NOISES[4]): 131072}     # noise 0.1: measured 46928 (variance; the mean 222 R_mean)


def kernel_of(c, i):
    return i // (len(c.nodes) // len(PCS.family()))


def check_all(name, res, c, key=None, want_cov=False):
    """assert_predictive of every particle of case c (all of them must have info == 0) at the multiple of (key, kernel); all failures
    reported together.  A particle of KNOWN_MISS is held to info == 0, the old criterion and its cap instead.  Prints, before it
    asserts, the smallest multiple at which every output would pass: of the small-amplitude kernel per noise, of the rest together."""
    mean, var, cov, info = res
    refs = c.refs()
    key = c.name if key is None else key
    assert len(mean) == len(refs)
    assert (np.asarray(info) == 0).all(), (name, info)
    fails, need_rest, need_small = [], 0.0, []
    for i, r in enumerate(refs):
        ci = cov[i] if want_cov else None
        small = kernel_of(c, i) == PCS.SMALL_AMPLITUDE
        assert np.isfinite(mean[i]).all() and np.isfinite(var[i]).all(), (name, i)
        need = r.needed_mult(mean[i], var[i], ci)
        if small: need_small.append(need)
        else: need_rest = max(need_rest, need)
        cap = KNOWN_MISS.get((key, r.noise)) if small else None
        try:
            if cap is not None:
                PC.assert_caps(r, (name, i))
                assert PC.passes_old_criterion(mean[i], var[i], r, ci), (name, i, "known miss: the old criterion")
                assert need <= cap, (name, i, "known miss: smallest passing multiple", need, "above its cap", cap)
            else:
                mult = MULT_SMALL.get(key, PC.MULT) if small else MULT_REST.get(key, PC.MULT)
                PC.assert_predictive(mean[i], var[i], r, cov=ci, mult=mult, ctx=(name, i, r.tree, r.noise))
        except AssertionError as e:
            fails.append(str(e))
    print(f"[pred-components] {name}: smallest passing multiple: small-amplitude kernel by noise [{', '.join(f'{x:.3f}' for x in need_small)}]"
          f" at {MULT_SMALL.get(key, PC.MULT):g}, the other {len(refs) - len(need_small)} particles {need_rest:.3f} at {MULT_REST.get(key, PC.MULT):g}"
          + (f"  ({len(fails)} particles fail)" if fails else ""))
    assert not fails, "\n".join(fails)


def predict(e, c, want_cov=False):
    return e.predict_batch(c.nodes, c.noises, c.tq, n=c.n, noise_pred=c.noise_pred, want_cov=want_cov, check=False, **c.means_kw)


def counters(e):
    return np.array([e.lag_predict_passes(), e.predict_structured_particles(), e.predict_reuse_stats()["reused"]])


@pytest.mark.parametrize("want_cov", [False, True])
@pytest.mark.parametrize("name", ["joint_17", "joint_129", "joint_300", "joint_means_129", "joint_noise_pred_17"])
def test_general_joint_path(pkg, name, want_cov):
    """Irregular times with one duplicated time: one padded tile, two tiles, three tile rows with a ragged last row.  With the
    covariance: every entry is checked and the diagonal is the marginal variance."""
    c = PCS.case(name)
    e = pkg.GPEngine(0)
    try:
        e.set_data(c.ts, c.xs)
        assert e.lattice_stats()["kind"] == 0
        res = predict(e, c, want_cov)
        assert (counters(e) == 0).all(), counters(e)          # no lattice pass, no structured pass, nothing resident
        check_all(f"joint {name} cov={want_cov}", res, c, want_cov=want_cov)
        if want_cov:
            assert np.array_equal(np.diagonal(res[2], axis1=1, axis2=2), res[1])
    finally:
        e.close()


def run_training_point_route(pkg, name):
    """the marginal call of a train_route case, with the evidence of which route it took"""
    c = PCS.case(name)
    on_train = np.isin(c.tq, c.ts[:c.n])
    taken = name == "train_route_300"
    assert on_train.sum() == PCS.TRAIN_ROUTE_MIN - (0 if taken else 1) and c.tq.size >= PCS.TRAIN_ROUTE_MIN and 3 * on_train.sum() >= c.n
    e = pkg.GPEngine(0)
    try:
        e.set_data(c.ts, c.xs)
        res = predict(e, c)
        joint = predict(e, c, want_cov=True)
        assert (counters(e) == 0).all()
        same = np.array_equal(res[1][:, on_train], joint[1][:, on_train])
        assert same == (not taken), (name, "variances at the training-time queries equal the joint pass's bit for bit:", same)
    finally:
        e.close()
    return c, res


@pytest.mark.parametrize("name", ["train_route_300", "train_route_below_300"])
def test_training_point_route(pkg, name):
    """joint_300's series with TRAIN_ROUTE_MIN queries on training times (mean = x - noise alpha, var = noise - noise^2 (K^-1)_ii from
    L^-T) and with one fewer (every query through the joint matrix).  The engine keeps no counter of this route; that it ran shows in
    the bits: a request for the covariance never takes it, and below the threshold the marginal call is that call's joint pass."""
    c, res = run_training_point_route(pkg, name)
    check_all(name, res, c)


@pytest.mark.parametrize("name,kind", [("lattice_grid_300", 1), ("lattice_business_days_300", 2)])
def test_lattice_pass_on_rank_tables(pkg, name, kind):
    """Queries on the series' own lattice: a shuffled regular grid; business days (a lattice with gaps: the weekend days between
    training times are lattice points too)."""
    c = PCS.case(name)
    e = pkg.GPEngine(0)
    try:
        e.set_data(c.ts, c.xs)
        assert e.lattice_stats()["kind"] == kind
        k0 = counters(e)
        res = predict(e, c)
        assert (counters(e) - k0).tolist() == [1, 0, 0], counters(e) - k0
        check_all(name, res, c)
    finally:
        e.close()


def run_structured_pass(pkg, monkeypatch):
    """(case, the structured pass's result, its dense twin's): the Toeplitz-class particles counted"""
    c = PCS.case("structured_420")
    n_class = PCS.N_TOEPLITZ_CLASS * len(PCS.STRUCTURED_NOISES)
    assert n_class >= PCS.STRUCT_PRED_MIN_CLASS
    a = pkg.GPEngine(0)
    monkeypatch.setenv("AGP_GRAD_FFT", "2")
    b = pkg.GPEngine(0)
    monkeypatch.delenv("AGP_GRAD_FFT")
    try:
        a.set_data(c.ts, c.xs); b.set_data(c.ts, c.xs)
        ra = predict(a, c)
        rb = predict(b, c)
        assert a.predict_structured_particles() == n_class and b.predict_structured_particles() == 0
    finally:
        a.close(); b.close()
    return c, ra, rb


def test_structured_pass(pkg, monkeypatch):
    """The whole of a 420-point grid, marginals only: the Toeplitz-class particles go through the joint Schur recursion without a
    dense factor, the ChangePoints through the dense pass beside them; a context with AGP_GRAD_FFT=2 is the dense twin."""
    c, ra, rb = run_structured_pass(pkg, monkeypatch)
    check_all("structured_420 dense twin", rb, c, key="structured_420 dense twin")
    check_all("structured_420", ra, c)


@pytest.mark.xfail(strict=True, raises=PC.BoundMiss, reason="x_u - noise alpha_u and noise - noise^2 (K^-1)_uu cancel where the noise exceeds the "
                   "kernel's amplitude; the smallest passing multiples are in profiles/predict_error_scale.txt, their caps in KNOWN_MISS")
@pytest.mark.parametrize("route,noise", sorted(KNOWN_MISS))
def test_known_cancellation(pkg, monkeypatch, route, noise):
    """The bound itself on the particles of KNOWN_MISS, at the small-amplitude kernel's multiple of 8: expected to miss (only
    PC.BoundMiss is expected; the day the form is replaced this passes, and strictly so fails until KNOWN_MISS loses the entry)."""
    c, res = run_training_point_route(pkg, route) if route == "train_route_300" else run_structured_pass(pkg, monkeypatch)[:2]
    (i,) = [i for i in range(len(c.nodes)) if kernel_of(c, i) == PCS.SMALL_AMPLITUDE and c.noises[i] == noise]
    assert res[3][i] == 0
    PC.assert_predictive(res[0][i], res[1][i], c.refs()[i], mult=PC.MULT, ctx=(route, noise))


@pytest.mark.parametrize("name", ["joint_300", "resident_prefix_200"])
def test_resident_factors(pkg, name):
    """logpdf_batch_extend at the same prefix first (n = n_max and n < n_max): the predictive pass starts from the factors it left."""
    c = PCS.case(name)
    e = pkg.GPEngine(0)
    try:
        e.set_data(c.ts, c.xs)
        _, info = e.logpdf_batch_extend(c.nodes, c.noises, n=c.n, check=False)
        assert (info == 0).all()
        r0 = e.predict_reuse_stats()["reused"]
        res = predict(e, c)
        assert e.predict_reuse_stats()["reused"] - r0 == len(c.nodes), e.predict_reuse_stats()
        check_all(f"resident {name}", res, c, key=f"resident {name}")
    finally:
        e.close()


def test_population_schedules(pkg):
    """72 distinct particles (the family at eight noises) on the shuffled grid with lattice queries: beyond the small-batch schedule"""
    c = PCS.case("population_300")
    assert len(c.nodes) >= 70 and len(c.nodes) > PCS.RIGHT_LOOKING_MAX_PARTICLES
    assert len({(k.to_tuple(), nz) for k, nz in zip(c.nodes, c.noises)}) == len(c.nodes)
    e = pkg.GPEngine(0)
    try:
        e.set_data(c.ts, c.xs)
        res = predict(e, c)
        assert counters(e).tolist() == [1, 0, 0]
        check_all("population_300", res, c)
    finally:
        e.close()


def test_predict_series_batch(pkg, engine):
    """One ragged call with series of 17, 144 and SERIES_MAX_N points; then the resident-series path (route 1) on the same data: its
    variance under the same bound as the short-series kernel's (mult = 8), its mean at the dense case's own multiple."""
    cs = [PCS.case(nm) for nm in ("joint_17", "series_144", f"series_{pkg.SERIES_MAX_N}")]
    assert [c.n for c in cs] == [17, 144, pkg.SERIES_MAX_N]
    nodes = [k for c in cs for k in c.nodes]
    noises = np.concatenate([c.noises for c in cs])
    sidx = np.repeat(np.arange(3, dtype=np.int32), [len(c.nodes) for c in cs])
    means, vars_, info = engine.predict_series_batch([(c.ts, c.xs) for c in cs], [c.tq for c in cs], nodes, noises, sidx,
                                                     noise_pred=np.concatenate([c.noise_pred for c in cs]), check=False)
    assert (info == 0).all(), info
    at = 0
    for c in cs:
        P = len(c.nodes)
        check_all(f"predict_series_batch n={c.n}", (means[at:at + P], vars_[at:at + P], None, info[at:at + P]), c, key=f"series kernel {c.n}")
        at += P
    e = pkg.GPEngine(0)
    try:
        for c in cs:
            e.set_data(c.ts, c.xs)
            res = predict(e, c)
            check_all(f"predict_batch on the series of n={c.n}", res, c)
            for i, r in enumerate(c.refs()):
                assert (r.errors(res[0][i], res[1][i])[1] <= r.bounds(PC.MULT)[1]).all(), (c.n, i, "route 1's variance at mult = 8")
    finally:
        e.close()
