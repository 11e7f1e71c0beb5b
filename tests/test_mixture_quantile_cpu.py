"""CPU checks of the mixture-quantile restatement (tests/_mixture_quantile_ref.py) that the GPU tests of agp_mixture_quantile /
agp_predict_quantile_batch compare against, and of the entries' declarations."""
import re
import sys
from pathlib import Path

import mpmath as mp
import numpy as np
import pytest
from scipy.special import erfc

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mixture_quantile_ref as R      # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("agp_mixture_quantile", "agp_predict_quantile_batch")


def assert_same(a, b):
    assert R.same_bits(a, b).all(), (a, b)


@pytest.mark.parametrize("P,m,max_iter", [(1, 9, 10**6), (3, 17, 10**6), (64, 33, 10**6), (65, 40, 12), (200, 25, 5),
                                          (7, 30, 1), (5, 8, 0)])
@pytest.mark.parametrize("q", [0.025, 0.5, 0.975])
def test_loop_and_search_agree_bitwise(P, m, max_iter, q):
    """(a) the reference's vectorised loop and (b) the per-point search: same x bit for bit, success = AND of the converged flags,
    with max_iter reached (small max_iter) and not reached."""
    rng = np.random.default_rng(P * 1000 + m)
    means, vars_, w = R.random_mixture(rng, P, m, scale=[1.0, 30.0, 0.01][P % 3], shift=[0.0, 5.0, -2.0][m % 3])
    xa, sa = R.quantile_loop(means, vars_, w, q, tol=1e-6, max_iter=max_iter)
    b = R.quantile_search(means, vars_, w, q, tol=1e-6, max_iter=max_iter)
    assert_same(xa, b["x"])
    assert sa == bool(b["converged"].all())
    assert (b["iters"] <= max(max_iter, 0)).all()
    if max_iter >= 10**6:
        assert sa
    if max_iter == 0:
        assert (b["x"] == 0).all() and not sa and (b["iters"] == 0).all()


def test_fixed_point_exit_equals_full_max_iter():
    """A tol below what the fp64 CDF resolves: a point either hits eps == 0 exactly (converged) or ends at a fixed point; running
    the literal loop for the full max_iter gives the same x."""
    rng = np.random.default_rng(3)
    means, vars_, w = R.random_mixture(rng, 6, 12)
    b = R.quantile_search(means, vars_, w, 0.3, tol=1e-300, max_iter=5000)
    assert (~b["converged"]).sum() >= 4 and (b["iters"] < 5000).all()
    xa, sa = R.quantile_loop(means, vars_, w, 0.3, tol=1e-300, max_iter=5000)
    assert not sa
    assert_same(xa, b["x"])
    # the search stopped at a point where one more update changes nothing
    b2 = R.quantile_search(means, vars_, w, 0.3, tol=1e-300, max_iter=int(b["iters"].max()) + 7)
    assert_same(b2["x"], b["x"]) and np.array_equal(b2["iters"], b["iters"])


@pytest.mark.parametrize("q", [0.001, 0.025, 0.3, 0.5, 0.975, 0.999])
@pytest.mark.parametrize("mu,sd", [(0.0, 1.0), (3.0, 0.2), (-250.0, 40.0), (1e-3, 1e-4)])
def test_single_component_is_the_normal_quantile(q, mu, sd):
    b = R.quantile_search(np.full((1, 1), mu), np.full((1, 1), sd * sd), np.ones(1), q, tol=1e-9)
    assert b["converged"].all()
    with mp.workdps(40):
        exact = mp.mpf(mu) + mp.mpf(sd) * mp.sqrt(2) * mp.erfinv(2 * mp.mpf(q) - 1)
        assert abs(R.mp_cdf(b["x"][0], [mu], [sd], [1.0]) - q) < 1e-9 + 1e-15
        # x within the tolerance, in x: |F(x) - q| < tol and F' = pdf
        assert abs(float(b["x"][0] - exact)) <= 1e-9 / float(mp.npdf(exact, mu, sd)) * 1.01 + 1e-15 * abs(mu)


@pytest.mark.parametrize("case", ["q_tiny", "q_near_1", "tol_zero", "nan_at_zero_weight", "huge_scale", "tiny_scale", "sigma_zero",
                                  "underflowed_weights"])
def test_edge_cases_terminate(case):
    rng = np.random.default_rng(11)
    means, vars_, w = R.random_mixture(rng, 9, 10)
    q, tol = 0.4, 1e-5
    if case == "q_tiny":
        q = 1e-300
    elif case == "q_near_1":
        q = 1.0 - 2.0 ** -53
    elif case == "tol_zero":
        tol = 0.0
    elif case == "nan_at_zero_weight":
        w[3] = 0.0; w /= w.sum(); means[3] = np.nan; vars_[3] = np.nan
    elif case == "huge_scale":
        means *= 1e150; vars_ *= 1e300
    elif case == "tiny_scale":
        means *= 1e-150; vars_ *= 1e-300
    elif case == "sigma_zero":
        vars_[::2] = 0.0
    elif case == "underflowed_weights":
        w[:4] = [1e-320, 5e-324, 0.0, 1e-310]; w[4:] /= w[4:].sum()
    b = R.quantile_search(means, vars_, w, q, tol=tol, max_iter=10**6)
    assert (b["iters"] < 10**4).all(), b["iters"].max()
    assert not np.isnan(b["x"]).any()
    for mi in (int(b["iters"].max()) + 3, int(b["iters"].max()) + 4):      # (both parities of a 2-cycle's exit)
        xa, sa = R.quantile_loop(means, vars_, w, q, tol=tol, max_iter=mi)
        bb = R.quantile_search(means, vars_, w, q, tol=tol, max_iter=mi)
        assert_same(xa, bb["x"])
        assert sa == bool(bb["converged"].all())
    if case in ("nan_at_zero_weight", "huge_scale", "tiny_scale", "underflowed_weights"):
        assert b["converged"].all()
        M, S = R.components(means, vars_)
        for i in range(0, 10, 3):
            assert abs(R.mp_cdf(b["x"][i], M[i], S[i], w) - q) < tol + R.delta(9)
    if case == "tol_zero":
        assert not b["converged"].any()


def test_erfc_bound_numpy():
    """scipy's erfc (the restatement's CDF) against mpmath on the arguments -z / sqrt 2, z in [-40, 10]: within ERFC_ULP_NP ulps
    of the result, so two CDFs agree to delta(P)."""
    rng = np.random.default_rng(0)
    z = np.concatenate([np.linspace(-40.0, 10.0, 4001), rng.uniform(-40.0, 10.0, 4000), rng.uniform(-1.0, 1.0, 1000)])
    t = -z * R.INVSQRT2
    worst = R.erfc_err_ulps(erfc(t), t)
    assert worst <= R.ERFC_ULP_NP, worst
    assert R.delta(2048) < 1e-13


def test_normcdf_matches_mpmath():
    with mp.workdps(40):
        for x, mu, sd in ((0.3, 0.0, 1.0), (-7.0, 1.0, 0.5), (12.0, -3.0, 2.0), (1.0, 1.0, 0.0), (0.5, 1.0, 0.0), (2.0, 1.0, 0.0)):
            got = float(R.normcdf(np.float64(x), np.float64(mu), np.float64(sd)))
            ref = R.mp_cdf(x, [mu], [sd], [1.0])
            # (absolute: the rounding of -z * invsqrt2, shared with the reference, moves the far tails relatively)
            assert abs(got - ref) <= 4 * 2.0 ** -53, (x, mu, sd, got, ref)


def test_symbols_declared_and_exported(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), s
        assert s in pkg.EXPORTED_SYMBOLS, s
    jl = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    for s in SYMBOLS:
        assert f"(:{s}, LIB)" in jl, s
    for name in ("predict_quantile", "predict_quantile_multi", "raw_components"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.GPEngine, "mixture_quantile") and hasattr(pkg.GPEngine, "predict_quantile_batch")
    assert hasattr(pkg.GPEngineMulti, "predict_quantile_batch")


def test_raw_components_transform(pkg):
    """predict_mvn's raw-space map (src/Transforms.jl:44-49) in its operation order, and the info of a bad variance."""
    rng = np.random.default_rng(2)
    mean = rng.standard_normal((3, 5)); var = rng.random((3, 5))
    var[1, 3] = -1e-12; var[2, 0] = np.nan
    mr, vr, info = pkg.raw_components(mean, var, np.array([0, 0, 0], np.int32), 100, (0.37, -1.25))
    assert np.array_equal(mr, (mean - (-1.25)) / 0.37)
    assert R.same_bits(vr, (1.0 / (0.37 * 0.37)) * var).all()
    assert info.tolist() == [0, 104, 101]
    _, _, info2 = pkg.raw_components(mean, var, np.array([7, 0, 0], np.int32), 100)
    assert info2.tolist() == [7, 104, 101]
