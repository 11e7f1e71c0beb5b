"""Host-side checks of the mixture moments' restatement (tests/_mixture_moments_ref.py): against the definition term by term in mpmath
on tiny cases, the closed forms of a single component, the mixture of equal components, and that the one-pass formula the kernels
avoid misses the bounds the device is held to.  No device."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _mixture_moments_ref as R      # noqa: E402


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("P,m", [(1, 1), (2, 3), (5, 4), (7, 2)])
def test_restatement_against_the_definition(P, m, space):
    rng = np.random.default_rng(100 * P + 10 * m + space)
    kw = dict(offset=1e6, spread=1.0) if space == 0 else dict(offset=2.0, spread=0.4, vscale=0.1)
    means, vars_, covs, w = R.random_mixture(rng, P, m, **kw)
    out = R.moments(means, w, covs=covs, space=space)
    bm, bc = R.brute_force(means, w, covs, space)
    # (both are correctly rounded values of the same rationals / 200-bit sums: equal to an ulp of the result)
    assert np.abs(out["mean"] - bm).max() <= R.EPS * np.abs(bm).max()
    assert np.abs(out["cov_full"] - bc).max() <= R.EPS * max(np.abs(bc).max(), 1e-300)
    assert np.array_equal(out["var"], np.diag(out["cov_full"]))
    assert (out["cov_bound"] >= 0).all() and (out["mean_bound"] > 0).all()
    # the marginal entry (vars only) is the diagonal of the full one
    marg = R.moments(means, w, vars=vars_, space=space)
    assert np.array_equal(marg["mean"], out["mean"]) and np.array_equal(marg["var"], out["var"])
    # a subset of the pairs gives the same elements
    sub = R.moments(means, w, covs=covs, space=space, pairs=[(m - 1, 0), (0, 0)])
    assert sub["cov"][0] == out["cov_full"][m - 1, 0] and sub["cov"][1] == out["cov_full"][0, 0]


def test_single_component_is_itself_and_lognormal_closed_forms():
    rng = np.random.default_rng(3)
    means, vars_, covs, w = R.random_mixture(rng, 1, 5, offset=1.5, spread=0.5, vscale=0.2)
    out = R.moments(means, w, covs=covs, space=0)
    assert np.array_equal(out["mean"], means[0]) and np.array_equal(out["cov_full"], covs[0])
    ln = R.moments(means, w, covs=covs, space=1)
    # Transforms.unapply_mean_var(::LogTransform, mu, var): (exp(mu + var / 2), (exp(var) - 1) exp(2 mu + var))
    mu, v = means[0], vars_[0]
    assert np.allclose(ln["mean"], np.exp(mu + v / 2), rtol=4 * R.EPS, atol=0)
    assert np.allclose(ln["var"], np.expm1(v) * np.exp(2 * mu + v), rtol=8 * R.EPS, atol=0)
    e = np.exp(mu + v / 2)
    assert np.allclose(ln["cov_full"], np.outer(e, e) * np.expm1(covs[0]), rtol=8 * R.EPS, atol=0)


@pytest.mark.parametrize("space", [0, 1])
def test_equal_components_give_the_component(space):
    rng = np.random.default_rng(5)
    means, _, covs, _ = R.random_mixture(rng, 1, 4, offset=1.0, spread=0.3, vscale=0.1)
    P = 6
    w = rng.random(P); w /= w.sum()
    one = R.moments(means, np.ones(1), covs=covs, space=space)
    mix = R.moments(np.repeat(means, P, axis=0), w, covs=np.repeat(covs, P, axis=0), space=space)
    assert np.array_equal(mix["mean"], one["mean"]) and np.array_equal(mix["cov_full"], one["cov_full"])


def test_one_pass_formula_misses_the_bounds_on_a_common_offset():
    """sum w (C + mu mu') - mean mean' in fp64, at an offset 10^6 times the spread: wrong by many times the bound."""
    rng = np.random.default_rng(9)
    means, _, covs, w = R.random_mixture(rng, 9, 6, offset=1e6, spread=1.0)
    out = R.moments(means, w, covs=covs)
    _, c1 = R.one_pass(means, w, covs)
    got = np.array([c1[i, j] for i, j in out["pairs"]])
    assert (np.abs(got - out["cov"]) > 100 * out["cov_bound"]).any()


def test_generator_covers_its_cases():
    rng = np.random.default_rng(1)
    means, vars_, covs, w = R.random_mixture(rng, 65, 17, offset=1e6)
    assert abs(w.sum() - 1.0) <= 4 * R.EPS and (w == 0).sum() >= 2 and w[0] == 0.0 and w.max() >= 0.85
    assert (vars_ == 0).any() and (covs.reshape(65, -1) == 0).all(axis=1).any()
    assert np.abs(means - 1e6).max() < 10.0
    assert np.array_equal(covs, covs.transpose(0, 2, 1))


def test_entries_are_declared():
    import __graft_entry__ as g
    pkg = g.load_package()
    for sym in ("agp_mixture_moments", "agp_predict_mixture_batch"):
        assert sym in pkg.EXPORTED_SYMBOLS
    assert callable(pkg.predict_mvn) and hasattr(pkg.MixtureModel, "lognormal")
