"""CPU tests of the predictive log-density (agp_predict_logpdf_batch): the reference restatement of tests/_pred_logpdf_ref.py
against its mpmath / 80-bit twins and the reference's Bayes identity, the raw-space Jacobian of predict_proba, and the entry's
declaration, export and Julia binding."""
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import _pred_logpdf_ref as R      # noqa: E402


def fixture_trees(G):
    base = [G.WhiteNoise(1), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
            G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1)]      # test/test_GP.jl:24-33
    comp = [base[2] + base[5], base[3] * base[4], G.ChangePoint(base[2], base[5], 0.5, 0.05),
            G.ChangePoint(base[3] + base[4], base[2] * base[5], 0.3, 0.2)]
    return [k.to_tuple() for k in base + comp]


def series(n, m, seed):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.random(n)); xs = 0.5 * rng.standard_normal(n)
    tp = np.concatenate([rng.random(m // 2), 1.0 + 0.2 * rng.random(m - m // 2)])
    y = 0.5 * rng.standard_normal(m)
    return ts, xs, tp, y


def test_helper_matches_mpmath_twin(pkg):
    for i, tree in enumerate(fixture_trees(pkg)):
        for n, m in ((0, 5), (1, 1), (7, 4), (23, 17), (40, 40)):
            ts, xs, tp, y = series(n, m, 100 * i + n)
            for npred in (None, 0.07):
                lp, S = R.reference(tree, 0.2, ts, xs, tp, y, noise_pred=npred)
                lm = R.reference_mp(tree, 0.2, ts, xs, tp, y, noise_pred=npred)
                assert abs(lp - lm) <= 1e-10 * S, (tree, n, m, lp, lm, S)
                ll = R.reference_ld(tree, 0.2, ts, xs, tp, y, noise_pred=npred)
                assert abs(ll - lm) <= 1e-10 * S, (tree, n, m, ll, lm, S)


def test_helper_mean_functions(pkg):
    tree = fixture_trees(pkg)[6]
    ts, xs, tp, y = series(30, 12, 5)
    mt = 0.3 * ts - 0.1; mp_ = 0.3 * tp - 0.1
    lp, S = R.reference(tree, 0.1, ts, xs, tp, y, mean_train=mt, mean_pred=mp_)
    lm = R.reference_mp(tree, 0.1, ts, xs, tp, y, mean_train=mt, mean_pred=mp_)
    assert abs(lp - lm) <= 1e-10 * S
    # oracle.predict_mvn's own mean-function form (a callable) gives the same predictive
    mu, cov = O.predict_mvn(tree, 0.1, ts, xs, tp, mean=lambda t: 0.3 * t - 0.1)
    assert abs(O.mvnormal_logpdf(y, cov, mu) - lp) <= 1e-12 * S


def test_helper_bayes_identity(pkg):
    """logpdf(joint) - logpdf(obs) = logpdf(predictive, y*) (test/experiment_hmc.jl:111-132), ChangePoints included."""
    for i, tree in enumerate(fixture_trees(pkg)):
        ts, xs, tp, y = series(60, 25, 7 + i)
        noise = 0.15
        lj = O.gp_logpdf(tree, noise, np.concatenate([ts, tp]), np.concatenate([xs, y]))
        lo = O.gp_logpdf(tree, noise, ts, xs)
        lp, S = R.reference(tree, noise, ts, xs, tp, y)       # noise_pred = noise: the joint model's predictive
        assert abs((lj - lo) - lp) <= 1e-9 * S, (tree, lj - lo, lp)


def test_helper_scale_and_edges(pkg):
    tree = fixture_trees(pkg)[3]
    ts, xs, tp, y = series(20, 6, 1)
    lp, S = R.reference(tree, 0.2, ts, xs, tp, y)
    assert S >= abs(lp) * 2 - 1e-9 and S > 6 * R.LOG2PI - 1e-12
    assert R.reference(tree, 0.2, ts, xs, tp[:0], y[:0]) == (0.0, 0.0)
    # n = 0: the prior predictive N(y; 0, K22 + noise_pred I)
    K = O.compute_cov_matrix_vectorized(tree, 0.05, tp)
    assert abs(R.reference(tree, 0.2, ts[:0], xs[:0], tp, y, noise_pred=0.05)[0] - O.mvnormal_logpdf(y, K)) <= 1e-12 * S


def test_raw_space_jacobian(pkg):
    """predict_proba scores RAW y under the un-transformed MvNormal (src/api.jl:515-519: mean (mu - b) / a, cov Sigma / a^2):
    logp_raw = logp_scaled(a y + b) + m log|a|."""
    tree = fixture_trees(pkg)[7]
    ts, xs, tp, y_scaled = series(40, 15, 3)
    for a, b in ((2.5, -0.3), (-0.04, 1.7)):
        y_raw = (y_scaled - b) / a
        mu, cov = R.predictive(tree, 0.1, ts, xs, tp)
        direct = O.mvnormal_logpdf(y_raw, cov / a ** 2, (mu - b) / a)
        lp, S = R.reference(tree, 0.1, ts, xs, tp, a * y_raw + b)
        assert abs(lp + len(tp) * math.log(abs(a)) - direct) <= 1e-10 * S


def test_entry_declared_exported_and_bound(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert re.search(r"\bint agp_predict_logpdf_batch\s*\(", hdr)
    assert "agp_predict_logpdf_batch" in pkg.EXPORTED_SYMBOLS
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    assert "ccall((:agp_predict_logpdf_batch, LIB)" in shim
    for fn in ("predict_logpdf", "predict_logpdf_batch"):
        # each docstring sits directly above its own definition (a stacked pair of string literals breaks `using AutoGPHIP`)
        m = re.search(r'"""\n((?:(?!""").)*)"""\nfunction ' + fn + r"\(", shim, re.S)
        assert m, fn
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and "agp_predict_logpdf_batch" in seen
    assert "agp_predict_logpdf_batch" in (ROOT / "INTEGRATION.md").read_text()
    assert callable(pkg.predict_proba) and hasattr(pkg.MvNormal, "logpdf")
    assert hasattr(pkg.GPEngine, "predict_logpdf_batch")
