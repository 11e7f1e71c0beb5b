"""CPU tests of the many-short-series predictive entry (agp_predict_series_batch): its declaration, export, documentation and
bindings; the kernel's block algorithm restated in NumPy (tests/_series_predict_ref.py) against oracle.predict_mvn; the Python-side
validation, which runs before any library call; and the LDS map's ChangePoint-table count quoted in the header."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _series_predict_ref as R
from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent
SYM = "agp_predict_series_batch"


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert SYM in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint %s\s*\(" % SYM, hdr)
    assert SYM in (ROOT / "INTEGRATION.md").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and SYM in seen
    assert hasattr(pkg.GPEngine, "predict_series_batch") and hasattr(pkg, "pack_queries")
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    # the docstring sits directly above its own definition
    assert re.search(r'"\nfunction predict_series_batch\(', shim)


def trees(G):
    return [G.SquaredExponential(0.3, 0.8),
            G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Periodic(0.5, 0.1, 0.8) + G.WhiteNoise(0.1), 0.45, 0.05),
            G.Linear(0.3, 0.2, 0.7) * G.SquaredExponential(0.25, 0.8) + G.Constant(0.1)]


@pytest.mark.parametrize("m", [1, 16, 17])
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 176])
def test_block_algorithm_against_the_oracle(pkg, n, m):
    """index algebra of the query block rows on the packed blocks, the masks of the padding columns and rows: mean and variance
    within 1e-8 max(1, max|ref|) of oracle.predict_mvn; queries past the series, on a training time and between two"""
    ts, xs = pkg.prior.synthetic_series(256, seed=40 + n, shuffle=True)
    tq = R.queries_for(ts, ts[:n], m)
    if m < 3:
        tq[0] = ts[0]                                    # a training time among the queries at every size
    ts, xs = ts[:n].copy(), xs[:n].copy()
    for node, noise, noise_pred in zip(trees(pkg), (0.1, 0.05, 0.2), (None, 0.3, 0.0)):
        mu, cov = O.predict_mvn(node.to_tuple(), noise, ts, xs, tq, noise_pred=noise_pred)
        mean, var = R.series_predict_blocks(node.to_tuple(), noise, ts, xs, tq, noise_pred=noise_pred)
        assert R.close(mean, mu), (n, m, node.to_tuple(), np.abs(mean - mu).max())
        assert R.close(var, np.diag(cov)), (n, m, node.to_tuple(), np.abs(var - np.diag(cov)).max())


def test_block_algorithm_prior_predictive(pkg):
    """an empty series: no block, mean 0, var = k(t*, t*) + noise_pred"""
    node = trees(pkg)[1]
    tq = np.array([0.1, 0.45, 0.45, 0.9])
    mu, cov = O.predict_mvn(node.to_tuple(), 0.1, np.zeros(0), np.zeros(0), tq, noise_pred=0.2)
    mean, var = R.series_predict_blocks(node.to_tuple(), 0.1, np.zeros(0), np.zeros(0), tq, noise_pred=0.2)
    assert (mean == 0.0).all() and (mu == 0.0).all() and R.close(var, np.diag(cov))


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_python_side_validation_runs_before_any_library_call(pkg):
    good = pkg.SquaredExponential(0.3, 0.8)
    ok = (np.linspace(0, 1, 5), np.zeros(5))
    q = np.array([1.1, 1.2])
    eng = object.__new__(pkg.GPEngine)
    eng._lib = _NoLibrary(); eng._ctx = None
    entry = eng.predict_series_batch
    with pytest.raises(ValueError, match="one vector of query times per series"):
        entry([ok, ok], [q], [good], [0.1], [0])
    with pytest.raises(ValueError, match="one vector of query times per series"):
        entry([ok], [q, q], [good], [0.1], [0])
    with pytest.raises(ValueError, match="series 1: the query times must be a vector"):
        entry([ok, ok], [q, q[None, :]], [good], [0.1], [0])
    with pytest.raises(ValueError, match="one noise_pred per particle"):
        entry([ok], [q], [good, good], [0.1, 0.1], [0, 0], noise_pred=[0.1])
    with pytest.raises(ValueError, match="one noise_pred per particle"):
        entry([ok], [q], [good, good], [0.1, 0.1], [0, 0], noise_pred=[[0.1, 0.1]])
    # ... and everything the value entries refuse
    with pytest.raises(ValueError, match="one noise per particle"):
        entry([ok], [q], [good, good], [0.1], [0, 0])
    with pytest.raises(ValueError, match="one series index per particle"):
        entry([ok], [q], [good], [0.1], [0, 0])
    n = pkg.SERIES_MAX_N + 1
    with pytest.raises(ValueError, match="series 1 has %d points" % n):
        entry([ok, (np.zeros(n), np.zeros(n))], [q, q], [good], [0.1], [0])
    # the helper itself
    q_off, ts_pred, npred = pkg.pack_queries([q, np.zeros(0), [3.0]], 3, [0.1, 0.2], 2)
    assert q_off.tolist() == [0, 2, 2, 3] and q_off.dtype == np.int64 and ts_pred.tolist() == [1.1, 1.2, 3.0]
    assert npred.dtype == np.float64 and npred.tolist() == [0.1, 0.2]
    assert pkg.pack_queries([], 0)[0].tolist() == [0]


def test_changepoint_tables_at_the_cap_match_the_header(pkg):
    """the number the header quotes is the one the map gives, and it is the value entry's"""
    import _series_grad_ref as G
    N = pkg.SERIES_MAX_N
    fit = max(k for k in range(1, 40) if R.cp_chain_fits(k, N))
    assert fit == max(k for k in range(1, 40) if G.cp_chain_fits(k, N, grad=False))
    assert R.cp_chain_fits(fit + 8, 100)                 # the same chains fit a 100-point series
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    doc = hdr[hdr.index("Forecasts of many short series"):hdr.index("int %s(" % SYM)]
    m = re.search(r"a chain of (\d+) ChangePoint nodes \((\d+) nodes, (\d+) parameters,\s*\*?\s*(\d+) per-point tables\) fits and one of (\d+) does not",
                  doc)
    assert m, "the header states the count"
    assert [int(x) for x in m.groups()] == [fit, 2 * fit + 1, 3 * fit + 1, fit, fit + 1]
    # the predictive kernel's map IS the value kernel's: one expression in csrc/agp_args.hpp, and the query entries behind the series'
    src = (ROOT / "autogp.jl_amd" / "csrc" / "agp_args.hpp").read_text()
    assert "series_pred_lds(int n, int n_ops, int n_prm, int n_cp) { return series_lds(n, n_ops, n_prm, n_cp); }" in src
    assert "constexpr int SERIES_QSLOT = 192;" in src and N <= 192


def test_ragged_case_is_the_stated_one(pkg):
    """the GPU test's shared input: the stated lengths, a training time and a midpoint among the queries, no particle the oracle
    cannot factor, and variances far from cancellation"""
    series, queries, nodes, noises, sidx, ref_mean, ref_var = R.ragged_case()
    assert [len(t) for t, _ in series] == list(R.RAGGED_N) and [len(q) for q in queries] == list(R.RAGGED_M)
    assert len(nodes) == 60
    for s, ((ts, _), q) in enumerate(zip(series, queries)):
        if len(q) >= 3 and len(ts) >= 2:
            assert q[0] == ts[0] and q[1] == 0.5 * (ts[0] + ts[1])
    assert all(np.isfinite(a).all() for a in ref_mean + ref_var)
    assert min(v.min() for v in ref_var if v.size) > 0.01
    for nd, nz, s in zip(nodes, noises, sidx):           # every training covariance factors: info == 0 is the only right answer
        if len(series[s][0]):
            np.linalg.cholesky(O.compute_cov_matrix_vectorized(nd.to_tuple(), float(nz), series[s][0]))
