"""CPU tests of the long-series forecast and band entries (agp_predict_long_series_batch, agp_predict_quantile_long_series_batch):
their declarations, exports, documentation and Julia bindings; the Python-side refusals; the Python twin of the kernel's LDS map
against the constants of csrc/agp_args.hpp; and the NumPy twin of stage P (tests/_long_series_predict_ref.py) against
oracle.predict_mvn, with three planted faults that the same tolerance catches.
Tolerance of the twin: |d| <= 1e-10 max(1, max|ref|) per particle block (_series_predict_ref.close's norm) — the oracle's route and an
independent float64 Cholesky route differ by at most 8.5e-14 in that norm on the GPU tests' ragged case, three orders below."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _long_series_predict_ref as LP
import _series_predict_ref as SP
from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("agp_predict_long_series_batch", "agp_predict_quantile_long_series_batch")
TWIN_TOL = 1e-10


def test_entries_are_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == []
    for sym in ENTRIES:
        assert sym in pkg.EXPORTED_SYMBOLS, sym
        m = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % sym, hdr)
        assert m and re.search(r"uint32_t\s+flags\s*$", m.group(1).strip()), sym      # the trailing flags word
        assert sym in doc and sym in seen, sym
    for name in ("predict_long_series_batch", "predict_quantile_long_series_batch"):
        assert hasattr(pkg.GPEngine, name), name
        assert re.search(r'"\nfunction %s\(' % name, shim), name                     # docstring directly above its own definition
    import inspect
    sig = inspect.signature(pkg.GPEngine.predict_long_series_batch)
    assert list(sig.parameters) == ["self", "series", "queries", "nodes", "noises", "series_index", "noise_pred", "want_logpdf",
                                    "all_long", "check", "programs"]
    assert sig.parameters["all_long"].default is False and sig.parameters["check"].default is True
    # the module-level band keeps its defaults: the short entry unless asked
    sig = inspect.signature(pkg.predict_quantile_series)
    assert sig.parameters["max_n"].default == pkg.SERIES_MAX_N and sig.parameters["all_long"].default is False


class NoLibrary:
    """stands where the loaded library would: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def test_bad_shapes_raise_before_any_library_call(pkg):
    eng = object.__new__(pkg.GPEngine)      # no library is loaded, no device is opened
    eng._lib = NoLibrary(); eng._ctx = None
    N = pkg.LONG_SERIES_MAX_N
    ok = (np.zeros(4), np.zeros(4))
    q = np.zeros(3)
    k = pkg.Constant(1.0)
    forecast = eng.predict_long_series_batch
    band = lambda series, queries, nodes, noises, sidx, **kw: eng.predict_quantile_long_series_batch(
        series, queries, nodes, noises, sidx, kw.pop("weights", np.full(len(nodes), 1.0 / max(1, len(nodes)))), 0.5, **kw)
    for call in (forecast, band):
        with pytest.raises(ValueError, match="series 1 has 513 points.*LONG_SERIES_MAX_N"):
            call([ok, (np.zeros(N + 1), np.zeros(N + 1))], [q, q], [k], [0.1], [0])
        with pytest.raises(ValueError, match="series 0"):
            call([(np.zeros(4), np.zeros(5))], [q], [k], [0.1], [0])
        with pytest.raises(ValueError, match="one noise per particle"):
            call([ok], [q], [k, k], [0.1], [0, 0])
        with pytest.raises(ValueError, match="one series index per particle"):
            call([ok], [q], [k, k], [0.1, 0.1], [0], all_long=True)
        with pytest.raises(ValueError, match="one vector of query times per series"):
            call([ok, ok], [q], [k], [0.1], [0])
        with pytest.raises(ValueError, match="series 0: the query times must be a vector"):
            call([ok], [np.zeros((2, 2))], [k], [0.1], [0])
        # (the band broadcasts noise_pred with np.broadcast_to, as predict_quantile_series_batch does: NumPy's own message)
        with pytest.raises(ValueError, match="one noise_pred per particle|could not be broadcast"):
            call([ok], [q], [k, k], [0.1, 0.1], [0, 0], noise_pred=np.zeros(3))
    with pytest.raises(ValueError, match="weights has shape"):
        band([ok], [q], [k, k], [0.1, 0.1], [0, 0], weights=np.ones(3))
    with pytest.raises(ValueError, match="y_transforms has shape"):
        band([ok], [q], [k], [0.1], [0], y_transforms=np.ones((2, 2)))
    with pytest.raises(ValueError, match="max_n must be"):
        pkg.predict_quantile_series(eng, [ok], [q], [k], [0.1], [0], [0.0], 0.5, max_n=300)
    with pytest.raises(ValueError, match="series 0 has 513 points"):
        pkg.predict_quantile_series(eng, [(np.zeros(N + 1), np.zeros(N + 1))], [q], [k], [0.1], [0], [0.0], 0.5, max_n=N)


def test_lds_map_twin_agrees_with_the_header():
    args = (ROOT / "autogp.jl_amd" / "csrc" / "agp_args.hpp").read_text()
    const = lambda name: re.search(r"constexpr int %s = ([^;]+);" % name, args).group(1).strip()
    assert int(const("LONG_SERIES_MAX_N")) == LP.LONG_SERIES_MAX_N == 512
    assert int(const("LONG_PRED_C")) == LP.LONG_PRED_C
    assert const("LONG_PRED_QSLOT") == "LONG_SERIES_MAX_N"
    assert const("LONG_PRED_SIG_STRIDE") == "LONG_PRED_QSLOT + 4 * LONG_PRED_C * 16"
    assert LP.LONG_PRED_SIG_STRIDE == 512 + 64 * LP.LONG_PRED_C and LP.ROUND == 64 * LP.LONG_PRED_C <= 32 * 16
    # the map itself: the value kernel's offsets (m.o_sig from long_series_lds with no table), tables of the predictive stride
    assert re.search(r"LongSeriesLds m = long_series_lds\(n, n_ops, n_prm, 0\);\s*m\.total = m\.o_sig \+ n_cp \* LONG_PRED_SIG_STRIDE;", args)
    assert re.search(r"m\.o_dblk = 256; m\.o_tpt = 512; m\.o_rvec = m\.o_tpt \+ m\.np; m\.o_avec = m\.o_rvec \+ m\.np; "
                     r"m\.o_ldg = m\.o_avec \+ m\.np;\s*m\.o_etab = m\.o_ldg \+ m\.np;\s*m\.o_prm = m\.o_etab \+ 128;", args)
    assert re.search(r"long_series_pred_ws_blocks\(int nb\) \{ return long_series_ws_blocks\(nb \+ 4 \* LONG_PRED_C\) \+ nb; \}", args)
    assert LP.long_series_pred_ws_blocks(32) == 40 * 41 // 2 + 32 == 852
    # ten ChangePoint nodes at 512 points fit — the value entry's documented capacity — and two such workgroups share a CU
    assert LP.cp_chain_fits(10, 512)
    assert 2 * 8 * LP.long_series_pred_lds_total(512, 21, 31, 10) <= 160 * 1024
    k_fit = max(k for k in range(1, 60) if LP.cp_chain_fits(k, 512))
    assert k_fit == 27 and not LP.cp_chain_fits(k_fit + 1, 512)
    # a table-free program's map is the value kernel's
    assert LP.long_series_pred_lds_total(442, 5, 7, 0) == LP.long_series_lds_total(442, 5, 7, 0)


TWIN_SHAPES = [(n, m) for n in (1, 17, 177, 257) for m in (1, 17, 65)] + [(33, LP.ROUND + 17)]


def twin_case(pkg, n, m):
    rng = np.random.default_rng(1000 * n + m)
    ts_full, xs_full = pkg.prior.synthetic_series(512, seed=500 + n, shuffle=True)
    ts, xs = ts_full[:n].copy(), xs_full[:n].copy()
    tq = SP.queries_for(ts_full, ts, m)
    nodes, noises = pkg.prior.sample_particles(rng, 2, max_depth=3)
    nodes = list(nodes) + [pkg.ChangePoint(pkg.SquaredExponential(0.3, 0.8), pkg.Periodic(0.7, 0.3, 0.9) + pkg.Linear(0.2, 0.3, 0.4),
                                           float(np.median(ts_full)), 0.05)]
    return ts, xs, tq, nodes, list(noises) + [0.1]


@pytest.mark.parametrize("n,m", TWIN_SHAPES)
def test_stage_p_twin_against_oracle(pkg, n, m):
    ts, xs, tq, nodes, noises = twin_case(pkg, n, m)
    worst = 0.0
    for nd, nz in zip(nodes, noises):
        mu, cov = O.predict_mvn(nd.to_tuple(), float(nz), ts, xs, tq)
        var = np.diag(cov)
        assert np.isfinite(mu).all() and np.isfinite(var).all()
        mean_t, var_t = LP.long_series_predict_blocks(nd.to_tuple(), float(nz), ts, xs, tq)
        worst = max(worst, np.abs(mean_t - mu).max() / max(1.0, np.abs(mu).max()), np.abs(var_t - var).max() / max(1.0, np.abs(var).max()))
        assert SP.close(mean_t, mu, TWIN_TOL) and SP.close(var_t, var, TWIN_TOL), (n, m, nd.to_tuple())
    print(f"stage P twin at n = {n}, m = {m}: worst |d| / max(1, max|ref|) = {worst:.3e}")
    # another noise_pred moves the variance alone
    nd, nz = nodes[0], float(noises[0])
    m0, v0 = LP.long_series_predict_blocks(nd.to_tuple(), nz, ts, xs, tq)
    m1, v1 = LP.long_series_predict_blocks(nd.to_tuple(), nz, ts, xs, tq, noise_pred=nz + 0.375)
    assert np.array_equal(m0, m1) and np.allclose(v1 - v0, 0.375, rtol=0, atol=1e-12)


@pytest.mark.parametrize("fault,n,m", [("neighbour_W", 177, 17), ("padding_weight", 177, 17), ("padding_weight", 17, 65),
                                       ("stale_scratch", 33, LP.ROUND + 17)])
def test_planted_faults_are_caught(pkg, fault, n, m):
    """each mistake the twin's structure guards against shows at the twin's tolerance, on every particle of the shape's case"""
    ts, xs, tq, nodes, noises = twin_case(pkg, n, m)
    for nd, nz in zip(nodes, noises):
        mu, cov = O.predict_mvn(nd.to_tuple(), float(nz), ts, xs, tq)
        good = LP.long_series_predict_blocks(nd.to_tuple(), float(nz), ts, xs, tq)
        assert SP.close(good[0], mu, TWIN_TOL) and SP.close(good[1], np.diag(cov), TWIN_TOL)
        bad = LP.long_series_predict_blocks(nd.to_tuple(), float(nz), ts, xs, tq, fault=fault)
        assert not (SP.close(bad[0], mu, TWIN_TOL) and SP.close(bad[1], np.diag(cov), TWIN_TOL)), (fault, nd.to_tuple())
    if fault == "stale_scratch":      # the fault lives in the rounds after the first: a single round does not show it
        ts, xs, tq, nodes, noises = twin_case(pkg, n, LP.ROUND)
        a = LP.long_series_predict_blocks(nodes[0].to_tuple(), float(noises[0]), ts, xs, tq)
        b = LP.long_series_predict_blocks(nodes[0].to_tuple(), float(noises[0]), ts, xs, tq, fault=fault)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_ragged_case_is_what_the_gpu_tests_expect():
    series, queries, nodes, noises, sidx, ref_mean, ref_var, ref_lp = LP.ragged_case()
    assert [len(t) for t, _ in series] == [0, 1, 2, 15, 16, 17, 33, 176, 177, 192, 193, 255, 256, 257, 442, 512]
    assert [len(q) for q in queries] == [5, 0, 1, 15, 16, 17, 33, 12, 65, 16, 529, 36, 1, 129, 36, 257]
    assert len(nodes) == 64 and all(np.isfinite(a).all() for a in ref_mean + ref_var)
    assert min(v.min() for v in ref_var if v.size) > 0.009
    assert (529 + 15) // 16 == 34 > 32
    s = 14                                                       # 442 points, 36 queries: one ON a training time, one between two
    assert queries[s][0] == series[s][0][0] and queries[s][1] == 0.5 * (series[s][0][0] + series[s][0][1])
    # the twin on the long series of the case, first particle each
    for s in (8, 10, 14):
        p = int(np.flatnonzero(sidx == s)[0])
        mean_t, var_t = LP.long_series_predict_blocks(nodes[p].to_tuple(), float(noises[p]), *series[s], queries[s])
        assert SP.close(mean_t, ref_mean[p], TWIN_TOL) and SP.close(var_t, ref_var[p], TWIN_TOL), s
