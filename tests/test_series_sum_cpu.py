"""CPU tests of the many-short-series decomposition entry (agp_predict_sum_series_batch): its declaration, export, documentation and
bindings; the kernel's coded-row algorithm restated in NumPy (tests/_series_sum_ref.py) against oracle.infer_gp_sum; the LDS need
with the selector tables counted, as the header quotes it; the shared ragged case; and the Python wrappers' layout and argument
checks against a stub library."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _series_sum_ref as R
import _sum_decomposition_ref as SD
from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent
SYM = "agp_predict_sum_series_batch"


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert SYM in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint %s\s*\(" % SYM, hdr)
    assert SYM in (ROOT / "INTEGRATION.md").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and SYM in seen
    assert hasattr(pkg.GPEngine, "predict_sum_series_batch") and hasattr(pkg, "predict_sum_series") and hasattr(pkg, "SeriesSums")
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    assert re.search(r'"\nfunction predict_sum_series_batch\(', shim)


def parts(G, M):
    """M component kernels: a ChangePoint among them, a sentinel Constant(0) at M = 3"""
    all_ = [G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Periodic(0.5, 0.1, 0.8) + G.WhiteNoise(0.1), 0.45, 0.05),
            G.Linear(0.3, 0.2, 0.7) * G.SquaredExponential(0.25, 0.8) + G.Constant(0.1),
            G.Constant(0)]
    return [t.to_tuple() for t in all_[:M]]


@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("n,m", [(1, 5), (15, 6), (16, 5), (17, 6), (17, 22), (33, 16), (176, 6)])
def test_coded_rows_against_the_oracle(pkg, n, m, M):
    """row order, codes, selector masks at training and query slots, addends, the masks past n and past (M + 1) m, the read-out:
    raw means, variances and quantiles within 1e-8 max(1, max|ref|) of the oracle's; m = 5 puts every code into one block of 16
    rows, m = 6 makes a component straddle two, m = 22 gives a second pass"""
    ts, xs = pkg.prior.synthetic_series(256, seed=60 + n, shuffle=True)
    tq = R.RP.queries_for(ts, ts[:n], m)
    ts, xs = ts[:n].copy(), xs[:n].copy()
    trees = parts(pkg, M)
    for noise, npred, yt in ((0.1, None, (1.0, 0.0)), (0.05, 0.0, (-0.8, 0.4)), (0.2, 0.3, (2.5, -1.0))):
        ref = R.oracle_rows(trees, noise, ts, xs, tq, noise_pred=npred, y_transform=yt, q=R.Q)
        got = R.series_sum_rows(trees, noise, ts, xs, tq, noise_pred=npred, y_transform=yt, q=R.Q)
        assert got[3] == 0
        for a, r, what in zip(got, ref, ("mean", "var", "x")):
            assert R.close(a, r), (n, m, M, what, np.abs(a - r).max())
    # ... and predict_mvn_sum's restatement agrees on the means (the reference's own row order F_1 .. F_M, X)
    comps, idx = SD.predict_mvn_sum([trees], [0.1], ts, xs, tq, y_transform=(2.5, -1.0))
    got = R.series_sum_rows(trees, 0.1, ts, xs, tq, y_transform=(2.5, -1.0))
    assert R.close(got[0], comps[0][0]) and idx["Y"] == slice(M * m, (M + 1) * m)


def test_coded_rows_prior_of_an_empty_series(pkg):
    """no block: means 0 (raw: -b / a, and 0 on F_1), var_i = K_i(t, t) + 1e-8, X also + noise_pred"""
    trees = parts(pkg, 2)
    tq = np.array([0.1, 0.45, 0.45, 0.9, 1.3])
    a, b = 2.0, 0.5
    mr, vr, x, info = R.series_sum_rows(trees, 0.1, np.zeros(0), np.zeros(0), tq, noise_pred=0.2, y_transform=(a, b), q=(0.5,))
    k = [np.diag(O.eval_cov(t, tq)) for t in trees]
    assert info == 0
    assert (mr[:5] == (0.0 - b) / a + b / a).all() and (mr[5:] == (0.0 - b) / a).all()
    assert np.array_equal(vr, (1.0 / (a * a)) * np.concatenate([k[0] + 1e-8, k[1] + 1e-8, (k[0] + k[1]) + (1e-8 + 0.2)]))
    assert np.array_equal(x[:, 0], mr)                   # the median: fma(sd, 0, mean)


def test_selector_tables_and_sentinel_rows(pkg):
    """SEL_i is 1 at the observable and at its own component only; a Constant(0) sentinel component therefore has scaled mean
    exactly 0 and variance exactly the jitter, whatever the other components are"""
    assert R.sel_table([0, 1, 2, 3, 0], 2).tolist() == [1.0, 0.0, 1.0, 0.0, 1.0]
    ts, xs = pkg.prior.synthetic_series(64, seed=5, shuffle=True)
    tq = R.RP.queries_for(ts, ts[:33], 6)
    trees = [parts(pkg, 1)[0], ("C", 0.0)]
    mr, vr, _, info = R.series_sum_rows(trees, 0.1, ts[:33], xs[:33], tq, noise_pred=0.0)
    assert info == 0 and (mr[6:12] == 0.0).all() and (vr[6:12] == 1e-8).all()
    assert np.abs(mr[:6] - mr[12:]).max() < 1e-12        # ... and X = F_1 then


def test_row_level_info_rule(pkg):
    """a transform that overflows a raw mean: info = n + g + 1 of the FIRST such row, NaN everywhere"""
    ts, xs = pkg.prior.synthetic_series(64, seed=6, shuffle=True)
    tq = R.RP.queries_for(ts, ts[:17], 6)
    trees = parts(pkg, 2)
    mr, vr, x, info = R.series_sum_rows(trees, 0.1, ts[:17], xs[:17], tq, y_transform=(1e-308, 1e300), q=(0.5,))
    # (mean - b) / a overflows on every row; on the F_1 rows + b / a = +inf gives NaN: not finite either way -> row 0
    assert info == 17 + 1 and np.isnan(mr).all() and np.isnan(vr).all() and np.isnan(x).all()


def test_lds_need_matches_the_header(pkg):
    """the limit the header quotes at the cap beside M = 2 selectors is the one series_lds gives"""
    N = pkg.SERIES_MAX_N

    def composite(k):
        """k ChangePoint nodes over k + 1 Constant leaves as F_1, a Constant as F_2"""
        t = ("C", 1.0)
        for _ in range(k):
            t = ("CP", t, ("C", 1.0), 0.5, 0.1)
        return [t, ("C", 1.0)]
    fits = lambda k: R.series_sum_lds_bytes(N, composite(k)) <= R.R.LDS_BYTES
    fit = max(k for k in range(0, 40) if fits(k))
    assert fits(fit) and not fits(fit + 1)
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    doc = hdr[hdr.index("DECOMPOSITIONS of many short series"):hdr.index("int %s(" % SYM)]
    m = re.search(r"M = 2 a composite with (\d+) ChangePoint nodes \((\d+) nodes, (\d+) parameters,\s*\*?\s*(\d+) tables: ([\d ]+) of "
                  r"([\d ]+) bytes\) fits and one with (\d+) \(([\d ]+) bytes\) does not; the predictive entry's limit there is (\d+)", doc)
    assert m, "the header states the limit"
    num = lambda s: int(s.replace(" ", ""))
    n_ops, n_prm, n_cp = R.composite_sizes(composite(fit))
    assert [num(g) for g in m.groups()] == [fit, n_ops, n_prm, n_cp, R.series_sum_lds_bytes(N, composite(fit)), R.R.LDS_BYTES, fit + 1,
                                            R.series_sum_lds_bytes(N, composite(fit + 1)),
                                            max(k for k in range(1, 40) if R.RP.cp_chain_fits(k, N))]
    assert n_cp == fit + 2                               # the selectors take a table each: two fewer ChangePoint nodes fit
    # one map, the predictive kernel's: the need is series_pred_lds of the composite's own sizes
    assert R.series_sum_lds_bytes(N, composite(3)) == 8 * R.RP.series_pred_lds_total(N, *R.composite_sizes(composite(3)))
    src = (ROOT / "autogp.jl_amd" / "csrc" / "agp_series.hip").read_text()
    assert "mode == SeriesMode::prediction || mode == SeriesMode::sum ? series_pred_lds(" in src


def test_ragged_case_is_the_stated_one(pkg):
    """the GPU test's shared input: the stated lengths and query counts, a training time and a midpoint among the queries, every
    composite inside the kernel's LDS, the oracle finite everywhere, the smallest scaled variance the jitter of a sentinel"""
    series, queries, splits, noises, sidx, yts, ref_mean, ref_var, ref_x = R.ragged_case()
    assert [len(t) for t, _ in series] == list(R.RAGGED_N) and [len(q) for q in queries] == list(R.RAGGED_M)
    assert len(splits) == 4 * 9 + 2 * 3 and all(len(sp) == 2 for sp in splits)
    for (ts, _), q in zip(series, queries):
        if len(q) >= 3 and len(ts) >= 2:
            assert q[0] == ts[0] and q[1] == 0.5 * (ts[0] + ts[1])
    need = [R.series_sum_lds_bytes(len(series[s][0]), [c.to_tuple() for c in sp]) for sp, s in zip(splits, sidx)]
    assert max(need) <= R.R.LDS_BYTES
    assert all(np.isfinite(a).all() for a in ref_mean + ref_var + ref_x)
    assert sum(1 for sp in splits for c in sp if c.to_tuple() == ("C", 0.0)) >= 10
    scaled_min = min((v * yts[s][0] ** 2).min() for v, s in zip(ref_var, sidx) if v.size)
    assert abs(scaled_min - 1e-8) <= 1e-20
    for sp, s, m_, x_ in zip(splits, sidx, ref_mean, ref_x):
        assert m_.shape == (3 * len(queries[s]),) and x_.shape == (3 * len(queries[s]), 3)
    # the hand-built particles: a ChangePoint with two non-trivial parts, and WhiteNoise queried at a training time
    for s in (6, 7, 8):
        mine = [sp for sp, t in zip(splits, sidx) if t == s][4:]
        assert len(mine) == 2
        assert all(c.to_tuple() != ("C", 0.0) for c in mine[0]) and any("CP" in repr(c.to_tuple()) for c in mine[0])
        assert mine[1][0].to_tuple()[0] == "WN" and queries[s][0] == series[s][0][0]
    for sp, nz, s in zip(splits, noises, sidx):          # every training covariance factors: info == 0 is the only right answer
        if len(series[s][0]):
            K = sum(O.eval_cov(c.to_tuple(), series[s][0]) for c in sp) + float(nz) * np.eye(len(series[s][0]))
            np.linalg.cholesky(K)


# ---- the Python wrappers against a stub library ----------------------------------------------------------------------------------

class _Stub:
    """stands in for the library: records the call and fills the outputs the way the entry lays them out — row r of particle p
    holds 1000 p + r, its variance the negative, quantile k of it + k / 10"""

    def __init__(self):
        self.calls = []

    def agp_predict_sum_series_batch(self, ctx, S, pt_off, ts, xs, q_off, ts_pred, P, M, series, op_off, ops, prm_off, prm, noise,
                                     noise_pred, slope, icpt, q, nq, mean, var, x, out_off, lp, info):
        qo = [q_off[s] for s in range(S + 1)]
        off = 0
        for p in range(P):
            out_off[p] = off
            rows = (M + 1) * (qo[series[p] + 1] - qo[series[p]])
            for r in range(rows):
                mean[off + r] = 1000.0 * p + r
                if var:
                    var[off + r] = -(1000.0 * p + r)
                for k in range(nq):
                    x[(off + r) * nq + k] = 1000.0 * p + r + k / 10.0
            off += rows
            if lp:
                lp[p] = -float(p)
            info[p] = 0
        out_off[P] = off
        self.calls.append(dict(S=S, P=P, M=M, nq=nq, n_comp_off=[op_off[i] for i in range(P * M + 1)],
                               noise_pred=None if not noise_pred else [noise_pred[p] for p in range(P)],
                               slope=None if not slope else [slope[s] for s in range(S)],
                               icpt=None if not icpt else [icpt[s] for s in range(S)],
                               q=[q[k] for k in range(nq)] if nq else None, has_var=bool(var), has_x=bool(x), has_lp=bool(lp)))
        return 0


def _engine(pkg, lib):
    eng = object.__new__(pkg.GPEngine)
    eng._lib = lib; eng._ctx = None
    return eng


def _two_series(pkg):
    ok = (np.linspace(0, 1, 5), np.zeros(5))
    series = [ok, (np.linspace(0, 1, 7), np.ones(7))]
    queries = [np.array([1.1, 1.2]), np.array([1.5, 1.6, 1.7])]
    G = pkg
    splits = [(G.SquaredExponential(0.3, 0.8), G.Constant(0)), (G.Periodic(0.5, 0.2, 0.7) + G.Linear(0.1, 0.2, 0.3), G.WhiteNoise(0.1)),
              (G.Constant(0), G.Linear(0.1, 0.2, 0.3))]
    return series, queries, splits, [0.1, 0.2, 0.3], [1, 0, 1]


def test_wrapper_layout_with_a_stub_library(pkg):
    series, queries, splits, noises, sidx = _two_series(pkg)
    lib = _Stub()
    eng = _engine(pkg, lib)
    r = eng.predict_sum_series_batch(series, queries, splits, noises, sidx, q=(0.025, 0.5, 0.975), y_transforms=[(2.0, 0.5), (-1.0, 0.0)],
                                     noise_pred=0.0, want_var=True, want_logpdf=True)
    c = lib.calls[-1]
    assert (c["S"], c["P"], c["M"], c["nq"]) == (2, 3, 2, 3) and len(c["n_comp_off"]) == 7 and c["n_comp_off"][-1] == 8
    assert c["noise_pred"] == [0.0] * 3 and c["slope"] == [2.0, -1.0] and c["icpt"] == [0.5, 0.0] and c["q"] == [0.025, 0.5, 0.975]
    assert c["has_var"] and c["has_x"] and c["has_lp"]
    assert isinstance(r, pkg.SeriesSums)
    assert [len(m) for m in r.mean] == [9, 6, 9] and [v.shape for v in r.x] == [(9, 3), (6, 3), (9, 3)]
    for p in range(3):
        rows = np.arange(len(r.mean[p]))
        assert np.array_equal(r.mean[p], 1000.0 * p + rows) and np.array_equal(r.var[p], -(1000.0 * p + rows))
        assert np.array_equal(r.x[p], (1000.0 * p + rows)[:, None] + np.arange(3)[None, :] / 10.0)
    assert r.logpdf.tolist() == [0.0, -1.0, -2.0] and r.info.tolist() == [0, 0, 0]
    assert r.mean[0].base is r.mean[2].base              # views cut from one particle-major array
    # no quantiles, no variances, no value: NULL pointers travel, x[p] is (rows, 0)
    r = eng.predict_sum_series_batch(series, queries, splits, noises, sidx)
    c = lib.calls[-1]
    assert c["nq"] == 0 and not c["has_var"] and not c["has_x"] and not c["has_lp"] and c["slope"] is None and c["noise_pred"] is None
    assert r.var is None and r.logpdf is None and [v.shape for v in r.x] == [(9, 0), (6, 0), (9, 0)]
    # the components encoded beforehand: the same call
    progs = pkg.encode_batch([c for sp in splits for c in sp])
    r2 = eng.predict_sum_series_batch(series, queries, None, noises, sidx, programs=progs)
    assert lib.calls[-1] == c and [m.tolist() for m in r2.mean] == [m.tolist() for m in r.mean]
    with pytest.raises(ValueError, match="same number"):
        eng.predict_sum_series_batch(series, queries, None, noises[:2] + [0.1, 0.2], sidx + [0], programs=progs)


def test_predict_sum_series_columns_with_a_stub_library(pkg):
    """one dict per series in predict_sum's row order — per particle of the series component 0 = Y (the LAST block of rows), then 1,
    2 — with the weights normalised within each series"""
    series, queries, splits, noises, sidx = _two_series(pkg)
    nodes = [a + b for a, b in splits]                   # (split again inside: the stub ignores the programs)
    lib = _Stub()
    out = pkg.predict_sum_series(_engine(pkg, lib), series, queries, nodes, noises, sidx, [0.0, -3.0, np.log(3.0)], pkg.Periodic,
                                 quantiles=(0.5,))
    assert lib.calls[-1]["M"] == 2 and len(out) == 2
    d0, d1 = out
    assert d0["ds"].tolist() == list(queries[0]) * 3 and d0["particle"].tolist() == [1] * 6 and d0["weight"].tolist() == [1.0] * 6
    assert d0["component"].tolist() == [0, 0, 1, 1, 2, 2]
    assert d0["y_mean"].tolist() == [1004.0, 1005.0, 1000.0, 1001.0, 1002.0, 1003.0]          # particle 1's rows: Y = rows 4, 5
    assert d0["y_0.5"].tolist() == d0["y_mean"].tolist()
    assert d1["particle"].tolist() == [1] * 9 + [2] * 9 and d1["component"].tolist() == ([0] * 3 + [1] * 3 + [2] * 3) * 2
    assert np.allclose(d1["weight"], [0.25] * 9 + [0.75] * 9)
    assert d1["y_mean"].tolist() == [6.0, 7.0, 8.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0] + [2006.0, 2007.0, 2008.0, 2000.0, 2001.0, 2002.0,
                                                                                    2003.0, 2004.0, 2005.0]


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_python_side_validation_runs_before_any_library_call(pkg):
    series, queries, splits, noises, sidx = _two_series(pkg)
    entry = _engine(pkg, _NoLibrary()).predict_sum_series_batch
    with pytest.raises(ValueError, match="same number"):
        entry(series, queries, [splits[0], splits[1][:1], splits[2]], noises, sidx)
    with pytest.raises(ValueError, match="same number"):
        entry(series, queries, [(), (), ()], noises, sidx)
    with pytest.raises(ValueError, match="one vector of query times per series"):
        entry(series, queries[:1], splits, noises, sidx)
    with pytest.raises(ValueError, match="one noise per particle"):
        entry(series, queries, splits, noises[:2], sidx)
    with pytest.raises(ValueError, match="one series index per particle"):
        entry(series, queries, splits, noises, sidx[:2])
    with pytest.raises(ValueError, match=r"y_transforms has shape \(3, 2\), expected \(2, 2\)"):
        entry(series, queries, splits, noises, sidx, y_transforms=[(1.0, 0.0)] * 3)
    with pytest.raises(ValueError, match="one noise_pred per particle"):
        entry(series, queries, splits, noises, sidx, noise_pred=[[0.1, 0.2, 0.3]])
    n = pkg.SERIES_MAX_N + 1
    with pytest.raises(ValueError, match="series 1 has %d points" % n):
        entry([series[0], (np.zeros(n), np.zeros(n))], queries, splits, noises, sidx)
