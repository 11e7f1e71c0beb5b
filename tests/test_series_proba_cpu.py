"""CPU tests of the many-short-series held-out entry (agp_predict_logpdf_series_batch): its declaration, export, documentation and
bindings; the kernel's index algebra restated in NumPy (tests/_series_proba_ref.py) against the reference restatement of the
predictive log-density (tests/_pred_logpdf_ref.py) at |lp - ref| <= 1e-8 S; the info rule on the joint points; the chain rule of the
per-point terms; the Python wrappers' transform and slope plumbing with the library and the engine stubbed; and the LDS need at the
joint length."""
import ctypes as C
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _pred_logpdf_ref as PR
import _series_cases as SC
import _series_proba_ref as R

ROOT = Path(__file__).resolve().parent.parent
SYM = "agp_predict_logpdf_series_batch"
TOL = 1e-8


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert SYM in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint %s\s*\(" % SYM, hdr)
    assert SYM in (ROOT / "INTEGRATION.md").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and SYM in seen
    assert hasattr(pkg.GPEngine, "predict_logpdf_series_batch") and hasattr(pkg, "predict_proba_series") and hasattr(pkg, "pack_heldout")
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    assert re.search(r'"\nfunction predict_proba_series_batch\(', shim)      # the docstring sits directly above its own definition
    assert "predict_proba_series_batch" in (ROOT / "autogp.jl_amd" / "julia" / "test" / "runtests.jl").read_text()
    kern = (ROOT / "autogp.jl_amd" / "csrc" / "agp_series_kernel.hpp").read_text()
    assert "k_series_predict_logpdf" in kern.split("#pragma once")[0]      # the header comment describes the instantiation


def trees(G):
    return [G.SquaredExponential(0.3, 0.8),
            G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Periodic(0.5, 0.1, 0.8) + G.WhiteNoise(0.1), 0.45, 0.05),
            G.Linear(0.3, 0.2, 0.7) * G.SquaredExponential(0.25, 0.8) + G.Constant(0.1)]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%d+%d" % s)
def test_block_algorithm_against_the_reference(pkg, shape):
    """joint points, packed blocks, identity padding, the two-noise diagonal and the row mask [n, N): the log-density within 1e-8 S
    of the m x m reference, the terms summing to it; every query kind and noise_pred None / smaller / larger at every shape"""
    n, m = shape
    rng = np.random.default_rng(1000 * n + m)
    ts, xs = pkg.prior.synthetic_series(256, seed=60 + n, shuffle=True)
    ts, xs = ts[:n].copy(), xs[:n].copy()
    y = 0.5 * rng.standard_normal(m)
    for i, (node, noise, noise_pred) in enumerate(zip(trees(pkg), (0.1, 0.05, 0.2), (None, 0.02, 0.3))):
        tq = R.queries(R.QUERY_KINDS[i], ts, m, rng)
        lp, terms, info = R.series_proba_blocks(node.to_tuple(), noise, ts, xs, tq, y, noise_pred=noise_pred)
        ref, S = PR.reference(node.to_tuple(), noise, ts, xs, tq, y, noise_pred=noise_pred)
        assert info == 0 and terms.shape == (m,)
        if m == 0:
            assert lp == 0.0 and ref == 0.0
            continue
        assert abs(lp - ref) <= TOL * S, (shape, i, lp, ref, S)
        assert abs(terms.sum() - lp) <= 1e-12 * S


def test_slope_enters_through_the_jacobian_alone(pkg):
    node = trees(pkg)[1]
    ts, xs = pkg.prior.synthetic_series(40, seed=3)
    tq = np.array([0.2, ts[5], 1.1]); y = np.array([0.1, -0.3, 0.2])
    lp1, t1, _ = R.series_proba_blocks(node.to_tuple(), 0.1, ts, xs, tq, y)
    lp2, t2, _ = R.series_proba_blocks(node.to_tuple(), 0.1, ts, xs, tq, y, slope=-2.5)
    assert abs(lp2 - (lp1 + 3 * math.log(2.5))) <= 1e-13 * abs(lp1) and np.allclose(t2 - t1, math.log(2.5), rtol=0, atol=1e-14)


def test_terms_are_the_prequential_scores(pkg):
    """the partial sum over the first j terms is the log-density of the first j held-out points: both sides of every block boundary
    the split creates at (17, 40)"""
    node = trees(pkg)[2]
    ts, xs = pkg.prior.synthetic_series(256, seed=8, shuffle=True)
    n, m = 17, 40
    rng = np.random.default_rng(2)
    tq = rng.random(m); y = 0.5 * rng.standard_normal(m)
    lp, terms, _ = R.series_proba_blocks(node.to_tuple(), 0.1, ts[:n], xs[:n], tq, y, noise_pred=0.04)
    for j in (1, 14, 15, 16, 30, 31, 32, 39, 40):        # joint positions 17 + j around 32 and 48
        ref, S = PR.reference(node.to_tuple(), 0.1, ts[:n], xs[:n], tq[:j], y[:j], noise_pred=0.04)
        lpj, _, _ = R.series_proba_blocks(node.to_tuple(), 0.1, ts[:n], xs[:n], tq[:j], y[:j], noise_pred=0.04)
        assert abs(terms[:j].sum() - ref) <= TOL * S and abs(lpj - ref) <= TOL * S, j


INFO_N = 40
INFO_POSITIONS = (1, 16, 17, INFO_N, INFO_N + 1, INFO_N + 16, SC.N_CAP)


def test_info_is_the_first_bad_pivot_of_the_joint_factor(pkg):
    """changepoint_particle on the JOINT times (the first INFO_N of CP_TS train, the rest are queries), both noises CP_NOISE: the
    first failing minor is the chosen joint position — 1 .. n when K11 fails, n + k when minor k of the predictive covariance does"""
    ts, tq = SC.CP_TS[:INFO_N], SC.CP_TS[INFO_N:]
    xs = np.zeros(INFO_N); y = np.zeros(len(tq))
    for pos in INFO_POSITIONS:
        node = SC.changepoint_particle(pkg, pos - 1)
        K = PR.O.compute_cov_matrix_vectorized(node.to_tuple(), SC.CP_NOISE, SC.CP_TS)
        assert SC.first_bad_minor(K) == pos
        lp, terms, info = R.series_proba_blocks(node.to_tuple(), SC.CP_NOISE, ts, xs, tq, y)
        assert info == pos and math.isnan(lp) and np.isnan(terms).all() and terms.shape == (len(tq),)


def test_lds_need_is_the_value_kernels_at_the_joint_length(pkg):
    import _series_grad_ref as G
    N = pkg.SERIES_MAX_N
    assert N == R.N_CAP
    for n, m in ((0, N), (1, N - 1), (100, 76), (N - 1, 1)):
        assert R.series_proba_lds_total(n, m, 5, 7, 2) == G.series_lds_total(N, 5, 7, 2)
        fit = max(k for k in range(1, 40) if R.cp_chain_fits(k, n, m))
        assert fit == max(k for k in range(1, 40) if G.cp_chain_fits(k, N, grad=False))
    assert R.cp_chain_fits(fit + 8, 60, 40)
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    doc = hdr[hdr.index("HELD-OUT SCORES of many short series"):hdr.index("int %s(" % SYM)]
    mt = re.search(r"a chain of (\d+) ChangePoint nodes fits and one of (\d+) does not", doc)
    assert mt and [int(x) for x in mt.groups()] == [fit, fit + 1]
    src = (ROOT / "autogp.jl_amd" / "csrc" / "agp_series.hip").read_text()
    assert "SeriesMode::held_out" in src


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def _stub_engine(pkg, lib):
    eng = object.__new__(pkg.GPEngine)
    eng._lib = lib; eng._ctx = None
    return eng


def test_python_side_validation_runs_before_any_library_call(pkg):
    good = pkg.SquaredExponential(0.3, 0.8)
    ok = (np.linspace(0, 1, 5), np.zeros(5))
    q = np.array([1.1, 1.2]); y = np.array([0.1, 0.2])
    entry = _stub_engine(pkg, _NoLibrary()).predict_logpdf_series_batch
    with pytest.raises(ValueError, match="one vector of query times per series"):
        entry([ok, ok], [q], [y, y], [good], [0.1], [0])
    with pytest.raises(ValueError, match="one vector of held-out values per series"):
        entry([ok, ok], [q, q], [y], [good], [0.1], [0])
    with pytest.raises(ValueError, match="series 1: 2 held-out values required"):
        entry([ok, ok], [q, q], [y, y[:1]], [good], [0.1], [0])
    with pytest.raises(ValueError, match="series 0: 2 held-out values required"):
        entry([ok], [q], [y[None, :]], [good], [0.1], [0])
    with pytest.raises(ValueError, match=r"y_transforms has shape \(2,\)"):
        entry([ok], [q], [y], [good], [0.1], [0], y_transforms=(1.0, 0.0))
    with pytest.raises(ValueError, match="weights has shape"):
        entry([ok], [q], [y], [good], [0.1], [0], weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="one noise_pred per particle"):
        entry([ok], [q], [y], [good, good], [0.1, 0.1], [0, 0], noise_pred=[[0.1, 0.1]])
    with pytest.raises(ValueError, match="one noise per particle"):
        entry([ok], [q], [y], [good, good], [0.1], [0, 0])
    # the packer itself; pack_queries keeps its results
    q_off, ts_pred, _ = pkg.pack_queries([q, np.zeros(0), [3.0]], 3)
    y_pred, slope = pkg.pack_heldout([y, [], [4.0]], q_off, [(2.0, 1.0), (1.0, 0.0), (-0.5, 0.25)])
    assert y_pred.tolist() == [1.2, 1.4, -1.75] and slope.tolist() == [2.0, 1.0, -0.5] and y_pred.dtype == np.float64
    y_pred, slope = pkg.pack_heldout([y, [], [4.0]], q_off)
    assert y_pred.tolist() == [0.1, 0.2, 4.0] and slope is None


class _RecordingLibrary:
    """stands in for the library: keeps what the wrapper passes down and answers with recognisable numbers"""
    def __init__(self):
        self.seen = None

    def agp_predict_logpdf_series_batch(self, ctx, S, pt_off, ts, xs, q_off, ts_pred, y_pred, P, series, op_off, ops, prm_off, prm, noise,
                                        noise_pred, y_slope, weights, out_logpdf, out_terms, out_off, out_series_logp, out_info):
        Q = q_off[S]
        m_of = [q_off[series[p] + 1] - q_off[series[p]] for p in range(P)]
        self.seen = dict(S=S, P=P, q_off=[q_off[i] for i in range(S + 1)], y_pred=[y_pred[i] for i in range(Q)],
                         y_slope=None if not y_slope else [y_slope[s] for s in range(S)],
                         weights=None if not weights else [weights[p] for p in range(P)],
                         noise_pred=None if not noise_pred else [noise_pred[p] for p in range(P)],
                         has_terms=bool(out_terms), has_mix=bool(out_series_logp))
        out_off[0] = 0
        for p in range(P):
            out_off[p + 1] = out_off[p] + m_of[p]
            out_logpdf[p] = -10.0 - p
            out_info[p] = 0
        if out_terms:
            for i in range(out_off[P]):
                out_terms[i] = 0.5 * i
        if out_series_logp:
            for s in range(S):
                out_series_logp[s] = 100.0 + s
        return 0


def test_wrapper_scales_the_held_out_values_and_passes_the_slopes(pkg):
    G = pkg
    lib = _RecordingLibrary()
    eng = _stub_engine(pkg, lib)
    s0 = (np.linspace(0, 1, 5), np.zeros(5)); s1 = (np.linspace(0, 1, 3), np.ones(3))
    qs = [np.array([1.1, 1.2]), np.array([1.3, 1.4, 1.5])]
    held = [np.array([0.5, -0.5]), np.array([1.0, 2.0, 3.0])]
    nodes = [G.SquaredExponential(0.3, 0.8), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7)]
    out = eng.predict_logpdf_series_batch([s0, s1], qs, held, nodes, [0.1, 0.2, 0.3], [1, 0, 1], weights=[0.25, 1.0, 0.75],
                                          y_transforms=[(2.0, 1.0), (-2.5, 0.3)], noise_pred=0.05, want_terms=True)
    seen = lib.seen
    assert seen["S"] == 2 and seen["P"] == 3 and seen["q_off"] == [0, 2, 5]
    assert seen["y_pred"] == [2.0 * 0.5 + 1.0, 2.0 * -0.5 + 1.0, -2.5 * 1.0 + 0.3, -2.5 * 2.0 + 0.3, -2.5 * 3.0 + 0.3]
    assert seen["y_slope"] == [2.0, -2.5] and seen["weights"] == [0.25, 1.0, 0.75] and seen["noise_pred"] == [0.05] * 3
    assert seen["has_terms"] and seen["has_mix"]
    assert out.logpdf.tolist() == [-10.0, -11.0, -12.0] and out.info.tolist() == [0, 0, 0] and out.series_logp.tolist() == [100.0, 101.0]
    assert [t.tolist() for t in out.terms] == [[0.0, 0.5, 1.0], [1.5, 2.0], [2.5, 3.0, 3.5]]      # particle-major behind out_off
    # without transforms, weights and terms: NULL slopes, NULL weights and out_series_logp together, NULL out_terms
    out = eng.predict_logpdf_series_batch([s0, s1], qs, held, nodes, [0.1, 0.2, 0.3], [1, 0, 1])
    seen = lib.seen
    assert seen["y_pred"] == [0.5, -0.5, 1.0, 2.0, 3.0] and seen["y_slope"] is None and seen["weights"] is None
    assert seen["noise_pred"] is None and not seen["has_terms"] and not seen["has_mix"]
    assert out.terms is None and out.series_logp is None


class _StubEngine:
    def __init__(self, pkg):
        self.pkg = pkg
        self.kw = None

    def predict_logpdf_series_batch(self, series, queries, heldout, nodes, noises, series_index, **kw):
        self.kw = kw
        P, S = len(nodes), len(series)
        return self.pkg.SeriesScores(-1.0 - np.arange(P), None, 50.0 + np.arange(S), np.zeros(P, dtype=np.int32))


def test_predict_proba_series_columns(pkg):
    """per series the reference's three columns and the mixture's score; weights through pack_series_mixture (softmax inside each
    series), particles of a series need not be adjacent, a series without particles has empty columns"""
    eng = _StubEngine(pkg)
    s = (np.linspace(0, 1, 4), np.zeros(4))
    lw = np.array([0.0, math.log(3.0), 1.0, 0.0])
    out = pkg.predict_proba_series(eng, [s, s, s], [[1.1]] * 3, [[0.2]] * 3, [None] * 4, [0.1] * 4, [2, 0, 0, 2], lw,
                                   y_transforms=[(1.0, 0.0)] * 3, noise_pred=0.01)
    assert len(out) == 3 and all(set(d) == {"particle", "weight", "logp", "mixture_logp"} for d in out)
    assert out[0]["particle"].tolist() == [1, 2] and out[0]["logp"].tolist() == [-2.0, -3.0]
    e = math.exp(1.0)
    assert np.allclose(out[0]["weight"], [3.0 / (3.0 + e), e / (3.0 + e)])
    assert out[2]["particle"].tolist() == [1, 2] and out[2]["logp"].tolist() == [-1.0, -4.0] and np.allclose(out[2]["weight"], [0.5, 0.5])
    assert out[1]["particle"].size == 0 and out[1]["weight"].size == 0 and out[1]["logp"].size == 0
    assert [d["mixture_logp"] for d in out] == [50.0, 51.0, 52.0]
    w = eng.kw["weights"]
    assert abs(w[[1, 2]].sum() - 1.0) < 1e-15 and abs(w[[0, 3]].sum() - 1.0) < 1e-15
    assert eng.kw["noise_pred"] == 0.01 and eng.kw["y_transforms"] == [(1.0, 0.0)] * 3


def test_ragged_case_is_the_stated_one(pkg):
    series, qs, held, nodes, noises, sidx, noise_pred = R.ragged_case()
    assert tuple((len(t), len(q)) for (t, _), q in zip(series, qs)) == R.SHAPES
    assert [len(y) for y in held] == [len(q) for q in qs]
    per = R.N_PRIOR + 10
    assert len(nodes) == per * len(R.SHAPES) and sidx.tolist() == [s for s in range(len(R.SHAPES)) for _ in range(per)]
    assert all(n + m <= R.N_CAP for n, m in R.SHAPES + R.EXTRA_SHAPES)
    blocks = lambda shapes: {-(-(n + m) // 16) for n, m in shapes if m}      # noqa: E731
    assert sorted(blocks(R.SHAPES)) == [1, 2, 3, 5, 9, 11] and sorted(blocks(R.SHAPES) | blocks(R.EXTRA_SHAPES)) == list(range(1, 12))
    assert (noise_pred[::2] < noises[::2]).all() and (noise_pred > 0).all()
    for s, ((ts, _), q) in enumerate(zip(series, qs)):
        if R.QUERY_KINDS[s % 3] == "training" and len(ts):
            assert np.isin(q, ts).all()
        elif R.QUERY_KINDS[s % 3] == "interleaved":
            assert ((q >= 0) & (q <= 1)).all()
    assert all(nd.depth() <= 3 for s in range(len(R.SHAPES)) for nd in nodes[s * per:s * per + R.N_PRIOR])
