"""CPU tests of the long held-out entry (agp_predict_logpdf_long_series_batch): its declaration, export, documentation and Julia
binding; the Python-side refusals; the LDS need at the joint length against the figures the header quotes; and the NumPy restatement
of k_long_series_predict_logpdf (tests/_long_series_proba_ref.py) — left-looking by block columns on the joint points, the read-out over
the query rows, the info rule — against the reference restatement of the predictive log-density (tests/_pred_logpdf_ref.py) on the
ragged case the GPU tests share.
Tolerances: the restatement against the reference |lp - ref| <= 1e-8 S, S the sum of the magnitudes of the terms the log-density is
made of (_pred_logpdf_ref.reference) — the project's for this quantity; sums of the restatement's own numbers in another order: 1e-12 S.
Every particle of the case is factored by the reference (asserted): none is skipped."""
import inspect
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _long_series_cases as LC
import _long_series_predict_ref as LP
import _long_series_proba_ref as LR
import _pred_logpdf_ref as PR
import _series_proba_ref as SPR

ROOT = Path(__file__).resolve().parent.parent
ENTRY = "agp_predict_logpdf_long_series_batch"
TOL = 1e-8


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, protos = CK.check()
    assert problems == []
    assert ENTRY in pkg.EXPORTED_SYMBOLS and ENTRY in doc and ENTRY in seen
    # agp_predict_logpdf_series_batch's parameters, then the trailing flags word
    assert protos[ENTRY] == (protos["agp_predict_logpdf_series_batch"][0], protos["agp_predict_logpdf_series_batch"][1] + ["u32"])
    m = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % ENTRY, re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))      # (comments hold semicolons)
    assert m and re.search(r"uint32_t\s+flags\s*$", m.group(1).strip())
    assert re.search(r'"\nfunction predict_proba_long_series_batch\(', shim)         # docstring directly above its own definition
    sig = inspect.signature(pkg.GPEngine.predict_logpdf_long_series_batch)
    short = inspect.signature(pkg.GPEngine.predict_logpdf_series_batch)
    assert list(sig.parameters) == [*list(short.parameters)[:-2], "all_long", "check", "programs"]
    assert sig.parameters["all_long"].default is False and sig.parameters["check"].default is True
    # the module-level wrapper keeps its defaults: the short entry unless asked
    sig = inspect.signature(pkg.predict_proba_series)
    assert sig.parameters["max_n"].default == pkg.SERIES_MAX_N and sig.parameters["all_long"].default is False
    # the kernel's argument type: the short held-out twin's and the workspace
    args = (ROOT / "autogp.jl_amd" / "csrc" / "agp_args.hpp").read_text()
    assert re.search(r"struct LongSeriesProbaArgs : SeriesProbaArgs \{\s*double\* ws;\s*long long ws_stride;", args)


class NoLibrary:
    """stands where the loaded library would: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def test_bad_shapes_raise_before_any_library_call(pkg):
    eng = object.__new__(pkg.GPEngine)      # no library is loaded, no device is opened
    eng._lib = NoLibrary(); eng._ctx = None
    N = pkg.LONG_SERIES_MAX_N
    ok = (np.zeros(4), np.zeros(4))
    q = np.zeros(3); y = np.zeros(3)
    k = pkg.Constant(1.0)
    call = eng.predict_logpdf_long_series_batch
    # pack_series applies its cap per series ...
    with pytest.raises(ValueError, match="series 1 has 513 points.*LONG_SERIES_MAX_N"):
        call([ok, (np.zeros(N + 1), np.zeros(N + 1))], [q, q[:0]], [y, y[:0]], [k], [0.1], [0])
    # ... and the joint length of a series with held-out points is checked here, both counts and the constant in the message
    with pytest.raises(ValueError, match=r"series 1 has 510 training and 3 held-out points.*LONG_SERIES_MAX_N \(512\)"):
        call([ok, (np.zeros(510), np.zeros(510))], [q, q], [y, y], [k], [0.1], [0])
    with pytest.raises(ValueError, match=r"series 0 has 0 training and 513 held-out points"):
        call([(np.zeros(0), np.zeros(0))], [np.zeros(N + 1)], [np.zeros(N + 1)], [k], [0.1], [0], all_long=True)
    with pytest.raises(ValueError, match="series 0"):
        call([(np.zeros(4), np.zeros(5))], [q], [y], [k], [0.1], [0])
    with pytest.raises(ValueError, match="one noise per particle"):
        call([ok], [q], [y], [k, k], [0.1], [0, 0])
    with pytest.raises(ValueError, match="one series index per particle"):
        call([ok], [q], [y], [k, k], [0.1, 0.1], [0], all_long=True)
    with pytest.raises(ValueError, match="one vector of query times per series"):
        call([ok, ok], [q], [y], [k], [0.1], [0])
    with pytest.raises(ValueError, match="one vector of held-out values per series"):
        call([ok, ok], [q, q], [y], [k], [0.1], [0])
    with pytest.raises(ValueError, match="series 0: 3 held-out values required"):
        call([ok], [q], [np.zeros(2)], [k], [0.1], [0])
    with pytest.raises(ValueError, match="one noise_pred per particle"):
        call([ok], [q], [y], [k, k], [0.1, 0.1], [0, 0], noise_pred=np.zeros(3))
    with pytest.raises(ValueError, match="weights has shape"):
        call([ok], [q], [y], [k, k], [0.1, 0.1], [0, 0], weights=np.ones(3))
    with pytest.raises(ValueError, match="y_transforms has shape"):
        call([ok], [q], [y], [k], [0.1], [0], y_transforms=np.ones((2, 2)))
    # the module-level wrapper: any max_n but the two caps, and the long entry's refusals through it
    for bad in (300, 0, N + 1):
        with pytest.raises(ValueError, match="max_n must be"):
            pkg.predict_proba_series(eng, [ok], [q], [y], [k], [0.1], [0], [0.0], max_n=bad)
    with pytest.raises(ValueError, match="series 0 has 513 points"):
        pkg.predict_proba_series(eng, [(np.zeros(N + 1), np.zeros(N + 1))], [q], [y], [k], [0.1], [0], [0.0], max_n=N)
    with pytest.raises(ValueError, match="series 0 has 510 training and 3 held-out points"):
        pkg.predict_proba_series(eng, [(np.zeros(510), np.zeros(510))], [q], [y], [k], [0.1], [0], [0.0], all_long=True)
    # pack_series itself: the cap it is given, per series; 512 points with nothing held out are no refusal of the joint check
    assert pkg.pack_series([(np.zeros(N), np.zeros(N))], max_n=N)[0].tolist() == [0, N]
    with pytest.raises(ValueError, match="series 0 has 512 points.*SERIES_MAX_N"):
        pkg.pack_series([(np.zeros(N), np.zeros(N))])


def test_lds_need_at_the_joint_length():
    """the long route keeps the long value kernel's map at N = n + m joint points; the figures include/autogp_hip.h and the new
    unit's header comment quote"""
    kern = (ROOT / "autogp.jl_amd" / "csrc" / "agp_long_series_kernel.hpp").read_text()
    assert "PRED ? long_series_pred_lds(n, h.n_ops, h.n_prm, h.n_cp) : long_series_lds(n, h.n_ops, h.n_prm, h.n_cp)" in kern
    assert LR.N_CAP == 512 and LR.N_SHORT == SPR.N_CAP == 176
    # however the joint length is split, the need is the value kernel's at that length
    for n, m in ((0, 512), (300, 212), (511, 1)):
        assert LR.long_series_proba_lds_total(n, m, 21, 31, 10) == LP.long_series_lds_total(512, 21, 31, 10)
    ten = 8 * LR.long_series_proba_lds_total(442, 70, 21, 31, 10)
    assert ten == 62832 and 61 * 1024 <= ten < 62 * 1024 and 2 * ten <= 160 * 1024      # 61 KiB: two workgroups share a CU
    assert LR.cp_chain_fits(10, 442, 70)
    k_fit = max(k for k in range(1, 60) if LR.cp_chain_fits(k, 442, 70))
    assert k_fit == 34 and not LR.cp_chain_fits(35, 442, 70)                            # the first count that does not fit: 35
    assert 8 * LR.long_series_proba_lds_total(0, 512, 69, 103, 34) == 161904 <= 160 * 1024 < 8 * LR.long_series_proba_lds_total(0, 512, 71, 106, 35)
    # a shorter joint series takes more: the first long length holds 35 and more
    assert LR.cp_chain_fits(35, 144, 36)
    # workspace: the value kernel's triangle, 528 blocks of 2 KiB at 512 joint points
    assert 32 * 33 // 2 == 528 and 528 * 2048 == 1081344


def test_ragged_case_is_what_the_gpu_tests_expect(pkg):
    series, qs, held, nodes, noises, sidx, noise_pred = LR.ragged_case()
    assert tuple((len(t), len(q)) for (t, _), q in zip(series, qs)) == LR.SHAPES and len(LR.SHAPES) == 24
    assert len(nodes) == 3 * len(LR.SHAPES) and [len(y) for y in held] == [len(q) for q in qs]
    assert (noise_pred[::2] < noises[::2]).all()
    N = np.array([n + m for n, m in LR.SHAPES])
    assert sorted(N[N > 176].tolist()) == [177, 177, 177, 177, 177, 177, 180, 337, 401, 465, 497, 512, 512, 512, 512]
    assert {337, 401, 465, 497, 512} <= set(LC.SIZES) and [n + m for n, m in LR.SHAPES_ALL] == [2, 16, 17, 65, 81]
    assert all(n + m <= 176 for n, m in LR.SHAPES_SHORT + LR.SHAPES_ALL) and all(n + m > 176 for n, m in LR.SHAPES_CAP + LR.SHAPES_LONG)
    # every fixture kernel — each leaf, both combinators, both ChangePoints — occurs on a series of more than 176 joint points
    fix = [k.to_tuple() for k in SPR.fixture_kernels(pkg)]
    above = {nodes[p].to_tuple() for p in range(len(nodes)) if N[sidx[p]] > 176}
    assert all(f in above for f in fix)
    # the three query kinds occur above 176 as well
    assert {s % 3 for s in range(len(N)) if N[s] > 176} == {0, 1, 2}


def test_restatement_against_the_reference():
    series, qs, held, nodes, noises, sidx, noise_pred = LR.ragged_case()
    refs = LR.ragged_references()
    assert len(refs) == len(nodes)                               # every particle is factored by the reference: none is skipped
    worst = worst_sum = 0.0
    for p, nd in enumerate(nodes):
        s = int(sidx[p])
        ref, S = refs[p]
        lp, terms, info = LR.long_series_proba_blocks(nd.to_tuple(), float(noises[p]), *series[s], qs[s], held[s],
                                                      noise_pred=float(noise_pred[p]))
        assert info == 0 and terms.shape == (len(qs[s]),), p
        if len(qs[s]) == 0:
            assert lp == 0.0 and ref == 0.0
            continue
        assert math.isfinite(ref) and S > 0.0
        worst = max(worst, abs(lp - ref) / S); worst_sum = max(worst_sum, abs(terms.sum() - lp) / S)
        assert abs(lp - ref) <= TOL * S, (p, LR.SHAPES[s], lp, ref, S)
        assert abs(terms.sum() - lp) <= 1e-12 * S, (p, LR.SHAPES[s])
    print(f"restatement against the reference: worst |lp - ref| / S = {worst:.3e}, worst |sum terms - lp| / S = {worst_sum:.3e} "
          f"over {len(nodes)} particles")


def test_restatement_agrees_with_the_short_kernels_restatement():
    """at most 176 joint points: the right-looking restatement of the short kernel and the left-looking one of the long kernel factor
    the same packed blocks"""
    series, qs, held, nodes, noises, sidx, noise_pred = LR.ragged_case()
    n_checked = 0
    for p, nd in enumerate(nodes):
        s = int(sidx[p])
        if sum(LR.SHAPES[s]) > 176 or len(qs[s]) == 0:
            continue
        a = LR.long_series_proba_blocks(nd.to_tuple(), float(noises[p]), *series[s], qs[s], held[s], noise_pred=float(noise_pred[p]), slope=-2.5)
        b = SPR.series_proba_blocks(nd.to_tuple(), float(noises[p]), *series[s], qs[s], held[s], noise_pred=float(noise_pred[p]), slope=-2.5)
        S = LR.ragged_references()[p][1]
        assert a[2] == b[2] == 0 and abs(a[0] - b[0]) <= 1e-12 * S and (np.abs(a[1] - b[1]) <= 1e-12 * S).all(), p
        n_checked += 1
    assert n_checked == 3 * 8


def test_slope_and_prior(pkg):
    """the Jacobian term, and the prior predictive (n = 0): every row is a query row, the value is the marginal likelihood of (tq, y)"""
    from oracle import oracle as O
    series, qs, held, nodes, noises, sidx, noise_pred = LR.ragged_case()
    s = LR.SHAPES.index((0, 177))
    for p in np.flatnonzero(sidx == s):
        nd, nz = nodes[p].to_tuple(), float(noises[p])
        lp, terms, info = LR.long_series_proba_blocks(nd, nz, *series[s], qs[s], held[s])
        direct = O.gp_logpdf(nd, nz, qs[s], held[s])
        S = PR.reference(nd, nz, *series[s], qs[s], held[s])[1]
        assert info == 0 and abs(lp - direct) <= TOL * S
        lp2, terms2, _ = LR.long_series_proba_blocks(nd, nz, *series[s], qs[s], held[s], slope=-2.5)
        assert abs(lp2 - (lp + 177 * math.log(2.5))) <= 1e-12 * (S + 177 * math.log(2.5))
        assert np.allclose(terms2 - terms, math.log(2.5), rtol=0, atol=1e-12)


def test_info_positions_on_the_joint_index():
    ts, xs, tq, y, nodes, noises, at = LR.bad_pivot_case()
    assert len(ts) == LR.BAD_SPLIT == 300 and len(tq) == 212
    got = [LR.long_series_proba_blocks(nd.to_tuple(), float(nz), ts, xs, tq, y) for nd, nz in zip(nodes, noises)]
    assert [g[2] for g in got] == [*LR.BAD_POSITIONS[:at], 0, *LR.BAD_POSITIONS[at:]]
    for i, (lp, terms, info) in enumerate(got):
        assert terms.shape == (212,)
        if i == at:
            ref, S = PR.reference(nodes[i].to_tuple(), float(noises[i]), ts, xs, tq, y)
            assert abs(lp - ref) <= TOL * S
        else:
            assert math.isnan(lp) and np.isnan(terms).all()
    # 1 .. n_s: K11 fails; n_s + k: leading minor k of the predictive covariance
    assert [p for p in LR.BAD_POSITIONS if p <= LR.BAD_SPLIT] == [1, 16, 177, 300]
    assert [p - LR.BAD_SPLIT for p in LR.BAD_POSITIONS if p > LR.BAD_SPLIT] == [1, 16, 197, 212]
