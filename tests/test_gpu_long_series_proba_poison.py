"""GPU test of agp_predict_logpdf_long_series_batch on a poisoned engine (AGP_POISON=1: every `values` buffer of the slot — the long
kernel's workspace with the joint factor among them — is NaN bytes before the call, and again between the launches of a split
call), after the pattern of tests/test_gpu_long_series_predict_poison.py: the ragged case under both routings, split into several
launches as well, the bad-pivot case and the mixtures must be, bit for bit, what an engine without poison returns — a block or a
vector entry read before it is written shows as a NaN or a changed bit here.  No reference and no tolerance: every comparison is
bitwise (a NaN compares as a NaN, whatever its payload).  The poisoned engine is a second GPEngine of this process, created while
AGP_POISON=1 is set — not a child process."""
import numpy as np
import pytest

import _long_series_proba_ref as LR
import test_gpu_long_series_proba as TP

pytestmark = pytest.mark.gpu


def nbits(sc):
    """every output of a call as one int64 vector, NaN as a flag of its own"""
    vals = np.concatenate([sc.logpdf, *sc.terms, sc.series_logp])
    return np.concatenate([TP.bits(np.nan_to_num(vals, nan=-1.0)), np.isnan(vals).astype(np.int64), np.asarray(sc.info, dtype=np.int64)])


def run_entries(engine):
    series, qs, held, nodes, noises, sidx, noise_pred = LR.ragged_case()
    w = TP.uniform_weights(sidx)
    call = lambda **kw: TP.scores(engine, series, qs, held, nodes, noises, sidx, weights=w, noise_pred=noise_pred,  # noqa: E731
                                  want_terms=True, **kw)
    out = [(f"ragged with mixtures, all_long={flag}", nbits(call(all_long=flag))) for flag in (False, True)]
    engine.set_workspace_limit(3 << 20)      # several launches share (and, poisoned, re-poison) one workspace
    try:
        out += [(f"ragged, split launches, all_long={flag}", nbits(call(all_long=flag))) for flag in (False, True)]
    finally:
        engine.set_workspace_limit(0)
    ts, xs, tq, y, cp, nz, at = LR.bad_pivot_case()
    P = len(cp)
    # the failing particles and the good one in one mixture, and the good one in a mixture of its own on a second series
    sidx2 = np.zeros(P + 1, dtype=np.int32); sidx2[P] = 1
    w2 = np.full(P + 1, 1.0 / P); w2[P] = 1.0
    res = TP.scores(engine, [(ts, xs), (ts, xs)], [tq, tq], [y, y], cp + [cp[at]], np.concatenate([nz, nz[at:at + 1]]), sidx2, weights=w2,
                    want_terms=True)
    assert np.isnan(res.series_logp[0]) and np.isfinite(res.series_logp[1])
    out.append(("bad pivots and their mixtures", nbits(res)))
    return out


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    ref = run_entries(engine)
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = run_entries(e)
            for (name, a), (_, b) in zip(ref, got):
                assert np.array_equal(a, b), (poison, name, np.flatnonzero(a != b)[:8])
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
