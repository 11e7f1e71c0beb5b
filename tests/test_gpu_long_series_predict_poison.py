"""GPU test of agp_predict_long_series_batch and agp_predict_quantile_long_series_batch on a poisoned engine (AGP_POISON=1: every
`values` buffer of the slot — the long kernel's workspace with its factor, its inverse blocks and its scratch rows among them — is
NaN bytes before the call, and again between the launches of a split call), after the pattern of
tests/test_gpu_long_series_poison.py: the ragged case under both routings, split into several launches as well, the bad-pivot case
and the band must be, bit for bit, what an engine without poison returns — a scratch row or an inverse block read before it is
written shows as a NaN or a changed bit here.  No reference and no tolerance: every comparison is bitwise.  The poisoned engine is a
second GPEngine of this process, created while AGP_POISON=1 is set — not a child process."""
import numpy as np
import pytest

import _long_series_predict_ref as LP
import test_gpu_long_series_predict as TP

pytestmark = pytest.mark.gpu


def run_entries(engine, G):
    series, queries, nodes, noises, sidx, *_ = LP.ragged_case()
    out = []
    for flag in (False, True):
        out.append((f"ragged, all_long={flag}", TP.pbits(TP.forecast(engine, series, queries, nodes, noises, sidx, all_long=flag))))
    engine.set_workspace_limit(4 << 20)      # several launches share (and, poisoned, re-poison) one workspace
    try:
        out.append(("ragged, split launches", TP.pbits(TP.forecast(engine, series, queries, nodes, noises, sidx))))
    finally:
        engine.set_workspace_limit(0)
    ts, xs, q, cp, nz, at = TP.bad_pivot_case(G)
    res = TP.forecast(engine, [(ts, xs)], [q], cp, nz, np.zeros(len(cp), dtype=np.int32))
    out.append(("bad pivots", np.concatenate([TP.bits(np.nan_to_num(np.concatenate(res[0] + res[1]), nan=-1.0)),
                                              np.isnan(np.concatenate(res[0] + res[1])).astype(np.int64), res[3].astype(np.int64)])))
    _, _, _, _, _, w, yt = TP.band_inputs()
    band = engine.predict_quantile_long_series_batch(series, queries, nodes, noises, sidx, w, TP.QS, y_transforms=yt, want_moments=True,
                                                     want_logpdf=True, check=False)
    out.append(("band", np.concatenate([TP.sbits(band, s) for s in range(len(series))] + [TP.bits(band.logpdf)])))
    return out


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    ref = run_entries(engine, pkg)
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = run_entries(e, pkg)
            for (name, a), (_, b) in zip(ref, got):
                assert np.array_equal(a, b), (poison, name, np.flatnonzero(a != b)[:8])
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
