"""GPU test of agp_predict_sample_series_batch on a poisoned engine (AGP_POISON=1: every `values` buffer of the slot is NaN bytes
before the call), after the pattern of tests/test_gpu_series_poison.py and on its case: samples (seeded, and with the caller's
components and normals), component means and covariances and info must be, bit for bit, what an engine without poison returns — a
region of a staging or output buffer that the entry sizes but never writes, or an operand read above the diagonal of a factored
block, shows as a NaN or a changed bit here.  No oracle and no tolerance: every comparison is bitwise.
The poisoned engine is a second GPEngine of this process, created while AGP_POISON=1 is set (the variable is read when an engine is
created) — exactly how tests/test_gpu_series_poison.py builds its engines — and not a child process: the engine under test shares
nothing with the session's engine but the process, and no further process opens the GPU."""
import numpy as np
import pytest

import test_gpu_series as TS
import test_gpu_series_poison as SP

pytestmark = pytest.mark.gpu
bits = TS.bits
R_SAMPLES = 19


def sample_case(G):
    """test_gpu_series_poison.poison_case() with the 176-point series cut to 150 points (150 + 1 query: ten blocks) and the series
    of 33 points + 65 queries (98 joint points: seven blocks, five query blocks)"""
    series, queries, nodes, noises, sidx = SP.poison_case(G)
    series = [(t[:150], x[:150]) for t, x in series]
    return series, queries, nodes, noises, sidx


def run_entry(engine, case):
    series, queries, nodes, noises, sidx = case
    S = len(series)
    w = np.array([1.0 / (sidx == s).sum() for s in sidx])
    yts = np.array([(1.5, 0.25), (-2.0, 1.0)] * S)[:S]
    out = []
    rng = np.random.default_rng(11)
    lists = [np.flatnonzero(sidx == s) for s in range(S)]
    comp = np.array([[lists[s][j % len(lists[s])] for j in range(R_SAMPLES)] for s in range(S)], dtype=np.int32)
    z = [rng.standard_normal((len(q), R_SAMPLES)) for q in queries]
    for kw in ({"seeds": np.arange(40, 40 + S)}, {"component": comp, "z": z}):
        r = engine.predict_sample_series_batch(series, queries, nodes, noises, sidx, w, R_SAMPLES, y_transforms=yts, want_moments=True,
                                               check=False, **kw)
        tag = "seeded" if "seeds" in kw else "caller"
        out += [(tag + " x", np.concatenate([bits(np.ascontiguousarray(x)).ravel() for x in r.x])),
                (tag + " component", r.component.astype(np.int64).ravel()),
                (tag + " mean", np.concatenate([bits(a) for a in r.mean])),
                (tag + " cov", np.concatenate([bits(np.ascontiguousarray(c)).ravel() for c in r.cov])),
                (tag + " info", r.info.astype(np.int64))]
    return out


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    case = sample_case(pkg)
    ref = run_entry(engine, case)
    out = dict(ref)
    assert (out["seeded info"] == 0).all() and (out["caller info"] == 0).all()
    assert all(np.isfinite(a.view(np.float64)).all() for name, a in ref if "info" not in name and "component" not in name)
    assert np.array_equal(out["seeded mean"], out["caller mean"]) and np.array_equal(out["seeded cov"], out["caller cov"])
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = run_entry(e, case)
            for (name, a), (_, b) in zip(ref, got):
                assert np.array_equal(a, b), (poison, name, np.flatnonzero(a != b)[:8])
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
