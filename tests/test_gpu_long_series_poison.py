"""GPU test of agp_logpdf_long_series_batch on a poisoned engine (AGP_POISON=1: every `values` buffer of the slot — the long kernel's
factor workspace among them — is NaN bytes before the call), after the pattern of tests/test_gpu_series_hmc_poison.py: the ragged
case of tests/test_gpu_long_series.py under both routings, split into several launches as well, and the bad-pivot case must be, bit
for bit, what an engine without poison returns — a workspace block read before it is written shows as a NaN or a changed bit here.
No reference and no tolerance: every comparison is bitwise.  The poisoned engine is a second GPEngine of this process, created while
AGP_POISON=1 is set — not a child process."""
import numpy as np
import pytest

import test_gpu_long_series as TL

pytestmark = pytest.mark.gpu


def run_entry(engine, G):
    series, nodes, noises, sidx, _ = TL.ragged_case()
    out = []
    for flag in (False, True):
        lp, info = engine.logpdf_long_series_batch(series, nodes, noises, sidx, all_long=flag, check=False)
        out.append((f"ragged, all_long={flag}", TL.bits(lp), info))
    engine.set_workspace_limit(3 << 20)      # several launches share (and, poisoned, re-poison) one workspace
    try:
        lp, info = engine.logpdf_long_series_batch(series, nodes, noises, sidx, check=False)
    finally:
        engine.set_workspace_limit(0)
    out.append(("ragged, split launches", TL.bits(lp), info))
    ts = TL.cp_ts()
    xs = np.random.default_rng(31).standard_normal(ts.size)
    cp = [TL.changepoint_particle(G, k) for k in TL.CP_POINTS] + [G.SquaredExponential(0.3, 0.8)]
    nz = np.full(len(cp), TL.CP_NOISE); nz[-1] = 0.1
    lp, info = engine.logpdf_long_series_batch([(ts, xs)], cp, nz, np.zeros(len(cp), dtype=np.int32), check=False)
    out.append(("bad pivots", TL.bits(lp), info))
    return out


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    ref = run_entry(engine, pkg)
    assert ref[3][2][:-1].tolist() == [k + 1 for k in TL.CP_POINTS] and ref[3][2][-1] == 0
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = run_entry(e, pkg)
            for (name, a, ia), (_, b, ib) in zip(ref, got):
                assert np.array_equal(a, b), (poison, name, np.flatnonzero(a != b)[:8])
                assert np.array_equal(ia, ib), (poison, name)
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
