"""GPU test of agp_hmc_series_batch on a poisoned engine (AGP_POISON=1: every `values` buffer of the slot is NaN bytes before the
call), after the pattern of tests/test_gpu_series_sum_poison.py on the golden cases of tests/test_gpu_series_hmc.py: the final state,
the transformed parameters, the noise, the log-density, the counts, info and the trace must be, bit for bit, what an engine without
poison returns — a region of an output buffer that the entry sizes but the kernel never writes, or an LDS entry of the chain read
before it is written, shows as a NaN or a changed bit here.  No reference and no tolerance: every comparison is bitwise.  The poisoned
engine is a second GPEngine of this process, created while AGP_POISON=1 is set — not a child process."""
import numpy as np
import pytest

import test_gpu_series_hmc as TH

pytestmark = pytest.mark.gpu


def run_entry(engine, G):
    cs = list(TH.short_cases())
    out = []
    for tag, kw in (("trace", dict(want_trace=True)), ("no trace, frozen noise", dict(want_trace=False, L_noise=0)),
                    ("not positive definite", None)):
        r = TH.call(engine, G, [TH.GOLD["notpd_case"]]) if kw is None else TH.call(engine, G, cs, **kw)
        out.append((tag, TH.rbits(r)))
    return out


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    ref = run_entry(engine, pkg)
    for poison in ("0", "1"):
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = run_entry(e, pkg)
            for (name, a), (_, b) in zip(ref, got):
                assert np.array_equal(a, b), (poison, name, np.flatnonzero(a != b)[:8])
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
