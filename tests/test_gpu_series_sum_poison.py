"""GPU test of agp_predict_sum_series_batch on a poisoned engine (AGP_POISON=1: every `values` buffer of the slot is NaN bytes before
the call), after the pattern of tests/test_gpu_series_sample_poison.py and on tests/test_gpu_series_poison.py's case: raw means,
variances, quantiles, training log-likelihoods and info must be, bit for bit, what an engine without poison returns — a region of a
staging or output buffer that the entry sizes but never writes, a selector entry of a query slot read before it is written, or an
operand read past a series' points, shows as a NaN or a changed bit here.  No oracle and no tolerance: every comparison is bitwise.
The poisoned engine is a second GPEngine of this process, created while AGP_POISON=1 is set (the variable is read when an engine is
created) — exactly how tests/test_gpu_series_poison.py builds its engines — and not a child process."""
import numpy as np
import pytest

import test_gpu_series as TS
import test_gpu_series_poison as SP

pytestmark = pytest.mark.gpu
bits = TS.bits
Q = (0.025, 0.5, 0.975)


def sum_case(G):
    """test_gpu_series_poison.poison_case(), every kernel split by Periodic / Linear / SquaredExponential in rotation; the deep and
    the wide tree (whose expansions outgrow a program) stand as they are beside a Periodic part"""
    series, queries, nodes, noises, sidx = SP.poison_case(G)
    leaf = (G.Periodic, G.Linear, G.SquaredExponential)
    splits = [G.split_kernel_sop(nd, leaf[k % 3]) if nd.size() < 20 else (nd, G.Periodic(0.7, 0.3, 0.4)) for k, nd in enumerate(nodes)]
    return series, queries, splits, noises, sidx


def run_entry(engine, case):
    series, queries, splits, noises, sidx = case
    S = len(series)
    yts = np.array([(1.5, 0.25), (-2.0, 1.0)] * S)[:S]
    out = []
    for tag, kw in (("own noise", {}), ("noise_pred", {"noise_pred": 0.5 * noises})):
        r = engine.predict_sum_series_batch(series, queries, splits, noises, sidx, q=Q, y_transforms=yts, want_var=True, want_logpdf=True,
                                            check=False, **kw)
        assert [len(m) for m in r.mean] == [3 * SP.N_QUERIES[s] for s in sidx]
        out += [(tag + " mean", np.concatenate([bits(a) for a in r.mean])), (tag + " var", np.concatenate([bits(a) for a in r.var])),
                (tag + " x", np.concatenate([bits(np.ascontiguousarray(a)).ravel() for a in r.x])), (tag + " logpdf", bits(r.logpdf)),
                (tag + " info", r.info.astype(np.int64))]
    return out


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    case = sum_case(pkg)
    ref = run_entry(engine, case)
    out = dict(ref)
    assert (out["own noise info"] == 0).all() and (out["noise_pred info"] == 0).all()
    assert all(np.isfinite(a.view(np.float64)).all() for name, a in ref if "info" not in name)
    assert np.array_equal(out["own noise logpdf"], out["noise_pred logpdf"])
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
