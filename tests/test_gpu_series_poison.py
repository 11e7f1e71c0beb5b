"""GPU test of the many-series entries on a poisoned engine (AGP_POISON=1: every `values` buffer of the slot is NaN bytes before the
call): agp_logpdf_series_batch, agp_logpdf_grad_series_batch and agp_predict_series_batch must return, bit for bit, what an engine
without poison returns — a region of a staging or output buffer that an entry sizes but never writes shows as a NaN or a changed bit
here and nowhere else.  (The band entry runs poisoned in test_gpu_series_quantile.py::test_batch_independence_bitwise.)  No oracle
and no tolerance: every comparison is bitwise.

The case: five series of 0, 1, 17, 33 and 176 points (0, 1, 2, 3 and 11 block rows) cut from test_gpu_series.ragged_case(), with 3,
0, 17, 65 and 1 query times — the prior predictive of the empty series, a series with nothing to predict, a second query block on a
second wave, a fifth query block back on wave 0 — and two of the ragged case's own particles each.  On the 176-point series also
cp_chain(G, 4), the longest ChangePoint chain whose per-point tables fit the gradient kernel's LDS at 176 points, the 31-node
full_tree(G, 4) and a 23-node tree.  A chain's evaluation stack is 2 deep whatever its length, so it is the 31-node tree (stack depth
5) that takes the depth-8 instantiation of the value and predictive kernels and the 64-node tape at depth 8 of the gradient kernel;
the 23-node tree (depth 4) takes the 64-node tape at depth 4, everything else the depth-4 / 16-node instantiations."""
import numpy as np
import pytest

import test_gpu_series as TS

pytestmark = pytest.mark.gpu
bits = TS.bits
LENS = (0, 1, 17, 33, 176)
N_QUERIES = (3, 0, 17, 65, 1)


def poison_case(G):
    series_all, nodes_all, noises_all, sidx_all, _ = TS.ragged_case()
    lens_all = [len(t) for t, _ in series_all]
    series, queries, nodes, noises, sidx = [], [], [], [], []
    for s, (n, m) in enumerate(zip(LENS, N_QUERIES)):
        src = lens_all.index(n)
        ts, xs = series_all[src]
        series.append((ts, xs))
        tq = (ts.max() if n else 1.0) + 0.01 * np.arange(1, m + 1)
        if m and n:
            tq[0] = ts[0]                                            # a query on a training time
        queries.append(tq)
        own = np.flatnonzero(sidx_all == src)[:2]
        nodes += [nodes_all[i] for i in own]; noises += [noises_all[i] for i in own]; sidx += [s, s]
    chain, deep, wide = TS.cp_chain(G, 4), TS.full_tree(G, 4), TS.full_tree(G, 3) + TS.full_tree(G, 2, 1)
    assert chain.size() == 9 and deep.size() == 31 and wide.size() == 23
    nodes += [chain, deep, wide]; noises += [0.1, 0.2, 0.15]; sidx += [4, 4, 4]
    return series, queries, nodes, np.array(noises), np.array(sidx, dtype=np.int32)


def run_entries(engine, case):
    """every output of the three entries as one list of (name, int64 bits)"""
    series, queries, nodes, noises, sidx = case
    lp, info = engine.logpdf_series_batch(series, nodes, noises, sidx, check=False)
    glp, grads, gn, ginfo = engine.logpdf_grad_series_batch(series, nodes, noises, sidx, check=False)
    means, vars_, plp, pinfo = engine.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, check=False)
    assert [len(m) for m in means] == [N_QUERIES[s] for s in sidx] == [len(v) for v in vars_]
    return [("logpdf", bits(lp)), ("info", info.astype(np.int64)),
            ("grad logpdf", bits(glp)), ("grads", bits(np.concatenate(grads))), ("grad_noise", bits(gn)), ("grad info", ginfo.astype(np.int64)),
            ("means", bits(np.concatenate(means))), ("vars", bits(np.concatenate(vars_))), ("predict logpdf", bits(plp)),
            ("predict info", pinfo.astype(np.int64))]


def test_poisoned_engine_bitwise(pkg, engine, monkeypatch):
    case = poison_case(pkg)
    ref = run_entries(engine, case)
    out = dict(ref)
    assert (out["info"] == 0).all() and (out["grad info"] == 0).all() and (out["predict info"] == 0).all()
    assert all(np.isfinite(a.view(np.float64)).all() for name, a in ref if "info" not in name)
    assert np.array_equal(out["logpdf"], out["grad logpdf"]) and np.array_equal(out["logpdf"], out["predict logpdf"])
    for poison in ("0", "1"):                                        # (tests/test_gpu_series_quantile.py builds the engines so)
        monkeypatch.setenv("AGP_POISON", poison)
        e = pkg.GPEngine(0)
        monkeypatch.delenv("AGP_POISON")
        try:
            got = run_entries(e, case)
            for (name, a), (_, b) in zip(ref, got):
                assert np.array_equal(a, b), (poison, name, np.flatnonzero(a != b)[:8])
            if poison == "1":
                assert e.poison_stats()["bytes"] > 0
        finally:
            e.close()
