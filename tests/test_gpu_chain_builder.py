"""GPU tests of the tile builder's program decode (csrc/agp_cov_kernel.hpp: stage_node_records, eval_chain; include/autogp_hip.h
agp_get_eval_stats).  k_cov_tiles reads a program from node records staged in LDS and evaluates chains — leaf (leaf binop)* —
without a stack.  Hand-built programs put every leaf kind a table-driven sweep can hold under every operator, ChangePoint in both
operand orders, as the second and as the third pair of a chain; the builder's tiles are checked against the oracle, against the
stack interpreter inside the dataflow kernel (an independent decode: program staged as opcodes + parameters) and against the direct
leaves of the general path, on tiles of every shape and on all three table kinds."""
import numpy as np
import pytest

from oracle import fast as F

pytestmark = pytest.mark.gpu
LP_TOL = 1e-8


def lp_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def programs(G):
    lin = G.Linear(0.1, 0.2, 0.3)
    deep = G.Plus(G.SquaredExponential(0.3, 1.0), G.Times(G.Periodic(0.5, 0.2, 1.0), G.GammaExponential(0.4, 1.3, 0.9)))
    leaves = [G.SquaredExponential(0.25, 0.8), deep, G.Linear(0.45, 0.15, 0.6), G.Constant(0.35), G.WhiteNoise(0.2)]
    first = G.Plus(lin, G.Periodic(0.6, 0.25, 0.9))                       # LIN LAG +
    second = G.Times(first, G.Linear(0.7, 0.3, 0.2))                      # ... LIN x
    out = []
    for comp in (first, second):                                          # the new leaf is the second / the third pair
        for lf in leaves:
            out += [G.Plus(comp, lf), G.Times(lf, comp), G.ChangePoint(comp, lf, 0.4, 0.05), G.ChangePoint(lf, comp, 0.55, 0.08)]
    long = first
    for k in range(6):                                                    # 15 nodes
        lf = leaves[k % len(leaves)]
        long = (G.Plus(long, lf), G.ChangePoint(lf, long, 0.3 + 0.1 * k, 0.06), G.Times(long, G.Linear(0.2 * k, 0.9, 0.1)))[k % 3]
    out.append(long)
    # not chains: two compound operands
    out.append(G.Plus(G.Times(lin, deep), G.Times(G.Linear(0.4, 0.1, 0.7), G.SquaredExponential(0.2, 1.0))))
    out.append(G.ChangePoint(G.Plus(lin, G.Constant(0.2)), G.Times(lin, deep), 0.5, 0.07))
    out += [lin, deep]                                                    # one node
    return out


SERIES = {
    "grid300": lambda P: P.synthetic_series(300, seed=31, shuffle=True),      # three tile rows, ragged last row, padded diagonal tile
    "grid256": lambda P: P.synthetic_series(256, seed=32, shuffle=True),      # no padding
    "bdays300": lambda P: P.calendar_series(300, freq="B", seed=33),          # rank tables, read in place
    "months900": lambda P: P.calendar_series(900, freq="M", seed=34),         # compact tables on the sorted sweep
}


@pytest.fixture(scope="module")
def engines(pkg):
    """builder (every tile prebuilt), dataflow kernel with in-kernel evaluation of small programs, general path"""
    import os
    made = {}
    for name, env in (("built", {"AGP_FUSE": "0"}), ("flow", {"AGP_FUSE": "1", "AGP_FLOW": "1"}), ("direct", {"AGP_FUSE": "0", "AGP_LAG": "0"})):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            made[name] = pkg.GPEngine(0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    yield made
    for e in made.values():
        e.close()


@pytest.mark.parametrize("series", list(SERIES))
def test_builder_chains_against_oracle_and_other_evaluators(pkg, engines, series):
    nodes = programs(pkg)
    noises = np.linspace(0.05, 0.3, len(nodes))
    probes = [pkg.probe_program(nd) for nd in nodes]
    n_chain = sum(1 for r in probes if r["chain"] and r["n_compiled"] > 1)
    assert n_chain == len(nodes) - 4 and max(r["n_compiled"] for r in probes if r["chain"]) == 15
    ts, xs = SERIES[series](pkg.prior)
    ref, rinfo = F.gp_logpdf_many(pkg.encode_batch(nodes), noises, ts, xs)
    res = {}
    for name, eng in engines.items():
        eng.set_data(ts, xs)
        s0 = eng.lag_stats()[1]
        lp, info = eng.logpdf_batch(nodes, noises, check=False)
        lp2, info2 = eng.logpdf_batch(nodes, noises, check=False)
        assert np.array_equal(lp, lp2) and np.array_equal(info, info2), name          # bitwise, run to run
        assert np.array_equal(info, rinfo), name
        ok = info == 0
        assert ok.sum() >= len(nodes) - 2
        err = lp_err(lp[ok], ref[ok])
        print(series, name, "max error against the oracle", err.max(), eng.eval_stats())
        assert err.max() <= LP_TOL, (name, int(np.argmax(err)))
        st = eng.eval_stats()
        if name == "built":
            assert st == {"one_node": 0, "chain": 0, "stack": 0, "prebuilt": len(nodes), "prebuilt_chain": n_chain}, st
            if series.startswith("grid"):
                assert eng.lag_stats()[0] and eng.lag_stats()[1] == s0 + 2          # lag tables were in use
            else:
                assert eng.lattice_stats()["kind"] == (2 if series == "bdays300" else 3)
        if name == "flow":
            assert st["stack"] > 0 and st["one_node"] == 2, st                      # small programs went through the kernels' interpreter
        res[name] = (lp, ok)
    a, ok = res["built"]
    # the project's fused-against-prebuilt bound (1e-10 on calendar series), and the table-against-direct bound
    tol = 1e-11 if series.startswith("grid") else 1e-10
    assert lp_err(a[ok], res["flow"][0][ok]).max() <= tol
    assert lp_err(a[ok], res["direct"][0][ok]).max() <= 1e-10
