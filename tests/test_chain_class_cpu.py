"""Chain programs (include/autogp_hip.h agp_probe_program; csrc/agp_engine.hip compile_program, is_chain): a table-driven sweep
orders the children of every binary node by the stack need of the COMPILED tree — a collapsed stationary subtree is one leaf —
and marks a compiled postfix of the form leaf (leaf binop)* as a chain (ProgHdr.flags), which the tile builder evaluates without
a stack.  Host code only: no device."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def G(pkg):
    return pkg


def _leaves(G):
    lin = G.Linear(0.1, 0.2, 0.3)
    # a deep stationary operand: three transcendental leaves under + and x, one table in a lag sweep
    deep = G.Plus(G.SquaredExponential(0.3, 1.0), G.Times(G.Periodic(0.5, 0.2, 1.0), G.GammaExponential(0.4, 1.3, 0.9)))
    return lin, deep


def test_one_node_programs(G):
    lin, deep = _leaves(G)
    assert G.probe_program(lin) == {"n_compiled": 1, "chain": True, "depth": 1, "n_tables": 0}
    assert G.probe_program(deep) == {"n_compiled": 1, "chain": True, "depth": 1, "n_tables": 1}       # collapsed into one table leaf
    assert G.probe_program(G.Constant(0.5)) == {"n_compiled": 1, "chain": True, "depth": 1, "n_tables": 0}


@pytest.mark.parametrize("op", ["Plus", "Times"])
def test_compound_on_either_side_is_a_chain(G, op):
    lin, deep = _leaves(G)
    comp = G.Plus(lin, G.Linear(0.4, 0.1, 0.7))
    mk = getattr(G, op)
    for tree in (mk(comp, lin), mk(lin, comp), mk(comp, deep), mk(deep, comp)):
        r = G.probe_program(tree)
        assert r["chain"] and r["n_compiled"] == 5 and r["depth"] == 2, (tree, r)


def test_deep_stationary_operand_beside_a_linear_sum(G):
    """(Lin + Lin) * S_deep: by the ORIGINAL tree S_deep is the deeper operand and would be evaluated first — LAG LIN LIN + *, two
    values held, not a chain; by the compiled tree it is one leaf"""
    lin, deep = _leaves(G)
    s = G.Plus(lin, G.Linear(0.4, 0.1, 0.7))
    for tree in (G.Times(s, deep), G.Times(deep, s), G.Plus(s, deep), G.Plus(deep, s)):
        r = G.probe_program(tree)
        assert r == {"n_compiled": 5, "chain": True, "depth": 2, "n_tables": 1}, (tree, r)


def test_changepoint_in_both_orders(G):
    lin, deep = _leaves(G)
    comp = G.Times(lin, deep)
    for tree in (G.ChangePoint(comp, lin, 0.4, 0.05), G.ChangePoint(lin, comp, 0.4, 0.05),
                 G.ChangePoint(comp, deep, 0.4, 0.05), G.ChangePoint(deep, comp, 0.4, 0.05)):
        r = G.probe_program(tree)
        assert r["chain"] and r["n_compiled"] == 5 and r["depth"] == 2, (tree, r)
    # a longer one: ((Lin x S) cp Lin) + S, compounds alternating sides
    tree = G.Plus(deep, G.ChangePoint(lin, G.ChangePoint(comp, lin, 0.4, 0.05), 0.6, 0.1))
    r = G.probe_program(tree)
    assert r["chain"] and r["n_compiled"] == 9 and r["depth"] == 2, r


def test_two_compound_operands_are_not_a_chain(G):
    lin, deep = _leaves(G)
    tree = G.Plus(G.Times(lin, deep), G.Times(G.Linear(0.4, 0.1, 0.7), deep))
    r = G.probe_program(tree)
    assert not r["chain"] and r["n_compiled"] == 7 and r["depth"] == 3 and r["n_tables"] == 2, r
    tree = G.ChangePoint(G.Plus(lin, lin), G.Times(lin, deep), 0.4, 0.05)
    r = G.probe_program(tree)
    assert not r["chain"] and r["depth"] == 3, r


def test_benchmark_population(G):
    """the 512 particles bench.py sweeps: 117 programs of more than one node after compilation, 95 of them chains (a Python
    restatement of the class test counts the same), none of which needs a stack deeper than 2"""
    nodes, _ = G.prior.sample_particles(np.random.default_rng(2048), 512, max_size=63)
    res = [G.probe_program(nd) for nd in nodes]
    multi = [r for r in res if r["n_compiled"] > 1]
    chains = [r for r in multi if r["chain"]]
    assert len(chains) >= 90, f"{len(chains)} of {len(multi)} multi-node programs are chains"
    deep = [r for r in chains if r["depth"] > 2]
    assert not deep, f"{len(deep)} of {len(chains)} chains need a stack deeper than 2: {deep[:3]}"
    assert all(r["n_compiled"] % 2 == 1 for r in chains)
    print(f"{len(chains)} of {len(multi)} multi-node programs are chains ({sum(r['n_compiled'] for r in chains)} of "
          f"{sum(r['n_compiled'] for r in multi)} nodes, {min(r['n_compiled'] for r in chains)}..{max(r['n_compiled'] for r in chains)} nodes each)")
