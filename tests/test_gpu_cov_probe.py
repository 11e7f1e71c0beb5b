"""The covariance tiles of the sweeps, entry by entry, on every table path (GPEngine.debug_cov_sweep = agp_debug_cov_sweep: the
sweep's own stages up to its covariance launch, every tile from k_cov_tiles, tiles and tables seeded with the sentinel -7).

Every entry of every live row and column is held to |dev - target| <= 8 R S (tests/_cov_probe_ref.py): the target is the
longdouble kernel at the element's own times on the general evaluator and at the representative difference of its table entry on
a table path; R is what the float64 routes of that (sweep, program) reach (admitted at R <= 8 x 2^-53 by
tests/test_cov_probe_cpu.py) and S the per-entry error scale.  The lag tables themselves are held to the same bound at the times
the device reports, those times are compared bit for bit with the host's lattice, padding rows and columns must hold the dense
packer's identity pattern, every position above the diagonal tiles the sentinel.  Each test asserts the path through out_mode."""
import os

import numpy as np
import pytest

import _cov_probe_ref as R

pytestmark = pytest.mark.gpu
_REFS = {}


@pytest.fixture(scope="module")
def cases(pkg):
    return R.sweep_cases(pkg.prior)


def engine_with(pkg, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.GPEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines(pkg):
    made = {"default": pkg.GPEngine(0), "no_ge_table": engine_with(pkg, {"AGP_GE_TABLE": "0"}), "built": engine_with(pkg, {"AGP_FUSE": "0"})}
    yield made
    for e in made.values():
        e.close()


def setup(pkg, cases, name):
    mk, n, mode, kw = cases[name]
    ts, xs = mk()
    n = len(ts) if n is None else n
    lay = R.sweep_layout(ts, n, mode, pkg.probe_lattice(ts) if mode != "general" else None)
    return ts, xs, n, mode, kw, lay


def refs_of(name, progs, ts, n, lay):
    out = []
    for nm, nd, nz in progs:
        if (name, nm) not in _REFS:
            _REFS[(name, nm)] = R.Ref(nd.to_tuple(), nz, ts[:n] if lay.mode == "general" else ts, lay, scalar_twin=n <= 300)
        out.append(_REFS[(name, nm)])
    return out


def check_entries(label, out, progs, refs, mults=None):
    worst = (0.0, None)
    for p, ((nm, nd, nz), ref) in enumerate(zip(progs, refs)):
        bad, ratio, where = R.violations(out["K"][p], ref)
        worst = max(worst, (ratio, (nm, where)))
        assert bad == 0, (label, nm, bad, ratio, where, ref.R / R.U)
    print(f"[cov-probe] {label}: worst |dev - target| / (R S) = {worst[0]:.2f} at {worst[1]}")


def table_index(lay, n):
    """(index into a table as out_tab holds it, entry) of the entries that stand for a difference of stored points."""
    if lay.mode == "sorted_lag":
        nt = -(-n // R.NB)
        bl, d = np.meshgrid(np.arange(nt), np.arange(-(R.NB - 1), R.NB), indexing="ij")
        g = np.abs(R.NB * bl + d)
        ok = g < n
        return (bl * 256 + d + R.NB - 1)[ok], g[ok]
    e = np.arange(lay.rep.size)
    return e, e


def check_tables(label, out, lay, progs, refs, n):
    m = lay.rep.size
    assert out["rep"] is not None and np.array_equal(out["rep"][:m], lay.rep), label          # the host's lattice, bit for bit
    pos, ent = table_index(lay, n)
    rep = out["rep"].astype(R.LD)
    X = R.Elements(rep[ent], rep[0])
    Xd = R.Elements(out["rep"][ent], out["rep"][0])
    t0, worst = 0, 0.0
    for (nm, nd, nz), ref in zip(progs, refs):
        subs = R.table_subtrees(nd.to_tuple())
        rows = out["tab"][t0:t0 + len(subs)][:, pos]
        t0 += len(subs)
        assert not (rows == R.SENTINEL).any(), (label, nm)
        free = list(range(len(subs)))
        for row in rows:          # (the compiler orders a node's operands by their stack need: match a table to its subtree by value)
            errs = []
            for s in free:
                T = R.eval_tree(subs[s], X, R.LD)
                S = R.error_scale(subs[s], Xd) + R.TINY
                errs.append(float(np.max(np.abs(row.astype(R.LD) - T).astype(np.float64) / S)))
            k = int(np.argmin(errs))
            assert errs[k] <= R.MULT * ref.R, (label, nm, errs[k] / R.U, ref.R / R.U)
            worst = max(worst, errs[k] / ref.R if ref.R > 0 else 0.0)
            free.pop(k)
    assert t0 == out["n_tables"], label
    print(f"[cov-probe] {label}: worst table |dev - target| / (R S) = {worst:.2f}")


def check_decodes(out, progs, pkg, group, tables):
    assert out["depth"] == (8 if group == "deep" else 4)
    for (nm, nd, nz), how in zip(progs, out["decode"]):
        pr = pkg.probe_program(nd)
        n_ops = pr["n_compiled"] if tables else len(pkg.encode(nd)[0])
        chain = pr["chain"] if tables else None
        if n_ops == 1:
            assert how == "one_node", nm
        elif group == "deep":
            assert how == "stack", nm
        elif chain is not None:
            assert how == ("chain" if chain else "stack"), nm
    if group == "deep":
        assert "stack" in out["decode"]
    elif len(progs) >= 20:
        assert {"chain", "stack", "one_node"} <= set(out["decode"])


CASE_NAMES = ["irregular1", "irregular2", "irregular127", "irregular128", "irregular129", "irregular257", "sorted129", "sorted256",
              "sorted300", "rank_prefix250", "rank_prefix129", "rank_gradient300", "rank_units256", "rank_units257", "rank_bdays300",
              "rank_lattice4096", "general_lattice4097", "compact_whole", "compact_whole_prefix", "compact_sorted"]


def test_case_names_are_the_reference_modules(cases):
    assert sorted(CASE_NAMES) == sorted(cases)


@pytest.mark.parametrize("group", R.GROUPS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_sweep_tiles_entry_by_entry(pkg, engines, cases, name, group):
    ts, xs, n, mode, kw, lay = setup(pkg, cases, name)
    progs = R.program_group(R.sweep_programs(pkg, ts, large=name in R.LARGE_CASES, for_gradient=bool(kw.get("for_gradient"))), group)
    refs = refs_of(name, progs, ts, n, lay)
    nodes = [nd for _, nd, _ in progs]
    noises = np.array([nz for _, _, nz in progs])
    for ename in (("default", "no_ge_table") if mode == "general" else ("default",)):
        eng = engines[ename]
        eng.set_data(ts, xs)
        out = eng.debug_cov_sweep(nodes, noises, n=n, **kw)
        label = f"{name}/{group}/{ename}"
        assert out["mode"] == mode, (label, out["mode"])
        assert np.array_equal(out["order"], lay.order), label
        assert out["logdt"] == (mode == "general" and ename == "default"), label
        check_decodes(out, progs, pkg, group, lay.tables)
        if name.startswith("rank_units"):
            assert out["tab_units"] == (1 if n == 256 else 2)
        if name == "rank_lattice4096":
            assert out["tab_units"] == 16
        if name == "compact_sorted":
            assert eng.compact_stats()["table_entries"] > 4096 and n >= 3 * R.NB
        if name == "compact_whole":
            assert eng.compact_stats()["table_entries"] <= 4096 < (n + 1) * eng.compact_stats()["lags_per_ordinal"]
        check_entries(label, out, progs, refs)
        if lay.tables:
            check_tables(label, out, lay, progs, refs, n)
        else:
            assert out["tab"] is None and out["n_tables"] == 0


@pytest.mark.parametrize("name", ["irregular129", "sorted300"])
def test_isolation_and_repeat(pkg, engines, cases, name):
    """A particle alone gives the bits it gives inside the mixed batch of all programs; a repeat gives the same bits; a matrix that is
    not positive definite changes nothing for its neighbours (no factorisation runs)."""
    ts, xs, n, mode, kw, lay = setup(pkg, cases, name)
    progs = R.sweep_programs(pkg, ts)
    nodes = [nd for _, nd, _ in progs] + [pkg.Times(pkg.Constant(-1.0), pkg.SquaredExponential(0.3, 1.0))]
    noises = np.array([nz for _, _, nz in progs] + [0.0])
    eng = engines["default"]
    eng.set_data(ts, xs)
    a = eng.debug_cov_sweep(nodes, noises, n=n, want_tables=False, **kw)
    b = eng.debug_cov_sweep(nodes, noises, n=n, want_tables=False, **kw)
    assert np.array_equal(a["K"], b["K"]) and a["decode"] == b["decode"] and a["mode"] == mode
    assert a["K"][-1][0, 0] < 0          # (the indefinite one came back like any other)
    c = eng.debug_cov_sweep(nodes[:-1], noises[:-1], n=n, want_tables=False, **kw)
    assert np.array_equal(a["K"][:-1], c["K"])
    for p in range(len(nodes)):
        one = eng.debug_cov_sweep(nodes[p:p + 1], noises[p:p + 1], n=n, want_tables=False, **kw)
        assert np.array_equal(one["K"][0], a["K"][p]), (name, p, one["decode"], a["decode"][p])


@pytest.mark.parametrize("name", ["irregular129", "sorted300", "rank_prefix250", "compact_whole_prefix", "compact_sorted"])
def test_tiles_are_what_production_factors(pkg, engines, cases, name):
    """The probe's live block through debug_factor_batch (the schedule logpdf_batch takes, y = xs in the sweep's order) gives the log
    density of the same context's logpdf_batch to 4 units in the last place of the largest of its three terms (three roundings,
    one for the order), and the same infos."""
    ts, xs, n, mode, kw, lay = setup(pkg, cases, name)
    progs = R.program_group(R.sweep_programs(pkg, ts, large=name in R.LARGE_CASES, for_gradient=bool(kw.get("for_gradient"))), "a")
    nodes = [nd for _, nd, _ in progs]
    noises = np.array([nz for _, _, nz in progs])
    eng = engines["built"]
    eng.set_data(ts, xs)
    lp, info = eng.logpdf_batch(nodes, noises, n=n, check=False)
    out = eng.debug_cov_sweep(nodes, noises, n=n, want_tables=False, **kw)
    assert out["mode"] == mode
    K = np.ascontiguousarray(out["K"][:, :n, :n])
    tile = np.arange(n) // R.NB
    upper = tile[:, None] < tile[None, :]          # (no sweep stores these tiles: mirrored from the lower ones)
    assert (K[:, upper] == R.SENTINEL).all()
    K[:, upper] = K.transpose(0, 2, 1)[:, upper]
    y = np.tile(xs[out["order"]], (len(nodes), 1))
    _, _, part, finfo = eng.debug_factor_batch(K, y, schedule=-1)
    if lay.mode in ("sorted_lag", "compact_sorted"):          # (logpdf_batch factors a rejected particle again in the caller's order)
        assert np.array_equal(finfo > 0, info > 0)
    else:
        assert np.array_equal(finfo, info)
    ok = info == 0
    assert ok.sum() >= len(nodes) - 2
    terms = np.stack([np.full(len(nodes), n * np.log(2 * np.pi)), part[:, 0], part[:, 1]])
    mine = -(terms[0] + terms[1] + terms[2]) / 2
    tol = 4 * np.spacing(np.abs(terms).max(axis=0)) / 2
    err = np.abs(mine - lp)
    print(f"[cov-probe] {name}: worst |probe + factor - logpdf_batch| = {np.max(err[ok] / tol[ok]) * 4:.2f} units in the last place")
    assert (err[ok] <= tol[ok]).all(), (name, np.argmax(err[ok] / tol[ok]))


def test_arguments(pkg, engines):
    import ctypes as C
    ts, xs = R.irregular_series(40, 3)
    nodes, noises = [pkg.SquaredExponential(0.3, 1.0), pkg.Linear(0.1, 0.2, 0.3)], np.array([0.1, 0.2])
    fresh = pkg.GPEngine(0)
    try:
        with pytest.raises(pkg.AGPError, match=r"\(-4\)"):          # no data
            fresh.debug_cov_sweep(nodes, noises, n=5)
    finally:
        fresh.close()
    eng = engines["default"]
    eng.set_data(ts, xs)
    stats = (eng.eval_stats(), eng.lag_stats(), eng.extend_stats() if hasattr(eng, "extend_stats") else None)
    with pytest.raises(pkg.AGPError, match=r"\(-4\)"):
        eng.debug_cov_sweep(nodes, noises, n=41)
    with pytest.raises(pkg.AGPError, match=r"\(-1\)"):
        eng.debug_cov_sweep(nodes, noises, n=0)
    with pytest.raises(pkg.AGPError, match=r"\(-1\)"):
        eng.debug_cov_sweep([], np.zeros(0), n=40)
    many = [pkg.Constant(0.1 + 1e-4 * i) for i in range(8193)]          # 8193 tiles of 2^14 doubles: past 2^27
    with pytest.raises(pkg.AGPError, match=r"\(-1\)"):
        eng.debug_cov_sweep(many, np.full(len(many), 0.1), n=40)
    with pytest.raises(pkg.AGPError, match=r"\(-3\)"):          # the gradient plan refuses what a gradient sweep refuses
        eng.debug_cov_sweep([R.chain_of(129, pkg)], np.array([0.1]), n=40, for_gradient=True)
    with pytest.raises(pkg.AGPError, match=r"\(-3\)"):
        eng.debug_cov_sweep(nodes, noises, n=40, programs=(np.array([0, 1, 2], dtype=np.int32), np.array([6, 2], dtype=np.uint8),
                                                           np.array([0, 0, 3], dtype=np.int32), np.array([0.1, 0.2, 0.3])))
    # null pointers, through the C ABI itself
    op_off, ops, prm_off, prm = pkg.encode_batch(nodes)
    lib, ctx = eng._lib, eng._ctx
    ip, dp, u8 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
    K = np.empty((2, 128, 128)); order = np.empty(40, dtype=np.int32); mode = np.zeros(10, dtype=np.int32)
    full = [ctx, 40, 2, ip(op_off), u8(ops), ip(prm_off), dp(prm), dp(noises), 0, 1, dp(K), ip(order), ip(mode), None, None]
    assert lib.agp_debug_cov_sweep(*full) == 0
    for hole in (3, 4, 5, 6, 7, 11, 12):
        args = list(full); args[hole] = None
        assert lib.agp_debug_cov_sweep(*args) == -1, hole
    assert lib.agp_debug_cov_sweep(None, *full[1:]) == -1
    # nothing of the context's counters moved
    assert stats == (eng.eval_stats(), eng.lag_stats(), eng.extend_stats() if hasattr(eng, "extend_stats") else None)
    assert eng.debug_cov_sweep(nodes, noises, n=40)["mode"] == "general"
