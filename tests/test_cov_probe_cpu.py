"""CPU side of the covariance probe (tests/_cov_probe_ref.py; no device): the longdouble targets are pinned against 60-digit
arithmetic (oracle/oracle_mp.py), every (sweep, program) the GPU tests use is ADMITTED — its float64 routes lie within
R <= 8 x 2^-53 of the target they aim at, in units of the per-entry scale S — every planted fault is caught at the bound the device
is held to (8 R S), and a table's representative target is tied to the elements' own: |T_rep - T_own| <= |dk/dd| |delta d| + 4 u S."""
import numpy as np
import pytest

import _cov_probe_ref as R
from oracle import oracle_mp as MP

U = R.U
PIN = 2.0 ** -7 * U          # the targets' own error: under 1 % of one unit of 2^-53 S (longdouble carries 11 more bits than double)


@pytest.fixture(scope="module")
def cases(pkg):
    return R.sweep_cases(pkg.prior)


def make(pkg, cases, name):
    mk, n, mode, kw = cases[name]
    ts, xs = mk()
    n = len(ts) if n is None else n
    lat = pkg.probe_lattice(ts) if mode != "general" else None
    return ts, n, R.sweep_layout(ts, n, mode, lat)


def program(pkg, ts, name, large=False):
    for nm, nd, nz in R.sweep_programs(pkg, ts, large):
        if nm == name:
            return nd.to_tuple(), nz
    raise KeyError(name)


@pytest.mark.parametrize("series", ["irregular129", "sorted129"])
def test_longdouble_targets_against_60_digits(pkg, cases, series):
    """At least 200 fixed entries per family — the tile corners and the smallest entries among them."""
    ts, n, _ = make(pkg, cases, series)
    lay = R.Layout("general", np.arange(n))
    worst = 0.0
    for nm, nd, nz in R.sweep_programs(pkg, ts):
        tree = nd.to_tuple()
        T_own, _, S = R.targets(tree, nz, ts, lay)
        ii, jj = R.sample_entries(n, k=200)
        small = np.argsort(np.abs(T_own).astype(np.float64), axis=None)[:8]
        ii = np.concatenate([ii, small // n]); jj = np.concatenate([jj, small % n])
        assert len(ii) >= 200
        for i, j in zip(ii, jj):
            v = MP.eval_cov_mp(tree, ts[i], ts[j]) + (MP._f(nz) if i == j else 0)
            err = abs(MP.mp.mpf(str(np.format_float_scientific(T_own[i, j], precision=30, unique=False))) - v)
            worst = max(worst, float(err / MP.mp.mpf(float(S[i, j]))))
            assert err <= PIN * S[i, j], (nm, int(i), int(j), float(err), float(S[i, j]))
    print(f"[cov-probe] {series}: worst |T_own - mp| / S = {worst / U:.2e} units of 2^-53")


def test_every_gpu_case_is_admitted(pkg, cases):
    """R <= 8 x 2^-53 for every (sweep, program) of tests/test_gpu_cov_probe.py."""
    table = []
    for name in cases:
        ts, n, lay = make(pkg, cases, name)
        kw = cases[name][3]
        tt = ts[:n] if lay.mode == "general" else ts
        for nm, nd, nz in R.sweep_programs(pkg, ts, large=name in R.LARGE_CASES, for_gradient=bool(kw.get("for_gradient"))):
            ref = R.Ref(nd.to_tuple(), nz, tt, lay, scalar_twin=n <= 300)
            table.append((ref.R / U, name, nm))
            assert ref.R <= R.R_CAP, (name, nm, {k: v / U for k, v in ref.route_err.items()})
    table.sort(reverse=True)
    print("[cov-probe] largest R (units of 2^-53):", [(round(r, 2), c, p) for r, c, p in table[:5]])


# ---- planted faults: each must leave at least one entry outside 8 R S -------------------------------------------------------------
def caught(ref, K, n_pad=None, pad_noise=0.0):
    n_pad = n_pad or R.NB * -(-K.shape[0] // R.NB)
    return R.violations(R.pad_route(K, n_pad, pad_noise), ref)[0] > 0


@pytest.fixture(scope="module")
def sorted300(pkg, cases):
    ts, n, lay = make(pkg, cases, "sorted300")
    tree, nz = program(pkg, ts, "chain0")
    ref = R.Ref(tree, nz, ts, lay)
    assert not caught(ref, R.table_route(tree, nz, ts, lay))          # (the route itself is inside the bound)
    return ts, lay, tree, nz, ref


@pytest.mark.parametrize("fault", [dict(corner_lag=1), dict(corner_lag=-1), dict(neighbour_block=True), dict(entry255=True)])
def test_fault_wrong_table_entry_sorted_layout(sorted300, fault):
    """The table read at lag g +- 1 in one tile corner only; the table of the neighbouring block lag; entry 255 of a sorted table."""
    ts, lay, tree, nz, ref = sorted300
    f = R.Faults()
    for k, v in fault.items():
        setattr(f, k, v)
    K = R.table_route(tree, nz, ts, lay, f)
    assert caught(ref, K)
    if "corner_lag" in fault:          # one entry, and its mirror is not touched
        assert R.violations(R.pad_route(K, 384), ref)[0] == 1


def test_fault_compact_window_rebased_by_one(pkg, cases):
    ts, n, lay = make(pkg, cases, "compact_sorted")
    tree, nz = program(pkg, ts, "chain2")
    ref = R.Ref(tree, nz, ts, lay, scalar_twin=False)
    assert not caught(ref, R.table_route(tree, nz, ts, lay))
    for step in (1, -1):
        f = R.Faults(); f.window_rebase = step
        assert caught(ref, R.table_route(tree, nz, ts, lay, f))


def test_fault_representative_from_rescaled_dates(pkg, cases):
    """The lag times taken as differences of rescaled dates, t_g - t_0, instead of g h as one product: caught
    where a fast period multiplies the half unit in the last place of |t| that a rescaled date carries."""
    P = pkg.prior
    ts, n, lay = make(pkg, cases, "rank_bdays300")
    x = P.datetime2unix(P.calendar_dates(300, "B"))
    slope, icpt = P.linear_transform_minmax(x, 0.0, 1.0)
    g = np.arange(lay.rep.size, dtype=np.float64)
    f = R.Faults(); f.rescaled_rep = (slope * (x[0] + 86400.0 * g) + icpt) - (slope * x[0] + icpt)
    assert (f.rescaled_rep != lay.rep).any() and np.abs(f.rescaled_rep - lay.rep).max() < 1e-14
    tree, nz = program(pkg, ts, "small5")          # Periodic(0.9, 0.004, 0.6) + Constant
    ref = R.Ref(tree, nz, ts, lay)
    assert not caught(ref, R.table_route(tree, nz, ts, lay))
    assert caught(ref, R.table_route(tree, nz, ts, lay, f))


@pytest.fixture(scope="module")
def irregular129(pkg, cases):
    ts, n, lay = make(pkg, cases, "irregular129")
    return ts, lay


def f64_route(tree, nz, ts, faults=None):
    X = R.Elements(ts[:, None], ts[None, :])
    return R.add_noise(R.eval_tree(tree, X, np.float64, None, faults), nz, np.float64)


def test_fault_noise_on_padding_and_missing_on_last_row(pkg, irregular129):
    ts, lay = irregular129
    tree, nz = program(pkg, ts, "small0")          # (noise 1e-5, the model's jitter)
    ref = R.Ref(tree, nz, ts, lay)
    K = f64_route(tree, nz, ts)
    assert not caught(ref, K)
    assert caught(ref, K, pad_noise=nz)
    K[-1, -1] -= nz
    assert caught(ref, K)


@pytest.mark.parametrize("fault", ["cp_swap", "sigma_column"])
def test_fault_changepoint(pkg, irregular129, fault):
    """ChangePoint operands swapped; sigma evaluated with the column's time for the row."""
    ts, lay = irregular129
    for name in ("chain2", "chain3", "small11"):
        tree, nz = program(pkg, ts, name)
        ref = R.Ref(tree, nz, ts, lay)
        f = R.Faults(); setattr(f, fault, True)
        assert not caught(ref, f64_route(tree, nz, ts)) and caught(ref, f64_route(tree, nz, ts, f)), name


def test_fault_se_tail_flushed_one_binade_early(pkg, cases):
    for series in ("irregular129", "sorted300"):
        ts, n, lay = make(pkg, cases, series)
        tree, nz = program(pkg, ts, "tail0")
        ref = R.Ref(tree, nz, ts, lay)
        v = ref.target[ref.target > 0].astype(np.float64)
        assert ((v >= 2.0 ** -1022) & (v < 2.0 ** -1021)).any()          # an entry lives in the last normal binade
        f = R.Faults(); f.flush_tail = True
        route = (lambda fl: R.table_route(tree, nz, ts, lay, fl)) if lay.tables else (lambda fl: f64_route(tree, nz, ts, fl))
        assert not caught(ref, route(None)) and caught(ref, route(f)), series


def test_fault_duplicated_time(pkg, irregular129):
    """The reference's WhiteNoise is (t_i == t_j) x value (src/GP.jl:137-140): at a duplicated time the off-diagonal entry carries
    it, while the observation noise sits on i == j alone.  Both confusions are caught: the noise added wherever the times agree, and
    WhiteNoise decided by the index."""
    ts, lay = irregular129
    i, j = np.argwhere((ts[:, None] == ts[None, :]) & ~np.eye(len(ts), dtype=bool))[0]
    tree, nz = program(pkg, ts, "small14")          # WhiteNoise + SE
    ref = R.Ref(tree, nz, ts, lay)
    K = f64_route(tree, nz, ts)
    assert not caught(ref, K)
    A = K.copy(); A[i, j] += nz; A[j, i] += nz
    B = K.copy(); B[i, j] -= 0.05; B[j, i] -= 0.05
    assert caught(ref, A) and caught(ref, B)


def replace_pair_operator(tree, pair):
    """The chain `tree` with the operator of its pair-th pair (1-based from the first leaf) replaced."""
    spine = []
    t = tree
    while t[0] in ("+", "*", "CP"):
        spine.append(t)
        t = t[1] if t[1][0] in ("+", "*", "CP") else (t[2] if t[2][0] in ("+", "*", "CP") else None)
        if t is None:
            break
    target = spine[len(spine) - pair]          # (the innermost binary node is pair 1)

    def rebuild(t):
        if t is target:
            return ("*" if t[0] != "*" else "+", t[1], t[2])
        if t[0] in ("+", "*"):
            return (t[0], rebuild(t[1]), rebuild(t[2]))
        if t[0] == "CP":
            return ("CP", rebuild(t[1]), rebuild(t[2]), t[3], t[4])
        return t
    return rebuild(tree)


def test_fault_operator_of_the_third_pair_of_the_15_node_chain(pkg, irregular129):
    ts, lay = irregular129
    node = [nd for nm, nd, _ in R.sweep_programs(pkg, ts) if nm == "chain40"][0]
    assert pkg.probe_program(node)["n_compiled"] == 15 and pkg.probe_program(node)["chain"]
    tree, nz = program(pkg, ts, "chain40")
    ref = R.Ref(tree, nz, ts, lay)
    wrong = replace_pair_operator(tree, 3)
    assert wrong != tree
    assert not caught(ref, f64_route(tree, nz, ts)) and caught(ref, f64_route(wrong, nz, ts))


# ---- a table may differ from the element's own value, by the slope times the representative's distance ---------------------------
@pytest.mark.parametrize("name", ["sorted300", "rank_prefix250", "rank_bdays300", "rank_lattice4096", "compact_whole_prefix"])
def test_representative_target_within_slope_times_distance(pkg, cases, name):
    ts, n, lay = make(pkg, cases, name)
    t = ts[lay.order].astype(R.LD)
    own = np.abs(t[:, None] - t[None, :])
    rp = lay.rep.astype(R.LD)
    dd = np.abs(own - np.abs(rp[lay.entry] - rp[0])).astype(np.float64)
    h = float(np.min(np.diff(np.unique(ts))))
    assert dd.max() <= 1e-11 * h * 4          # what agp_set_data admits: every point within 1e-11 spacings of its lattice position
    worst = 0.0
    for nm, nd, nz in R.sweep_programs(pkg, ts, large=True):
        tree = nd.to_tuple()
        T_own, T_rep, S = R.targets(tree, nz, ts, lay)
        _, slope = R.abs_and_slope(tree, R.sweep_elements(ts, lay, np.float64))
        diff = np.abs(T_rep - T_own).astype(np.float64)
        bound = 1.001 * slope * dd + 4 * U * S
        assert (diff <= bound).all(), (nm, float((diff / bound).max()))
        worst = max(worst, float((diff / S).max()))
    print(f"[cov-probe] {name}: worst |T_rep - T_own| / S = {worst / U:.2f} units of 2^-53, |delta d| <= {dd.max():.2e}")
