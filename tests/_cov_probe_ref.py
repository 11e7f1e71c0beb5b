"""Reference side of the covariance probe (GPEngine.debug_cov_sweep, agp_debug_cov_sweep): host-only numpy, no device.

One tree evaluator (eval_tree), parametrised by dtype, gives
  * two np.longdouble TARGETS of a sweep's covariance matrix: T_own, the kernel at every element's own stored times, and T_rep,
    the same with every stationary leaf at the REPRESENTATIVE difference of the element's table entry, rep[e] - rep[0] — the rule
    in the header of csrc/agp_cov_kernel.hpp (a maximal stationary subtree is evaluated once per entry, on the "element"
    (rep[e], rep[0])); Linear leaves and ChangePoint sigmoids stay on the element's own times either way;
  * the float64 ROUTES (the oracle's vectorised and scalar forms, this evaluator in float64, and on table paths a table route:
    build each table at rep, gather by entry) whose distance to the target they aim at defines R of a (sweep, program);
  * the per-entry error scale S (error_scale): the magnitude of the terms whose rounding makes up an entry's error;
  * the host's own table layouts (sweep_layout): the sweep order, the entry of every element and the entries' times, restated from
    agp_set_data so that the device's copy can be compared bit for bit;
  * the planted faults of tests/test_cov_probe_cpu.py (Faults), each a switch inside the table route.
The device is held to |dev - target| <= MULT R S entry by entry (violations)."""
import math

import numpy as np

from oracle import oracle as O

LD = np.longdouble
U = 2.0 ** -53
MULT = 8                      # the project's multiple (oracle/predcheck.py)
R_CAP = 8 * U                 # admission: a (sweep, program) whose routes are further than this from their targets is not used
SENTINEL = -7.0
NB = 128
PI_LD = LD("3.14159265358979323846264338327950288")
TINY = 1e-300


# ---------------------------------------------------------------------------------------------------------------------------------
# trees
def is_stationary(tree):
    tag = tree[0]
    if tag in ("+", "*"):
        return is_stationary(tree[1]) and is_stationary(tree[2])
    return tag in ("SE", "GE", "PER", "C", "WN")


def is_heavy(tree):
    tag = tree[0]
    if tag in ("+", "*", "CP"):
        return is_heavy(tree[1]) or is_heavy(tree[2])
    return tag in ("SE", "GE", "PER")


def table_subtrees(tree):
    """The maximal stationary subtrees with a transcendental leaf: what a table-driven sweep tabulates (one lag table each)."""
    if is_stationary(tree):
        return [tree] if is_heavy(tree) else []
    if tree[0] in ("+", "*", "CP"):
        return table_subtrees(tree[1]) + table_subtrees(tree[2])
    return []


class Elements:
    """The elements a tree is evaluated on: row / column times (broadcastable), and what the stationary leaves see — the absolute
    difference d (None: the elements' own |tr - tc|) and where the two times are the same point (WhiteNoise)."""

    def __init__(self, tr, tc, d=None, same=None):
        self.tr, self.tc = tr, tc
        self.d = np.abs(tr - tc) if d is None else d
        self.same = (tr == tc) if same is None else same


def eval_tree(tree, X, dt, hook=None, faults=None):
    """The kernel tree on the elements X in arithmetic dt (np.float64 or np.longdouble), operations in the reference's order
    (src/GP.jl:137-140,163-166,199-203,241-245,285-289,331-336,375-377,421-423,493-501).  hook(subtree): the value of a maximal heavy
    stationary subtree from somewhere else (the table route)."""
    tag = tree[0]
    if hook is not None and is_stationary(tree) and is_heavy(tree):
        return hook(tree)
    f = dt
    if tag == "WN":
        return np.where(X.same, f(tree[1]), f(0.0)) + np.zeros(np.broadcast(X.tr, X.tc).shape, dtype=dt)
    if tag == "C":
        return np.full(np.broadcast(X.tr, X.tc).shape, f(tree[1]), dtype=dt)
    if tag == "LIN":
        return f(tree[2]) + f(tree[3]) * ((X.tr - f(tree[1])) * (X.tc - f(tree[1])))
    if tag == "SE":
        v = f(tree[2]) * np.exp(f(-0.5) * X.d * X.d / (f(tree[1]) * f(tree[1])))
        if faults is not None and faults.flush_tail:          # (a tail flushed to zero one binade early)
            v = np.where(v < f(2.0 ** -1021), f(0.0), v)
        return v
    if tag == "GE":
        return f(tree[3]) * np.exp(-((X.d / f(tree[1])) ** f(tree[2])))
    if tag == "PER":
        pi = PI_LD if dt is LD else f(math.pi)
        s = np.sin((pi / f(tree[2])) * X.d)
        return f(tree[3]) * np.exp((f(-2.0) / (f(tree[1]) * f(tree[1]))) * (s * s))
    a = eval_tree(tree[1], X, dt, hook, faults)
    b = eval_tree(tree[2], X, dt, hook, faults)
    if tag == "+":
        return a + b
    if tag == "*":
        return a * b
    if tag == "CP":
        loc, sc = f(tree[3]), f(tree[4])
        tr = X.tc if (faults is not None and faults.sigma_column) else X.tr
        si = f(0.5) * (f(1.0) + np.tanh((loc - tr) / sc))
        sj = f(0.5) * (f(1.0) + np.tanh((loc - X.tc) / sc))
        if faults is not None and faults.cp_swap:
            a, b = b, a
        return (si * sj) * a + ((f(1.0) - si) * (f(1.0) - sj)) * b
    raise ValueError(tag)


def error_scale(tree, X):
    """S of every element (float64): Constant, WhiteNoise |value|; Linear |bias| + |amp| |(ti - c)(tj - c)|; SE amp e^-x (1 + x),
    x = d^2 / 2 l^2; GammaExponential amp e^-x (1 + x (1 + |gamma log(d / l)|)), x = (d / l)^gamma; Periodic
    amp e^-x (1 + x + c u |sin 2u|), u = pi d / p, c = 2 / l^2, x = c sin^2 u; Plus adds, Times multiplies; ChangePoint
    (1 - (1 - si)(1 - sj)) S_left + (1 - si sj) S_right — the reference forms 1 - sigma by subtraction, so the far side carries an
    absolute error."""
    tag = tree[0]
    shape = np.broadcast(X.tr, X.tc).shape
    d = np.asarray(X.d, dtype=np.float64)
    if tag == "WN":
        return np.where(X.same, abs(tree[1]), 0.0) + np.zeros(shape)
    if tag == "C":
        return np.full(shape, abs(tree[1]))
    if tag == "LIN":
        tr, tc = np.asarray(X.tr, dtype=np.float64), np.asarray(X.tc, dtype=np.float64)
        return abs(tree[2]) + abs(tree[3]) * np.abs((tr - tree[1]) * (tc - tree[1]))
    if tag == "SE":
        x = d * d / (2.0 * tree[1] ** 2)
        return abs(tree[2]) * np.exp(-x) * (1.0 + x) + np.zeros(shape)
    if tag == "GE":
        x = (d / tree[1]) ** tree[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.where(d > 0, np.abs(tree[2] * np.log(np.where(d > 0, d, 1.0) / tree[1])), 0.0)
        return abs(tree[3]) * np.exp(-x) * (1.0 + x * (1.0 + lg)) + np.zeros(shape)
    if tag == "PER":
        u = math.pi * d / tree[2]
        c = 2.0 / tree[1] ** 2
        x = c * np.sin(u) ** 2
        return abs(tree[3]) * np.exp(-x) * (1.0 + x + c * u * np.abs(np.sin(2.0 * u))) + np.zeros(shape)
    a, b = error_scale(tree[1], X), error_scale(tree[2], X)
    if tag == "+":
        return a + b
    if tag == "*":
        return a * b
    if tag == "CP":
        tr, tc = np.asarray(X.tr, dtype=np.float64), np.asarray(X.tc, dtype=np.float64)
        si = 0.5 * (1.0 + np.tanh((tree[3] - tr) / tree[4]))
        sj = 0.5 * (1.0 + np.tanh((tree[3] - tc) / tree[4]))
        return (1.0 - (1.0 - si) * (1.0 - sj)) * a + (1.0 - si * sj) * b
    raise ValueError(tag)


def abs_and_slope(tree, X):
    """(|k|, an upper bound of |dk / dd|) of every element in float64, d the stationary leaves' difference: for the bound
    |T_rep - T_own| <= |dk/dd| |delta d| + 4 u S."""
    tag = tree[0]
    shape = np.broadcast(X.tr, X.tc).shape
    d = np.asarray(X.d, dtype=np.float64)
    if tag in ("WN", "C", "LIN"):
        Xd = Elements(np.asarray(X.tr, dtype=np.float64), np.asarray(X.tc, dtype=np.float64), d, X.same)
        return np.abs(eval_tree(tree, Xd, np.float64)) + np.zeros(shape), np.zeros(shape)
    if tag == "SE":
        k = abs(tree[2]) * np.exp(-0.5 * d * d / tree[1] ** 2)
        return k + np.zeros(shape), k * d / tree[1] ** 2 + np.zeros(shape)
    if tag == "GE":
        x = (d / tree[1]) ** tree[2]
        k = abs(tree[3]) * np.exp(-x)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(d > 0, k * tree[2] * x / np.where(d > 0, d, 1.0), np.where(tree[2] >= 1.0, k / tree[1], np.inf))
        return k + np.zeros(shape), g + np.zeros(shape)
    if tag == "PER":
        u = math.pi * d / tree[2]
        c = 2.0 / tree[1] ** 2
        k = abs(tree[3]) * np.exp(-c * np.sin(u) ** 2)
        return k + np.zeros(shape), k * c * np.abs(np.sin(2.0 * u)) * math.pi / tree[2] + np.zeros(shape)
    (ka, ga), (kb, gb) = abs_and_slope(tree[1], X), abs_and_slope(tree[2], X)
    if tag == "+":
        return ka + kb, ga + gb
    if tag == "*":
        return ka * kb, ga * kb + ka * gb
    if tag == "CP":          # (weights of at most 1)
        return ka + kb, ga + gb
    raise ValueError(tag)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host's layouts
def compact_fit(index_sorted):
    """(W, base) of agp_set_data's compact tables from the lattice indices of the SORTED points: base[od] the smallest lattice lag
    of two points od ordinals apart, W the most lags any ordinal difference spans."""
    gl = np.asarray(index_sorted, dtype=np.int64)
    n = gl.size
    base = np.zeros(n, dtype=np.int64)
    W = 1
    for od in range(1, n):
        lag = gl[od:] - gl[:-od]
        base[od] = lag.min()
        W = max(W, int(lag.max() - base[od] + 1))
    return W, base


class Layout:
    """How a sweep over the first n points of a resident series reads its stationary leaves (restated from agp_set_data and
    plan_tables): mode; order (the caller's position of sweep row i); entry (n, n) the table entry of every element; rep the
    entries' times; live, the entries of a table that stand for a difference between stored points."""

    def __init__(self, mode, order, entry=None, rep=None, live=None):
        self.mode, self.order, self.entry, self.rep, self.live = mode, order, entry, rep, live

    @property
    def tables(self):
        return self.mode != "general"


def sweep_layout(ts_all, n, mode, lattice):
    """lattice: probe_lattice(ts_all) of the package (the admission test of agp_set_data on its own, host code)."""
    ts_all = np.asarray(ts_all, dtype=np.float64)
    n_max = ts_all.size
    ident = np.arange(n, dtype=np.int64)
    if mode == "general":
        return Layout(mode, ident)
    perm = np.argsort(ts_all, kind="stable")
    tss = ts_all[perm]
    idx = np.asarray(lattice["index"], dtype=np.int64)
    h = lattice["spacing"]
    if mode == "sorted_lag":
        assert lattice["kind"] == 1 and n == n_max
        entry = np.abs(ident[:, None] - ident[None, :])
        return Layout(mode, perm, entry, tss.copy(), np.arange(n))
    if mode == "rank":
        assert lattice["kind"] in (1, 2)
        n_lat = lattice["n_lattice"]
        if lattice["kind"] == 1:
            rep = tss[0] + np.arange(n_lat, dtype=np.float64) * h
            rep[idx[perm]] = tss
        else:
            rep = np.arange(n_lat, dtype=np.float64) * h          # g h as ONE product
        r = idx[:n]
        return Layout(mode, ident, np.abs(r[:, None] - r[None, :]), rep, np.arange(n_lat))
    assert lattice["kind"] == 3
    W, base = compact_fit(idx[perm])
    rep = np.zeros(W * n_max)
    for off in range(W):
        rep[off::W] = (base + off).astype(np.float64) * h
    ordinal = np.empty(n_max, dtype=np.int64)
    ordinal[perm] = np.arange(n_max)
    if mode == "compact_sorted":
        assert n == n_max
        o, g, order = np.arange(n_max), idx[perm], perm
    else:
        assert mode == "compact_whole"
        o, g, order = ordinal[:n], idx[:n], ident
    od = np.abs(o[:, None] - o[None, :])
    entry = W * od + np.abs(g[:, None] - g[None, :]) - base[od]
    lay = Layout(mode, order, entry, rep, np.arange(W * n_max))
    lay.W, lay.base = W, base
    return lay


# ---------------------------------------------------------------------------------------------------------------------------------
# targets, routes, R
class Faults:
    """Planted faults of the float64 table route / evaluator (tests/test_cov_probe_cpu.py): each one is off by default."""
    corner_lag = 0             # the table read at lag g + this in ONE tile corner (a - b = 127 of tile (0, 0))
    neighbour_block = False    # sorted layout: tile (1, 0) reads the table of block lag 0
    window_rebase = 0          # compact window: the tiles with a window of their own read entry e + this
    rescaled_rep = None        # times of the lattice points as rescaled dates, t_0 + g h rounded, instead of g h
    entry255 = False           # sorted layout: the element at a - b = 127 reads entry 255 (= the table at lag 0's padding value)
    flush_tail = False
    cp_swap = False
    sigma_column = False


def sweep_elements(ts, lay, dt, rep=None):
    """Elements of the sweep's matrix in arithmetic dt: own times, and on a table path the representative differences."""
    t = np.asarray(ts, dtype=np.float64)[lay.order].astype(dt)
    tr, tc = t[:, None], t[None, :]
    if not lay.tables:
        return Elements(tr, tc)
    rp = np.asarray(lay.rep if rep is None else rep, dtype=np.float64).astype(dt)
    d = np.abs(rp[lay.entry] - rp[0])
    return Elements(tr, tc, d, tr == tc)


def add_noise(K, noise, dt):
    K = K.copy()
    K[np.diag_indices(K.shape[0])] += dt(noise)
    return K


def targets(tree, noise, ts, lay, rep=None):
    """(T_own, T_rep or None, S): the longdouble targets and the error scale of the target the sweep aims at."""
    Xo = sweep_elements(ts, Layout("general", lay.order), LD)
    T_own = add_noise(eval_tree(tree, Xo, LD), noise, LD)
    T_rep = None
    Xs = Xo
    if lay.tables:
        Xs = sweep_elements(ts, lay, LD, rep)
        T_rep = add_noise(eval_tree(tree, Xs, LD), noise, LD)
    S = error_scale(tree, Xs) + abs(noise) * np.eye(T_own.shape[0]) + TINY
    return T_own, T_rep, S


def table_route(tree, noise, ts, lay, faults=None):
    """The float64 table route: every maximal heavy stationary subtree evaluated once per entry on the element (rep[e], rep[0]),
    gathered by the elements' entries; the rest of the tree on the elements' own times."""
    t = np.asarray(ts, dtype=np.float64)[lay.order]
    n = t.size
    rep = np.asarray(lay.rep, dtype=np.float64)
    if faults is not None and faults.rescaled_rep is not None:
        rep = faults.rescaled_rep
    entry = lay.entry

    def hook(sub):
        Xt = Elements(rep, rep[0])
        tab = eval_tree(sub, Xt, np.float64, None, faults)
        e = entry.copy()
        if faults is not None:
            ti, tj = np.arange(n)[:, None] // NB, np.arange(n)[None, :] // NB
            a_b = (np.arange(n)[:, None] % NB) - (np.arange(n)[None, :] % NB)
            if faults.corner_lag:
                e[(ti == 0) & (tj == 0) & (a_b == NB - 1)] += faults.corner_lag
            if faults.neighbour_block:
                e = np.where((ti == 1) & (tj == 0), np.abs(a_b), e)
            if faults.window_rebase:
                e = np.where(ti - tj >= 1, np.minimum(e + faults.window_rebase, tab.size - 1), e)
            if faults.entry255:
                pad0 = eval_tree(sub, Elements(np.zeros(1), np.zeros(1)), np.float64)[0]          # (entry 255: evaluated at dt = 0)
                v = tab[e]
                return np.where((ti >= tj) & (a_b == NB - 1), pad0, v)
        return tab[e]
    X = Elements(t[:, None], t[None, :])
    return add_noise(eval_tree(tree, X, np.float64, hook, faults), noise, np.float64)


def sample_entries(n, k=300, seed=0):
    """A fixed sample of entries: the corners of every tile, the diagonal ends and k seeded ones."""
    edges = sorted({0, n - 1} | {b for b in range(0, n, NB)} | {b - 1 for b in range(NB, n, NB)} | {min(n - 1, b + NB - 1) for b in range(0, n, NB)})
    pairs = {(i, j) for i in edges for j in edges}
    rng = np.random.default_rng(seed + n)
    pairs |= {(int(a), int(b)) for a, b in rng.integers(0, n, size=(k, 2))}
    ij = np.array(sorted(pairs), dtype=np.int64)
    return ij[:, 0], ij[:, 1]


class Ref:
    """Targets, scale and R of one (sweep, program): target is the one the sweep aims at."""

    def __init__(self, tree, noise, ts, lay, rep=None, scalar_twin=True):
        self.tree, self.noise, self.lay = tree, noise, lay
        self.T_own, self.T_rep, self.S = targets(tree, noise, ts, lay, rep)
        self.target = self.T_rep if lay.tables else self.T_own
        t = np.asarray(ts, dtype=np.float64)[lay.order]
        n = t.size
        # the scale of the own-time target (the routes that aim at it are measured on it)
        S_own = self.S if not lay.tables else error_scale(tree, Elements(t[:, None], t[None, :])) + abs(noise) * np.eye(n) + TINY
        self.S_own = S_own
        routes = {"vectorized": (O.compute_cov_matrix_vectorized(tree, noise, t), self.T_own, S_own),
                  "float64": (add_noise(eval_tree(tree, Elements(t[:, None], t[None, :]), np.float64), noise, np.float64), self.T_own, S_own)}
        if lay.tables:
            routes["float64_rep"] = (add_noise(eval_tree(tree, sweep_elements(ts, lay, np.float64, rep), np.float64), noise, np.float64), self.T_rep, self.S)
            routes["table"] = (table_route(tree, noise, ts, lay), self.T_rep, self.S)
        self.route_err = {}
        with np.errstate(invalid="ignore"):
            for name, (K, T, S) in routes.items():
                self.route_err[name] = float(np.max(np.abs(K.astype(LD) - T) / S))
            if scalar_twin:          # (a Python double loop: on the fixed sample of entries)
                ii, jj = sample_entries(n)
                v = np.array([O.eval_cov_scalar(tree, float(t[i]), float(t[j])) + (noise if i == j else 0.0) for i, j in zip(ii, jj)])
                self.route_err["scalar"] = float(np.max(np.abs(v.astype(LD) - self.T_own[ii, jj]) / S_own[ii, jj]))
        self.R = max(self.route_err.values())

    def bound(self, mult=MULT):
        return mult * self.R * self.S


def padded_target(ref, n_pad):
    """(target, scale) of the padded tiles as they lie: the dense packer's identity pattern on the padding rows and columns (exact:
    scale 0), the sentinel above the diagonal TILES (exact)."""
    n = ref.target.shape[0]
    T = np.zeros((n_pad, n_pad), dtype=LD)
    T[:n, :n] = ref.target
    S = np.zeros((n_pad, n_pad))
    S[:n, :n] = ref.bound()
    pad = np.arange(n, n_pad)
    T[pad, pad] = 1.0
    ti = np.arange(n_pad) // NB
    upper = ti[:, None] < ti[None, :]
    T[upper] = SENTINEL
    S[upper] = 0.0
    return T, S


def violations(K_pad, ref):
    """Entries of the padded tiles (n_pad, n_pad) outside the bound: |dev - target| <= MULT R S on the live block, exact equality on
    padding and above the diagonal tiles.  -> (count, worst ratio on the live block, its (row, column))."""
    n_pad = K_pad.shape[0]
    T, B = padded_target(ref, n_pad)
    err = np.abs(K_pad.astype(LD) - T).astype(np.float64)
    bad = ~(err <= B)          # (a NaN is a violation)
    n = ref.target.shape[0]
    ti = np.arange(n) // NB
    lower = ti[:, None] >= ti[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(lower, err[:n, :n] / B[:n, :n], 0.0)
    w = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
    return int(bad.sum()), float(ratio[w]) * MULT, (int(w[0]), int(w[1]))


def pad_route(K, n_pad, pad_noise=0.0):
    """A route's live block laid out as the padded tiles (for the planted faults)."""
    n = K.shape[0]
    P = np.zeros((n_pad, n_pad))
    P[:n, :n] = K
    pad = np.arange(n, n_pad)
    P[pad, pad] = 1.0 + pad_noise
    ti = np.arange(n_pad) // NB
    P[ti[:, None] < ti[None, :]] = SENTINEL
    return P


# ---------------------------------------------------------------------------------------------------------------------------------
# programs (tuple trees of the oracle)
def chain_of(n_nodes, G):
    """A chain of n_nodes nodes (n_nodes odd): leaf (leaf binop)*, few enough tables for any sweep.  Every fourth pair rounds
    (a Linear, Periodic or Constant operand, one ChangePoint); the others scale by a power of two, each by a different one, so that
    a node record read from the wrong place moves the value by a factor of two while 64 operations do not add 64 roundings (with all
    of them rounding, the float64 routes of the 129-node chain sat at 11 units of 2^-53 S: not admitted)."""
    node = G.SquaredExponential(0.3, 1.0)
    k, expo = 0, 0
    while 2 * k + 1 < n_nodes:
        if k % 4 == 3:
            lf = (G.Linear(0.1 + 0.013 * k, 0.9, 0.2), G.Periodic(0.8, 0.23, 0.1), G.Linear(0.7 - 0.011 * k, 1.0, 0.1), G.Constant(0.05))[(k // 4) % 4]
            if k == 31:
                node = G.ChangePoint(node, lf, 0.2, 0.05)
            else:
                node = G.Times(node, lf) if (k // 4) % 4 == 2 else G.Plus(node, lf)
        else:
            a = (k % 7) + 1 if expo <= 0 else -((k % 5) + 1)          # the running exponent stays within +-7
            expo += a
            node = G.Times(node, G.Constant(2.0 ** a) if k % 2 else G.Linear(0.01 * k, 2.0 ** a, 0.0))
        k += 1
    return node


def deep_tree(G, depth=5):
    """A full binary tree of Linear leaves and products / sums: its evaluation stack need is depth + 1 (the depth-8 instantiation)."""
    count = [0]

    def rec(d):
        if d == 0:
            count[0] += 1
            k = count[0]
            return G.Linear(0.02 * k, 0.8, 0.3) if k % 3 else G.SquaredExponential(0.2 + 0.01 * k, 0.9)
        a, b = rec(d - 1), rec(d - 1)
        return G.Plus(a, b) if d % 2 else G.Times(a, b)
    return rec(depth)


def tail_kernels(G, ts):
    """SE / GammaExponential tails: the pair of points 0.8 of the series apart sits at exp(-708.0), inside the last normal binade
    [2^-1022, 2^-1021); longer differences give subnormal entries and underflow."""
    u = np.unique(ts)
    d = float(u[int(round(0.8 * (len(u) - 1)))] - u[0]) if len(u) > 1 else 1.0
    l_se = d / math.sqrt(2.0 * 708.0)
    l_ge = d / (708.0 ** (1.0 / 1.5))
    return [G.SquaredExponential(l_se, 1.0), G.GammaExponential(l_ge, 1.5, 1.0),
            G.SquaredExponential(l_se, 1.0) + G.Constant(1e-3)], [1e-4, 1e-3, 1e-2]


# ---------------------------------------------------------------------------------------------------------------------------------
# the sweeps the GPU tests probe (tests/test_gpu_cov_probe.py), admitted on the CPU by tests/test_cov_probe_cpu.py
def irregular_series(n, seed):
    """Irregular times in [0, 1] with one duplicated point (n > 3)."""
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.random(n))
    if n > 3:
        ts[n // 2] = ts[n // 2 - 1]
    xs = 0.5 * rng.standard_normal(n) + np.sin(6 * ts)
    return ts, xs


def lattice_subset(n, n_lat, seed):
    """n points of an n_lat-point lattice of spacing 2^-12 from 0: both ends, two neighbours, the rest seeded; shuffled."""
    rng = np.random.default_rng(seed)
    g = np.concatenate([[0, 1, n_lat - 1], 2 + rng.choice(n_lat - 3, size=n - 3, replace=False)])
    g = rng.permutation(g)
    ts = g.astype(np.float64) / 4096.0          # (a spacing of 2^-12: every time and every difference is exact)
    return ts, np.sin(5 * ts) + 0.1 * rng.standard_normal(n)


def compact_switch(prior):
    """The sizes on either side of the whole / window switch of the compact tables on month starts: the largest n_max with
    W n_max <= 4096 entries (16 LDS units of 256), and the next."""
    best = None
    for W in range(1, 9):
        n = 4096 // W
        if n > 4000:
            continue
        ts, _ = prior.calendar_series(n, freq="M", seed=34)
        x = np.round((ts - ts[0]) / np.min(np.diff(ts)) * 28.0)          # day counts of month starts (shortest month: 28 days)
        if compact_fit(x.astype(np.int64))[0] == W:
            best = n
    assert best is not None
    return best, best + 1


# name -> (series builder(prior), prefix n or None, the TableMode the sweep must report, keyword arguments of debug_cov_sweep)
def sweep_cases(prior):
    n_whole, n_sorted = compact_switch(prior)
    cases = {}
    for n in (1, 2, 127, 128, 129, 257):
        cases[f"irregular{n}"] = (lambda n=n: irregular_series(n, 1000 + n), None, "general", dict(allow_tables=n != 2))
    for n in (129, 256, 300):
        cases[f"sorted{n}"] = (lambda n=n: prior.synthetic_series(n, seed=40 + n, shuffle=True), None, "sorted_lag", {})
    for n in (250, 129):
        cases[f"rank_prefix{n}"] = (lambda: prior.synthetic_series(300, seed=31, shuffle=True), n, "rank", {})
    cases["rank_gradient300"] = (lambda: prior.synthetic_series(300, seed=31, shuffle=True), None, "rank", dict(for_gradient=True))
    for n in (256, 257):
        cases[f"rank_units{n}"] = (lambda n=n: prior.synthetic_series(n, seed=50 + n, shuffle=True), None, "rank", dict(for_gradient=True))
    cases["rank_bdays300"] = (lambda: prior.calendar_series(300, freq="B", seed=33), None, "rank", {})
    cases["rank_lattice4096"] = (lambda: lattice_subset(300, 4096, 7), None, "rank", {})
    cases["general_lattice4097"] = (lambda: lattice_subset(300, 4097, 7), None, "general", {})
    cases["compact_whole"] = (lambda: prior.calendar_series(n_whole, freq="M", seed=34), None, "compact_whole", {})
    cases["compact_whole_prefix"] = (lambda: prior.calendar_series(n_whole, freq="M", seed=34, shuffle=True), 200, "compact_whole", {})
    cases["compact_sorted"] = (lambda: prior.calendar_series(n_sorted, freq="M", seed=34, shuffle=True), None, "compact_sorted", {})
    return cases


LARGE_CASES = ("compact_whole", "compact_sorted")      # ~1000 points: a subset of the programs keeps each test to seconds


def sweep_programs(G, ts, large=False, for_gradient=False):
    """(name, node, noise) of every program of a sweep: programs() of tests/test_gpu_chain_builder.py, small_kernels() of
    tests/test_gpu_grad_components.py, chains of 65 and 129 nodes (the chunk boundaries of stage_node_records), a tree that needs
    the depth-8 stack, and the tails.  for_gradient: without the two long chains (a gradient sweep takes trees of up to 64 nodes)."""
    from test_gpu_chain_builder import programs
    from test_gpu_grad_components import small_kernels
    out = []
    chain = programs(G)
    out += [(f"chain{i}", nd, 0.05 + 0.01 * i) for i, nd in enumerate(chain)]
    small, noises = small_kernels(G, np.asarray(ts), duplicates=True)
    out += [(f"small{i}", nd, float(z)) for i, (nd, z) in enumerate(zip(small, noises))]
    out += [("chain65", chain_of(65, G), 0.1), ("chain129", chain_of(129, G), 0.1), ("deep8", deep_tree(G), 0.1)]
    tails, tz = tail_kernels(G, np.asarray(ts))
    out += [(f"tail{i}", nd, z) for i, (nd, z) in enumerate(zip(tails, tz))]
    if for_gradient:
        out = [r for r in out if r[0] not in ("chain65", "chain129")]
    if large:
        keep = {"chain2", "chain19", "chain40", "chain41", "chain42", "small2", "small5", "small11", "chain65", "deep8", "tail0"}
        out = [r for r in out if r[0] in keep]
    return out


GROUPS = ("a", "b", "deep")


def program_group(progs, group):
    """The batches a sweep's programs are probed in.  One program that needs more than four stack slots puts its whole batch on the
    depth-8 instantiation of the tile builder, which has the stack interpreter only: "deep" is that program with every fifth of
    the others beside it; "a" and "b" halve the rest (depth <= 4: chains are decoded in place)."""
    rest = [r for r in progs if r[0] != "deep8"]
    if group == "deep":
        return [r for r in progs if r[0] == "deep8"] + rest[::5]
    return rest[0::2] if group == "a" else rest[1::2]
