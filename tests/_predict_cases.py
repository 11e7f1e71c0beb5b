"""TEST INFRASTRUCTURE: the cases of tests/test_gpu_predict_components.py and of the cap test of tests/test_predcheck_cpu.py — series,
query times, particles — and their references (oracle/predcheck.py), computed once per process and never modified.

Family: nine kernels (a short and a long length scale, a summand 1e-3 of its neighbour, a product with a Linear summand, a
GammaExponential with and without WhiteNoise, a lone Linear, an amplitude of 1e-4, a ChangePoint) at noise 1e-5 (the model's
jitter), 1e-3 and 0.1; noise_pred = 0 unless the case says otherwise.  Queries: every 7th training time, every 9th midpoint between
neighbouring times, five times after the series (lattice cases: lattice points only — on the business-day calendar the weekend
days between training days)."""
import functools
import re
from pathlib import Path

import numpy as np

from oracle import predcheck as PC

NOISES = (1e-5, 1e-3, 0.1)
POPULATION_NOISES = tuple(np.geomspace(1e-5, 0.1, 8))
STRUCTURED_NOISES = tuple(np.geomspace(1e-5, 0.1, 5))         # 40 particles of the Toeplitz class (STRUCT_PRED_MIN_CLASS below)


def csrc_constant(header, name):
    """`constexpr int name = value;` of a header of the engine's sources: the thresholds the cases sit on are read, not copied"""
    text = (Path(__file__).resolve().parent.parent / "autogp.jl_amd" / "csrc" / header).read_text()
    found = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert found, (header, name)
    return int(found.group(1))


# agp_predict.hip split_queries: the diag(K^-1) route is taken (no covariance requested, n >= 2 NB, m >= NB) once the queries that are
# training times number at least NB (the tile edge) and at least n / 3
TRAIN_ROUTE_MIN = csrc_constant("agp_common.hpp", "NB")
STRUCT_PRED_MIN_CLASS = csrc_constant("agp_host.hpp", "STRUCT_PRED_MIN_CLASS")              # the structured pass wants that many particles of its class
RIGHT_LOOKING_MAX_PARTICLES = csrc_constant("agp_host.hpp", "RIGHT_LOOKING_MAX_PARTICLES")  # above it: no small-batch schedule
SMALL_AMPLITUDE = 5          # index of Constant(1e-4) * SE(0.2, 1.0) in family()


@functools.lru_cache(maxsize=None)
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def family():
    G = pkg()
    SE = G.SquaredExponential
    return [SE(0.1, 0.8),
            SE(0.3, 1.0) + SE(0.05, 1e-3),
            G.Periodic(0.7, 0.21, 1.1) * SE(0.5, 0.9) + G.Linear(0.3, 0.2, 0.5),
            G.GammaExponential(0.3, 1.2, 0.7),
            G.Linear(0.1, 0.3, 0.7),
            G.Constant(1e-4) * SE(0.2, 1.0),
            G.ChangePoint(G.Periodic(0.5, 0.1, 1.0), SE(0.2, 0.6), 0.45, 0.01),
            G.GammaExponential(0.3, 1.2, 0.7) + G.WhiteNoise(0.05),
            SE(2.0, 1.0)]


N_TOEPLITZ_CLASS = 8         # all of family() but the ChangePoint (agp_host.hpp toeplitz_class)


def particles(noises=NOISES):
    """(nodes, noises): every kernel of the family at every noise, kernel-major"""
    fam = family()
    return [k for k in fam for _ in noises], np.array([nz for _ in fam for nz in noises], dtype=np.float64)


def signal(ts, rng):
    return np.cos(9 * ts) + 0.3 * ts + 0.1 * rng.standard_normal(ts.shape[0])


def irregular_series(n, seed):
    """sorted irregular times with one duplicated time"""
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.random(n))
    if n > 3:
        ts[n // 2] = ts[n // 2 - 1]
    return ts, signal(ts, rng)


def general_queries(ts):
    u = np.unique(ts)
    h = (u[-1] - u[0]) / max(1, len(u) - 1)
    mid = (0.5 * (u[:-1] + u[1:]))[::9]
    return np.concatenate([ts[::7], mid, u[-1] + h * np.arange(1, 6)])


def lattice_queries(ts, h, before=0):
    """every 7th training time, five grid points after the series (and `before` grid points before it: a query before the series
    keeps the call off the structured pass)"""
    return np.concatenate([ts[::7], ts.max() + h * np.arange(1, 6), ts.min() - h * np.arange(1, before + 1)])


def business_days(n, seed):
    """(ts, xs, tq) of n shuffled business days as GPModel rescales them (min-max over the observed dates, slope * x + intercept) and
    queries on the lattice of days: every 7th training day, every 9th weekend day between them, the five business days that follow"""
    G = pkg()
    x = G.prior.datetime2unix(G.prior.calendar_dates(n + 5, "B"))
    slope, icpt = G.prior.linear_transform_minmax(x[:n])
    _, xs = G.prior.calendar_series(n, "B", seed=seed)
    perm = np.random.default_rng(seed).permutation(n)
    ts = np.ascontiguousarray((slope * x[:n] + icpt)[perm]); xs = np.ascontiguousarray(xs[perm])
    day = 86400.0
    free = np.setdiff1d(np.arange(int(round((x[n - 1] - x[0]) / day)) + 1), np.rint((x[:n] - x[0]) / day).astype(np.int64))
    tq = np.concatenate([ts[::7], slope * (x[0] + day * free[::9]) + icpt, slope * x[n:] + icpt])
    return ts, xs, tq


def mean_fn(t):
    return 0.4 - 1.3 * t


class Case:
    def __init__(self, name, ts, xs, n, tq, noises=NOISES, noise_pred=0.0, mean=None, want_cov=False):
        self.name, self.ts, self.xs, self.n, self.tq, self.mean, self.want_cov = name, ts, xs, int(n), tq, mean, want_cov
        self.nodes, self.noises = particles(noises)
        self.noise_pred = np.broadcast_to(np.asarray(noise_pred, dtype=np.float64), self.noises.shape).copy()
        for a in (self.ts, self.xs, self.tq, self.noises, self.noise_pred):
            a.setflags(write=False)
        self._refs = None

    @property
    def means_kw(self):
        if self.mean is None:
            return {}
        return dict(mean_train=np.array([self.mean(t) for t in self.ts[:self.n]]), mean_pred=np.array([self.mean(t) for t in self.tq]))

    def refs(self):
        if self._refs is None:
            self._refs = PC.references(self.nodes, self.noises, self.ts[:self.n], self.xs[:self.n], self.tq, self.noise_pred,
                                       mean=self.mean, want_cov=self.want_cov)
        return self._refs


def _build():
    G = pkg()
    out = {}

    def add(c):
        out[c.name] = c
    # 1. general joint path: one padded tile, two tiles, three tile rows with a ragged last row
    for n in (17, 129, 300):
        ts, xs = irregular_series(n, seed=100 + n)
        add(Case(f"joint_{n}", ts, xs, n, general_queries(ts), want_cov=True))
    # (mean functions and noise_pred on the series of joint_129 / joint_17: what differs from those cases is the argument alone)
    ts, xs = out["joint_129"].ts, out["joint_129"].xs
    add(Case("joint_means_129", ts, xs, 129, general_queries(ts), mean=mean_fn, want_cov=True))
    ts, xs = out["joint_17"].ts, out["joint_17"].xs
    add(Case("joint_noise_pred_17", ts, xs, 17, general_queries(ts), noise_pred=0.5 * particles()[1] + 0.02, want_cov=True))
    # 2. training-point route: joint_300's series, training-time queries up to the threshold and one fewer
    ts, xs = out["joint_300"].ts, out["joint_300"].xs
    base = general_queries(ts)
    n_train = ts[::7].shape[0]
    extra = np.setdiff1d(np.arange(300), np.arange(0, 300, 7))
    for k, name in ((TRAIN_ROUTE_MIN, "train_route_300"), (TRAIN_ROUTE_MIN - 1, "train_route_below_300")):
        add(Case(name, ts, xs, 300, np.concatenate([base, ts[extra[:k - n_train]]])))
    # 5. resident factors: joint_300 itself and a prefix n < n_max of it
    add(Case("resident_prefix_200", ts, xs, 200, general_queries(ts[:200])))
    # 3. lattice pass on rank tables: a shuffled regular grid and a business-day calendar
    ts, xs = G.prior.synthetic_series(300, seed=31, shuffle=True)
    tq = lattice_queries(ts, 1.0 / 299, before=2)
    add(Case("lattice_grid_300", ts, xs, 300, tq))
    # 6. population schedules: the same series and queries, 72 distinct particles
    add(Case("population_300", ts, xs, 300, tq, noises=POPULATION_NOISES))
    ts, xs, tq = business_days(300, seed=11)
    add(Case("lattice_business_days_300", ts, xs, 300, tq))
    # 4. structured pass: the whole of a grid (consecutive points), marginals, at least STRUCT_PRED_MIN_CLASS = 32 particles of the class
    ts, xs = G.prior.synthetic_series(420, seed=41, shuffle=True)
    add(Case("structured_420", ts, xs, 420, lattice_queries(ts, 1.0 / 419), noises=STRUCTURED_NOISES))
    # 7. the short-series kernel: joint_17 and two longer series, the longest at the kernel's cap — prefixes of shuffled 256-point
    # series, the data of the short-series suite's own ragged case (_series_predict_ref.ragged_case)
    for s, n in enumerate((144, G.SERIES_MAX_N)):
        ts, xs = G.prior.synthetic_series(256, seed=301 + s, shuffle=True)
        add(Case(f"series_{n}", ts[:n].copy(), xs[:n].copy(), n, general_queries(ts[:n])))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


CASE_NAMES = ("joint_17", "joint_129", "joint_300", "joint_means_129", "joint_noise_pred_17", "train_route_300", "train_route_below_300",
              "resident_prefix_200", "lattice_grid_300", "population_300", "lattice_business_days_300", "structured_420", "series_144",
              "series_176")


def case(name):
    return cases()[name]
