"""GRADIENT CHECKER — TEST INFRASTRUCTURE ONLY.

One assertion for every gradient comparison of the suite, component by component:

    |g_k - ref_k| <= tau * S_k          (and the same for d/dnoise with S_noise)

where S_k is component k's natural error scale (oracle.gp_logpdf_grad_scales: the sum of the magnitudes of the terms that make
up g_k).  The particle-wide criterion |g - ref|_inf <= tau * max(1, |g|_inf, |d/dnoise|) says nothing about a component whose
S_k is orders of magnitude below the particle's largest component (a small-amplitude summand, a GammaExponential's gamma, a
period, a Linear leaf inside a product); this one does.  It is checked IN ADDITION to the particle-wide one, which this helper
also asserts, so nothing is relaxed.

Against the fp64 oracle (tau = TAU_ORACLE) a miss goes to the 80-bit arbiter (oracle.gp_logpdf_grad_longdouble), per component:
the device passes where |g_k - g80_k| <= max(tau S_k, 4 |g64_k - g80_k|) (both double-precision computations form K^-1 with an
error of cond(K) eps: the device may not be more than 4x further from the 80-bit value than the fp64 oracle is).  The arbiter is
O(n^3) Python loops (about 1.3 s at n = 512, 15 s at n = 1024); above ARBITER_MAX_N it is not run and a miss is a failure.

Device-versus-device comparisons take S_k from the oracle and use TAU_PATHS (no arbiter: both sides are the device).

Floor: a component with S_k = 0 (every term of g_k is zero: a ChangePoint at scale 1e-3 whose tanh is saturated at every point,
a Linear leaf's location derivative where every derivative entry vanishes) must come back as exactly 0 or within 2^-52 of the
particle-wide scale max(1, |g_ref|_inf, |d/dnoise_ref|).  No other floor is applied.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

TAU_ORACLE = 1e-7
TAU_PATHS = 1e-9
ZERO_SCALE_FLOOR = 2.0 ** -52
ARBITER_MAX_N = 1024


class GradRef:
    """The fp64 oracle's gradient of one particle with its per-component scales; the 80-bit arbiter on demand."""

    def __init__(self, tree, noise, ts, xs):
        self.tree, self.noise = tree, float(noise)
        self.ts = np.asarray(ts, dtype=np.float64); self.xs = np.asarray(xs, dtype=np.float64)
        self.lp, self.g, self.gn, self.S, self.Sn = O.gp_logpdf_grad_scales(tree, self.noise, self.ts, self.xs)
        self._arb = None

    @property
    def n(self):
        return self.ts.shape[0]

    @property
    def particle_scale(self):
        """The particle-wide scale of the old criterion."""
        return max(1.0, np.abs(self.g).max() if self.g.size else 0.0, abs(self.gn))

    @property
    def all_g(self):
        return np.append(self.g, self.gn)

    @property
    def all_S(self):
        return np.append(self.S, self.Sn)

    def arbiter(self):
        if self._arb is None:
            gl, gnl = O.gp_logpdf_grad_longdouble(self.tree, self.noise, self.ts, self.xs)
            self._arb = np.append(gl, gnl)
        return self._arb


def reference(tree, noise, ts, xs):
    return GradRef(tree, noise, ts, xs)


def references(nodes, noises, ts, xs, threads=8):
    """GradRef of every (node, noise) of a population (nodes: oracle trees or objects with .to_tuple()); None where the oracle's
    Cholesky factorisation fails (the callers check only particles the device factored).  The oracle runs in threads (its large
    array operations and LAPACK release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    trees = [t if isinstance(t, tuple) else t.to_tuple() for t in nodes]

    def one(a):
        try:
            return GradRef(a[0], float(a[1]), ts, xs)
        except np.linalg.LinAlgError:
            return None
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, zip(trees, noises)))


def _bound(ref, tau):
    S = ref.all_S
    return np.where(S > 0, tau * S, ZERO_SCALE_FLOOR * ref.particle_scale)


def component_ratios(g, gn, ref, against=None):
    """|g_k - r_k| / S_k per component (d/dnoise last); r = the oracle, or `against` = (g2, gn2).  S_k = 0: inf unless equal."""
    got = np.append(np.asarray(g, dtype=np.float64), float(gn))
    r = ref.all_g if against is None else np.append(np.asarray(against[0], dtype=np.float64), float(against[1]))
    d = np.abs(got - r)
    S = ref.all_S
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(S > 0, d / np.where(S > 0, S, 1.0), np.where(d <= ZERO_SCALE_FLOOR * ref.particle_scale, 0.0, np.inf))


def assert_grad_components(g, gn, ref, tau=None, against=None, ctx=None, particle_wide=True):
    """Assert the gradient (g, gn) of ref's particle component by component (see the module docstring); return the worst
    |g_k - r_k| / S_k that was accepted (after arbitration: the arbitrated distance).  against=None: versus the fp64 oracle,
    tau defaults to TAU_ORACLE and misses are arbitrated; against=(g2, gn2): versus another path, tau defaults to TAU_PATHS.
    particle_wide: also assert the old criterion |g - r|_inf <= tau max(1, |g_ref|_inf, |gn_ref|) (oracle comparisons: through
    the arbiter, as before)."""
    tau = (TAU_ORACLE if against is None else TAU_PATHS) if tau is None else tau
    got = np.append(np.asarray(g, dtype=np.float64), float(gn))
    assert got.shape == ref.all_g.shape, (ctx, got.shape, ref.all_g.shape)
    r = ref.all_g if against is None else np.append(np.asarray(against[0], dtype=np.float64), float(against[1]))
    bound = _bound(ref, tau)
    d = np.abs(got - r)
    miss = ~(d <= bound)
    sc = ref.particle_scale
    wide_miss = particle_wide and not (d.max() <= tau * sc)
    if against is None and (miss.any() or wide_miss):
        assert ref.n <= ARBITER_MAX_N, (ctx, "no arbiter above n =", ARBITER_MAX_N, "components", np.flatnonzero(miss),
                                        component_ratios(g, gn, ref)[miss], "particle-wide", d.max() / sc)
        g80 = ref.arbiter()
        d80 = np.abs(got - g80)
        e64 = np.abs(ref.all_g - g80)
        ok = d80 <= np.maximum(bound, 4.0 * e64)
        if not ok[miss].all():
            bad = miss & ~ok
            with np.errstate(divide="ignore", invalid="ignore"):
                raise AssertionError((ctx, "per component", np.flatnonzero(bad), "|g - g80| / S", (d80 / ref.all_S)[bad],
                                      "|g64 - g80| / S", (e64 / ref.all_S)[bad], "S / particle scale", ref.all_S[bad] / sc))
        if wide_miss:
            assert d80.max() <= max(tau * sc, 4.0 * e64.max()), (ctx, "particle-wide", d.max() / sc, d80.max() / sc, e64.max() / sc)
        d = np.where(miss, d80, d)
    else:
        assert not miss.any(), (ctx, "per component", np.flatnonzero(miss), component_ratios(g, gn, ref, against)[miss], ref.all_S[miss] / sc)
        assert not wide_miss, (ctx, "particle-wide", d.max() / sc)
    S = ref.all_S
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(S > 0, d / np.where(S > 0, S, 1.0), 0.0)))
