"""CPU checks of the sum-of-products decomposition (src/GP.jl:520-660; src/api.jl:898-1034): the host tree rewrites
split_kernel_sop / extract_kernel against the reference's own cases, the additivity of the split covariances, the fp64 inverse
normal CDF of csrc/agp_ndtri.hpp against mpmath, and the numpy restatement of predict_mvn_sum / predict_sum that the GPU tests use."""
import ctypes
import subprocess
import sys
from pathlib import Path

import mpmath as mp
import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _sum_decomposition_ref as R      # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


# ---- tree rewrites ---------------------------------------------------------------------------------------------------------

def test_split_kernel_sop_reference_cases(pkg):
    """test/test_GP.jl:108-146, tree for tree (the Times expansion's term order included)."""
    G = pkg
    l, w, p, g = G.Linear(1), G.WhiteNoise(1), G.Periodic(1, 1), G.GammaExponential(1, 1)
    p2, l2 = G.Periodic(2, 1), G.Linear(2)
    s = G.Constant(0)
    bases = [G.WhiteNoise(0.3), G.Constant(0.7), G.Linear(0.2, 0.1, 0.6), G.SquaredExponential(0.3, 0.8),
             G.GammaExponential(0.4, 1.3, 0.7), G.Periodic(0.5, 0.2, 0.4)]
    for b in bases:
        assert G.split_kernel_sop(b, type(b)) == (b, s)
        for j in bases:
            if type(j) is not type(b):
                assert G.split_kernel_sop(b, type(j)) == (s, b)
    assert G.split_kernel_sop(l * l + p * l + g * w, G.Linear) == (l * l + p * l, g * w)
    assert G.split_kernel_sop(l * (l + p + g), G.Periodic) == (l * p, l * (l + g))
    assert G.split_kernel_sop((l * p) * (l + g), G.Periodic) == ((l * p) * (l + g), s)
    assert G.split_kernel_sop((l + p) * (g + l), G.Periodic) == (p * (g + l), l * (g + l))
    assert G.split_kernel_sop((l + p) * (p2 + l2), G.Periodic) == (p * p2 + p * l2 + l * p2, l * l2)
    k = G.ChangePoint(p * l + l, p * p + g, 1, 1)
    assert G.split_kernel_sop(k, G.WhiteNoise) == (s, k)
    assert G.split_kernel_sop(k, G.GammaExponential) == (G.ChangePoint(s, g, 1, 1), G.ChangePoint(p * l + l, p * p, 1, 1))
    k = G.ChangePoint(l, p, 1, 1)
    assert G.split_kernel_sop(k, G.WhiteNoise) == (s, k)
    assert G.split_kernel_sop(k, G.Linear) == (G.ChangePoint(l, s, 1, 1), G.ChangePoint(s, p, 1, 1))


def test_split_kernel_sop_docstring_examples(pkg):
    """src/GP.jl:591-600; the last example's sum is ((p*p + p*l) + l*p), the order the expansion produces."""
    G = pkg
    l, p, c = G.Linear(1), G.Periodic(1, 1), G.Constant(1)
    s = G.Constant(0)
    assert G.split_kernel_sop(l, G.Linear) == (l, s)
    assert G.split_kernel_sop(l, G.Periodic) == (s, l)
    assert G.split_kernel_sop(l * p + l * c, G.Periodic) == (l * p, l * c)
    assert G.split_kernel_sop(p * p, G.Periodic) == (p * p, s)
    a, b = G.split_kernel_sop((l + p) * (l + p), G.Periodic)
    assert a == G.Plus(G.Plus(G.Times(p, p), G.Times(p, l)), G.Times(l, p)) and b == G.Times(l, l)
    assert a != G.Plus(G.Times(p, p), G.Plus(G.Times(p, l), G.Times(l, p)))      # (the shape, not only the set of terms)


def test_extract_kernel(pkg):
    """src/GP.jl:520-561: Constant(1) under Times, Constant(0) under Plus and ChangePoint, Constant(0) for an empty result."""
    G = pkg
    l, p, g = G.Linear(1), G.Periodic(1, 1), G.GammaExponential(1, 1)
    c0, c1 = G.Constant(0), G.Constant(1)
    assert G.extract_kernel(l * p + g, G.Periodic) == c1 * p + c0
    assert G.extract_kernel(l * p + g, G.Periodic, retain=False) == l * c1 + g
    assert G.extract_kernel(p, G.Periodic) == p
    assert G.extract_kernel(p, G.Periodic, retain=False) == c0
    assert G.extract_kernel(l, G.Periodic) == c0
    assert G.extract_kernel(G.ChangePoint(l, p, 0.3, 0.1), G.Linear) == G.ChangePoint(l, c0, 0.3, 0.1)
    assert G.extract_kernel(G.ChangePoint(l, p, 0.3, 0.1), G.Linear, retain=False) == G.ChangePoint(c0, p, 0.3, 0.1)
    assert G.extract_kernel(l * l, G.Periodic) == c1 * c1


LEAVES = ("WhiteNoise", "Constant", "Linear", "SquaredExponential", "GammaExponential", "Periodic")


@pytest.mark.parametrize("leaf", LEAVES)
def test_split_covariances_add_up(pkg, leaf):
    """For random prior populations: cov(k_a) + cov(k_b) == cov(k) (oracle covariance), and each side of the split holds a leaf of
    the type (k_a) or none (k_b) — up to the Constant(0) sentinel."""
    G = pkg
    T = getattr(G, leaf)
    rng = np.random.default_rng(LEAVES.index(leaf))
    nodes, _ = G.prior.sample_particles(rng, 60)
    ts = np.concatenate([np.sort(rng.random(40)), [0.5, 0.5]])          # (a repeated time: the WhiteNoise terms)

    def leaves(nd):
        return [x for x in G.unroll(nd) if isinstance(x, G.LeafNode)]
    for nd in nodes:
        a, b = G.split_kernel_sop(nd, T)
        Ka, Kb, K = (O.eval_cov(x.to_tuple(), ts) for x in (a, b, nd))
        assert np.abs(Ka + Kb - K).max() <= 1e-12 * max(1.0, np.abs(K).max()), (nd, a, b)
        assert all(not isinstance(x, T) for x in leaves(b))
        assert a == G.Constant(0) or any(isinstance(x, T) for x in leaves(a))


# ---- inverse normal CDF --------------------------------------------------------------------------------------------------

NDTRI_SRC = r'''
#include "agp_ndtri.hpp"
extern "C" {
void v_ndtri(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = agp::ndtri(x[i]); }
double bound() { return agp::AGP_NDTRI_REL_BOUND; }
}
'''


@pytest.fixture(scope="module")
def ndtri_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ndtri")
    (d / "nd.cpp").write_text(NDTRI_SRC)
    so = d / "libnd.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(ROOT / "autogp.jl_amd" / "csrc"),
                    "-o", str(so), str(d / "nd.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    lib.bound.restype = ctypes.c_double
    return lib


def ndtri(lib, q):
    q = np.ascontiguousarray(q, dtype=np.float64); z = np.empty_like(q)
    lib.v_ndtri(q.ctypes.data_as(ctypes.c_void_p), z.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(q.size))
    return z


def mp_ndtri(q, z0):
    """The exact quantile of the double q: the root of Phi(z) = q at 40 digits, started from z0."""
    if q == 0.5:
        return 0.0
    qq = mp.mpf(float(q))
    return float(mp.findroot(lambda z: mp.erfc(-z / mp.sqrt(2)) / 2 - qq, mp.mpf(float(z0))))


def test_ndtri_against_mpmath(ndtri_lib):
    """q in [1e-300, 1 - 1e-16], log-spaced into both tails and linear across the middle: relative error within the header's
    stated bound (absolute near q = 1/2)."""
    mp.mp.dps = 40
    rng = np.random.default_rng(3)
    q = np.concatenate([np.logspace(-300, -1, 700), np.linspace(1e-6, 1 - 1e-6, 700), 1 - np.logspace(-16, -1, 300),
                        rng.random(300), [1e-300, 0.5, 0.5 + 2 ** -53, 0.425 + 0.5, 0.075, 1 - 1e-16, np.exp(-25.0)]])
    z = ndtri(ndtri_lib, q)
    ref = np.array([mp_ndtri(v, z0) for v, z0 in zip(q, z)])
    err = np.abs(z - ref) / np.maximum(np.abs(ref), 1.0 / 8)
    bound = ndtri_lib.bound()
    print("ndtri: max error", err.max(), "at q =", q[np.argmax(err)])
    assert err.max() <= bound, (err.max(), q[np.argmax(err)])
    assert ndtri(ndtri_lib, [0.5])[0] == 0.0
    x = ndtri(ndtri_lib, [0.0, 1.0, -0.1, 1.1, np.nan])
    assert x[0] == -np.inf and x[1] == np.inf and np.isnan(x[2:]).all()


# ---- restatement of predict_mvn_sum / predict_sum -------------------------------------------------------------------------

def _population(pkg, seed, P=5, n=40, p=7):
    G = pkg
    rng = np.random.default_rng(seed)
    nodes, noises = G.prior.sample_particles(rng, P, max_depth=3)
    noises = np.maximum(noises, 0.05)
    ts = np.sort(rng.random(n)); xs = 0.4 * rng.standard_normal(n); tp = np.linspace(0.0, 1.3, p)
    return nodes, noises, ts, xs, tp


def test_restatement_matches_oracle_infer_gp_sum(pkg):
    """Raw means: (mu - b)/a, + b/a on F_1 only; the raw Y mean is the sum of the raw component means (the intercept counted once);
    covariance scaled by 1/a^2; quantiles are oracle.quantile of the raw marginals, the median the mean."""
    G = pkg
    nodes, noises, ts, xs, tp = _population(pkg, 1)
    a, b = 2.5, -0.7
    splits = [[x.to_tuple() for x in G.split_kernel_sop(nd, G.Periodic)] for nd in nodes]
    comps, idx = R.predict_mvn_sum(splits, noises, ts, xs, tp, y_transform=(a, b))
    p = tp.shape[0]
    assert idx["Y"] == slice(2 * p, 3 * p) and idx["F"] == [slice(0, p), slice(p, 2 * p)]
    for (mr, Sr), sp, nz in zip(comps, splits, noises):
        mu, S, iF, iX = O.infer_gp_sum(sp, nz, ts, xs, tp)
        assert np.array_equal(mr[iF[1]], (mu[iF[1]] - b) / a) and np.array_equal(mr[iX], (mu[iX] - b) / a)
        assert np.array_equal(mr[iF[0]], (mu[iF[0]] - b) / a + b / a)
        assert np.abs(mr[iF[0]] + mr[iF[1]] - mr[iX]).max() <= 1e-9 * max(1.0, np.abs(mr).max())
        assert np.array_equal(Sr, (1.0 / (a * a)) * S)
    lw = np.linspace(-1.0, 0.5, len(nodes))
    cols = R.predict_sum(splits, noises, lw, ts, xs, tp, y_transform=(a, b), quantiles=[0.1, 0.5, 0.9])
    assert list(cols) == ["ds", "y_mean", "component", "particle", "weight", "y_0.1", "y_0.5", "y_0.9"]
    P = len(nodes)
    assert cols["y_mean"].shape == (3 * P * p,)
    assert np.array_equal(cols["component"], np.tile(np.repeat([0, 1, 2], p), P))
    assert np.array_equal(cols["particle"], np.repeat(np.arange(1, P + 1), 3 * p))
    assert np.allclose(cols["weight"][::p][::3], O.particle_weights(lw))
    assert np.array_equal(cols["y_0.5"], cols["y_mean"])
    assert (cols["y_0.1"] <= cols["y_mean"]).all() and (cols["y_0.9"] >= cols["y_mean"]).all()
    mr, Sr = comps[2]
    assert np.array_equal(cols["y_mean"][6 * p:7 * p], mr[idx["Y"]])          # particle 3, component 0: the observable rows
    assert np.array_equal(cols["y_mean"][7 * p:8 * p], mr[idx["F"][0]])


class _RestatedEngine:
    """Stands in for GPEngine.predict_sum_batch / infer_gp_sum_batch with the restatement (the module functions' shaping only)."""

    def __init__(self, ts, xs):
        self.ts, self.xs = ts, xs

    def predict_sum_batch(self, split, noises, ts_pred, q=(), noise_pred=None, y_transform=(1.0, 0.0)):
        comps, _ = R.predict_mvn_sum([[x.to_tuple() for x in s] for s in split], noises, self.ts, self.xs, ts_pred, y_transform,
                                     noise_pred)
        mean = np.array([m for m, _ in comps])
        x = np.array([O.quantile(m, S, list(q)) if len(q) else np.zeros((m.shape[0], 0)) for m, S in comps])
        return mean, x, np.zeros(len(comps), dtype=np.int32)

    def infer_gp_sum_batch(self, split, noises, ts_pred, noise_pred=None, want_cov=False):
        out = [O.infer_gp_sum([x.to_tuple() for x in s], nz, self.ts, self.xs, ts_pred, noise_pred=noise_pred)
               for s, nz in zip(split, noises)]
        mean = np.array([o[0] for o in out]); cov = np.array([o[1] for o in out])
        return mean, np.diagonal(cov, axis1=1, axis2=2).copy(), cov, np.zeros(len(out), np.int32), out[0][2], out[0][3]


def test_module_functions_shape_like_the_reference(pkg):
    """predict_sum / predict_mvn_sum of the package: columns, row order, weights and the raw transform as the restatement."""
    G = pkg
    nodes, noises, ts, xs, tp = _population(pkg, 2, P=4, p=5)
    lw = np.array([-0.3, 0.0, -2.0, -1.0])
    eng = _RestatedEngine(ts, xs)
    cols = G.predict_sum(eng, nodes, noises, lw, tp, G.Linear, y_transform=(3.0, 1.5), noise_pred=0.02, quantiles=[0.25, 0.75])
    splits = [[x.to_tuple() for x in G.split_kernel_sop(nd, G.Linear)] for nd in nodes]
    ref = R.predict_sum(splits, noises, lw, ts, xs, tp, y_transform=(3.0, 1.5), noise_pred=0.02, quantiles=[0.25, 0.75])
    assert list(cols) == list(ref)
    for k in ref:
        assert np.allclose(cols[k], ref[k], rtol=1e-12, atol=0.0), k
    comps, w, idx = G.predict_mvn_sum(eng, nodes, noises, lw, tp, G.Linear, y_transform=(3.0, 1.5))
    rc, ridx = R.predict_mvn_sum(splits, noises, ts, xs, tp, y_transform=(3.0, 1.5))
    assert idx == ridx and np.allclose(w, O.particle_weights(lw), rtol=1e-14)
    for d, (m, S) in zip(comps, rc):
        assert np.array_equal(d.mean(), m) and np.array_equal(d.cov(), S)
