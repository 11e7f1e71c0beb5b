"""TEST INFRASTRUCTURE: a NumPy restatement of k_series_predict_logpdf (csrc/agp_series_kernel.hpp) on the kernel's own data layout —
the JOINT points (the series' training times, then its query times, no padding between), packed lower 16 x 16 blocks with block
(rb, cb) at blk_idx(rb, cb), identity rows / columns past N = n + m, the two-noise diagonal (noise below n, noise_pred in [n, N)) — in
the kernel's order of operations: the right-looking block steps with the forward solve carried along, the first non-positive pivot
as info, and the read-out restricted to the rows [n, N): ld = 2 sum log L_kk, ss = sum z_k^2, the per-point terms.  Covariance
entries come from the oracle (oracle.eval_cov): this pins the index algebra, the masks and the info rule on a machine without a GPU,
not the device's arithmetic.  Also the shared ragged case of tests/test_gpu_series_proba.py and the LDS need at the joint length."""
import functools
import math

import numpy as np

import _series_grad_ref as R
from oracle import oracle as O

BS = R.BS
blk_idx = R.blk_idx
LOG2PI = math.log(2.0 * math.pi)
N_CAP = 176

# (training points, held-out points) of the ragged call: every block count 1 .. 11, the split on a block boundary, just after one and
# just before one, the prior, nothing held out, and the cap from both ends
SHAPES = ((0, 5), (0, 176), (5, 0), (1, 1), (15, 1), (16, 16), (17, 5), (32, 1), (33, 47), (126, 18), (144, 32), (160, 16), (175, 1),
          (1, 175), (100, 76))
QUERY_KINDS = ("future", "interleaved", "training")
# SHAPES end in 1, 2, 3, 5, 9 or 11 blocks of 16 joint points: here the other final block counts (4, 6, 7, 8, 10), the split inside a block
EXTRA_SHAPES = ((40, 20), (80, 10), (100, 12), (120, 8), (150, 5))


def series_proba_lds_total(n, m, n_ops, n_prm, n_cp):
    """the kernel's LDS need in doubles: the value kernel's map (series_lds of csrc/agp_args.hpp) at the JOINT length"""
    return R.series_lds_total(n + m, n_ops, n_prm, n_cp)


def cp_chain_fits(k, n, m):
    """tests' cp_chain(G, k) — 2k + 1 nodes, 3k + 1 parameters, k tables — under the kernel's map at n + m joint points"""
    return 8 * series_proba_lds_total(n, m, 2 * k + 1, 3 * k + 1, k) <= R.LDS_BYTES


def joint_blocks(tree, noise, ts, tq, noise_pred):
    """the packed lower blocks of stage 3 and (N, nb): K on the joint points + the two-noise diagonal, identity past N"""
    n, m = len(ts), len(tq)
    N = n + m
    nb = (N + BS - 1) // BS
    npad = nb * BS
    Kp = np.eye(npad)
    if N:
        Kp[:N, :N] = O.eval_cov(tree, np.concatenate([ts, tq]))
        idx = np.arange(N)
        Kp[idx, idx] += np.where(idx < n, noise, noise_pred)
    return R.pack_lower(Kp, nb), N, nb


def series_proba_blocks(tree, noise, ts, xs, tq, y, noise_pred=None, slope=1.0):
    """(logpdf, terms[m], info) by the kernel's block algorithm; NaN in logpdf and in every term when info != 0"""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64)
    tq = np.asarray(tq, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    noise_pred = noise if noise_pred is None else noise_pred
    n, m = ts.shape[0], tq.shape[0]
    if m == 0:
        return 0.0, np.zeros(0), 0                       # (never launched)
    blk, N, nb = joint_blocks(tree, noise, ts, tq, noise_pred)
    npad = nb * BS
    r = np.zeros(npad); r[:n] = xs; r[n:N] = y           # rhs: xs, then the held-out values; padding 0
    z = np.zeros(npad)
    bad = 0
    for jb in range(nb):
        D = blk[blk_idx(jb, jb)]
        L = np.zeros((BS, BS))
        for c in range(BS):                              # the diagonal block, pivot by pivot
            d = D[c, c] - L[c, :c] @ L[c, :c]
            if not d > 0.0:
                bad = jb * BS + c + 1
                break
            L[c, c] = math.sqrt(d)
            L[c + 1:, c] = (D[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
        if bad:
            break
        blk[blk_idx(jb, jb)] = L
        W = np.linalg.inv(L)
        z[jb * BS:(jb + 1) * BS] = W @ r[jb * BS:(jb + 1) * BS]
        for ib in range(jb + 1, nb):                     # panel, then the right-hand side below the step
            blk[blk_idx(ib, jb)] = blk[blk_idx(ib, jb)] @ W.T
            r[ib * BS:(ib + 1) * BS] -= blk[blk_idx(ib, jb)] @ z[jb * BS:(jb + 1) * BS]
        for ib in range(jb + 1, nb):                     # trailing blocks
            for cb in range(jb + 1, ib + 1):
                blk[blk_idx(ib, cb)] = blk[blk_idx(ib, cb)] - blk[blk_idx(ib, jb)] @ blk[blk_idx(cb, jb)].T
    if bad:
        return math.nan, np.full(m, math.nan), bad
    rows = np.arange(npad)
    dii = np.array([blk[blk_idx(k // BS, k // BS)][k % BS, k % BS] for k in rows])
    mask = (rows >= n) & (rows < N)                      # the query rows: training rows and the identity padding stay out
    ld = 2.0 * np.log(dii[mask]).sum()
    ss = (z[mask] ** 2).sum()
    lj = math.log(abs(slope))
    lp = -0.5 * (m * LOG2PI + ld + ss) + m * lj
    terms = -0.5 * (LOG2PI + z[mask] ** 2) - np.log(dii[mask]) + lj
    return float(lp), terms, 0


def queries(kind, ts, m, rng):
    """m query times: past the series ("future"), anywhere in its range ("interleaved"), or ON training times drawn with
    replacement ("training"; an empty series takes "future")"""
    if kind == "training" and len(ts) > 0:
        return ts[rng.integers(0, len(ts), m)].copy()
    if kind == "interleaved":
        return rng.random(m)
    return 1.0 + 0.3 * np.arange(1, m + 1) / max(m, 1)


def fixture_kernels(G):
    """the fixture kernels of tests/test_gpu_predict_logpdf.py (test/test_GP.jl:24-33 and four combinations)"""
    base = [G.WhiteNoise(1), G.Constant(0.5), G.Linear(0.1, 1.3, 0.7), G.SquaredExponential(0.47, 0.13),
            G.GammaExponential(0.42, 0.58, 3.2), G.Periodic(0.96, 0.21, 1.1)]
    return base + [base[2] + base[5], base[3] * base[4], G.ChangePoint(base[2], base[5], 0.5, 0.05),
                   G.ChangePoint(base[3] + base[4], base[2] * base[5], 0.3, 0.2)]


N_PRIOR = 3


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The shared case: one series per entry of SHAPES (prefixes of shuffled synthetic series; query kind s % 3), three prior
    particles of depth <= 3 and the ten fixture kernels on each, noises in [0.05, 0.3], held-out values 0.5 N(0, 1), and a per-particle
    noise_pred — 0.3 noise (smaller than the noise) for even particles, drawn from [0.02, 0.12] for odd ones.  Computed once, never
    modified.  (series, queries, heldout, nodes, noises, sidx, noise_pred)"""
    import __graft_entry__ as g
    pkg = g.load_package()
    rng = np.random.default_rng(20261020)
    series, qs, held, nodes, noises, sidx = [], [], [], [], [], []
    for s, (n, m) in enumerate(SHAPES):
        ts, xs = pkg.prior.synthetic_series(256, seed=500 + s, shuffle=True)
        ts, xs = ts[:n].copy(), xs[:n].copy()
        series.append((ts, xs))
        qs.append(queries(QUERY_KINDS[s % 3], ts, m, rng))
        held.append(0.5 * rng.standard_normal(m))
        nd, _ = pkg.prior.sample_particles(rng, N_PRIOR, max_depth=3)
        nd = nd + fixture_kernels(pkg)
        nodes += nd; noises += list(0.05 + 0.25 * rng.random(len(nd))); sidx += [s] * len(nd)
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    P = len(nodes)
    noise_pred = np.where(np.arange(P) % 2 == 0, 0.3 * noises, 0.02 + 0.1 * rng.random(P))
    for a in (noises, sidx, noise_pred, *qs, *held):
        a.setflags(write=False)
    return series, qs, held, nodes, noises, sidx, noise_pred
