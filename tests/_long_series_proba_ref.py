"""TEST INFRASTRUCTURE of the long held-out entry (agp_predict_logpdf_long_series_batch; k_long_series_predict_logpdf,
csrc/agp_long_series_kernel.hpp):

  * long_series_proba_blocks: a NumPy restatement of the kernel on its own data layout and in its order — the JOINT points (the
    series' training times, then its query times, no padding between), packed lower 16 x 16 blocks with block (rb, cb) at
    blk_idx(rb, cb), the two-noise diagonal (noise below n, noise_pred in [n, N)), identity rows / columns past N = n + m
    (_series_proba_ref.joint_blocks); the factorisation LEFT-looking by block columns with the forward solve and 2 log L_kk of every
    row carried along — S(ib, j) = K(ib, j) - sum_{k<j} L(ib, k) L(j, k)', the diagonal block pivot by pivot, the panel S W', z_j = W
    r_j, r_ib -= L(ib, j) z_j —; the read-out over the rows [n, N) alone; the first non-positive pivot on the joint index as info.
    Covariance entries come from the oracle (oracle.eval_cov): this pins the index algebra, the masks, the read-out and the info rule
    on a machine without a GPU, not the device's arithmetic.
  * the LDS need at the joint length: the long value kernel's map (long_series_lds of csrc/agp_args.hpp) at N points;
  * the shared ragged case of tests/test_gpu_long_series_proba.py and the bad-pivot case on joint times split at 300."""
import functools
import math

import numpy as np

import _long_series_predict_ref as LP
import _series_cases as SC
import _series_grad_ref as R
import _series_proba_ref as SPR

BS = R.BS
blk_idx = R.blk_idx
LOG2PI = SPR.LOG2PI
N_SHORT = 176                                   # AGP_SERIES_MAX_N: joint lengths up to here take the short kernel
N_CAP = LP.LONG_SERIES_MAX_N                     # AGP_LONG_SERIES_MAX_N

# (training points, held-out points).  Short-routed: the prior, nothing held out, a tutorial split, the short cap
SHAPES_SHORT = ((0, 5), (5, 0), (126, 18), (175, 1))
# both sides of the short cap (from either end, and the prior) and of the block boundaries 176 / 177 of the split
SHAPES_CAP = ((176, 1), (1, 176), (0, 177), (144, 36), (160, 17), (161, 16), (175, 2))
# the long_update bodies of tests/_long_series_cases.py (N = 337, 401, 465, 497, 512): C = 6, 7, 8, 32 block rows with one real row in
# the last — the query row —, the 442-point data set's length as the TRAINING part, and the cap as the prior, from above and from below
SHAPES_LONG = ((300, 37), (385, 16), (400, 65), (496, 1), (442, 70), (0, 512), (511, 1), (1, 511))
# short-routed by default; under AGP_LONG_SERIES_ALL the long kernel at N = 2, 16, 17, 65, 81: one ragged block, a full block, the
# first long_update, a fifth block row, the first C = 2
SHAPES_ALL = ((1, 1), (15, 1), (16, 1), (17, 48), (33, 48))
SHAPES = SHAPES_SHORT + SHAPES_CAP + SHAPES_LONG + SHAPES_ALL
QUERY_KINDS = SPR.QUERY_KINDS


def long_series_proba_lds_total(n, m, n_ops, n_prm, n_cp):
    """the long route's LDS need in doubles: long_series_lds(n + m, ..).total of csrc/agp_args.hpp"""
    return LP.long_series_lds_total(n + m, n_ops, n_prm, n_cp)


def cp_chain_fits(k, n, m):
    """tests' cp_chain(G, k) — 2k + 1 nodes, 3k + 1 parameters, k tables — under the long kernel's map at n + m joint points"""
    return 8 * long_series_proba_lds_total(n, m, 2 * k + 1, 3 * k + 1, k) <= R.LDS_BYTES


def long_route(n, m, all_long=False):
    """does a particle of a series with n training and m held-out points take the long kernel?  (m == 0: never launched)"""
    return m > 0 and (n + m > N_SHORT or all_long)


def long_series_proba_blocks(tree, noise, ts, xs, tq, y, noise_pred=None, slope=1.0):
    """(logpdf, terms[m], info) by the kernel's block algorithm; NaN in logpdf and in every term when info != 0"""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64)
    tq = np.asarray(tq, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    noise_pred = noise if noise_pred is None else noise_pred
    n, m = ts.shape[0], tq.shape[0]
    if m == 0:
        return 0.0, np.zeros(0), 0                       # (never launched)
    assert n + m <= N_CAP
    blk, N, nb = SPR.joint_blocks(tree, noise, ts, tq, noise_pred)
    npad = nb * BS
    r = np.zeros(npad); r[:n] = xs; r[n:N] = y           # rhs: xs, then the held-out values; padding 0
    z = np.zeros(npad)
    ldg = np.zeros(npad)                                 # 2 log L_kk of every row (padding rows: log 1)
    bad = 0
    for j in range(nb):
        acc = {ib: blk[blk_idx(ib, j)].copy() for ib in range(j, nb)}      # (a) K(ib, j), the diagonal block with both triangles
        for ib in range(j, nb):                          # (b) S(ib, j) = K(ib, j) - sum_{k<j} L(ib, k) L(j, k)', k ascending
            for k in range(j):
                acc[ib] = acc[ib] - blk[blk_idx(ib, k)] @ blk[blk_idx(j, k)].T
        D = acc[j]
        L = np.zeros((BS, BS))
        for c in range(BS):                              # (c) the diagonal block, pivot by pivot
            d = D[c, c] - L[c, :c] @ L[c, :c]
            if not d > 0.0:
                bad = j * BS + c + 1                     # the JOINT index, 1-based
                break
            L[c, c] = math.sqrt(d)
            L[c + 1:, c] = (D[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
        if bad:
            break
        W = np.linalg.inv(L)
        blk[blk_idx(j, j)] = L
        for ib in range(j + 1, nb):                      # (d) the panel: written once, finished, afterwards only read
            blk[blk_idx(ib, j)] = acc[ib] @ W.T
        z[j * BS:(j + 1) * BS] = W @ r[j * BS:(j + 1) * BS]
        ldg[j * BS:(j + 1) * BS] = 2.0 * np.log(np.diag(L))
        for ib in range(j + 1, nb):                      # (e) the right-hand side below the step
            r[ib * BS:(ib + 1) * BS] -= blk[blk_idx(ib, j)] @ z[j * BS:(j + 1) * BS]
    if bad:
        return math.nan, np.full(m, math.nan), bad
    rows = np.arange(npad)
    assert (ldg[N:] == 0.0).all() and (z[N:] == 0.0).all()      # the identity padding contributes an exact 0
    mask = rows >= n                                     # the query rows (and the padding behind them: exact zeros)
    ld = ldg[mask].sum()
    ss = (z[mask] ** 2).sum()
    lj = math.log(abs(slope))
    lp = -0.5 * (m * LOG2PI + ld + ss) + m * lj
    terms = (-0.5 * (z[n:N] ** 2 + LOG2PI) - 0.5 * ldg[n:N]) + lj
    return float(lp), terms, 0


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The shared case: one series per entry of SHAPES (prefixes of shuffled synthetic series; query kind s % 3), on each one prior
    particle of depth <= 3 and two of the ten fixture kernels of _series_proba_ref.fixture_kernels, cycling (so the fifteen series
    with more than 176 joint points see every leaf and both ChangePoints three times), noises in [0.05, 0.3], held-out values 0.5 N(0, 1),
    and a per-particle noise_pred — 0.3 noise (smaller than the noise) for even particles, drawn from [0.02, 0.12] for odd ones.
    Computed once, never modified.  (series, queries, heldout, nodes, noises, sidx, noise_pred)"""
    import __graft_entry__ as g
    pkg = g.load_package()
    rng = np.random.default_rng(20261024)
    fix = SPR.fixture_kernels(pkg)
    series, qs, held, nodes, noises, sidx = [], [], [], [], [], []
    at = 0
    for s, (n, m) in enumerate(SHAPES):
        ts, xs = pkg.prior.synthetic_series(512, seed=600 + s, shuffle=True)
        ts, xs = ts[:n].copy(), xs[:n].copy()
        series.append((ts, xs))
        qs.append(SPR.queries(QUERY_KINDS[s % 3], ts, m, rng))
        held.append(0.5 * rng.standard_normal(m))
        nd, _ = pkg.prior.sample_particles(rng, 1, max_depth=3)
        nd = list(nd) + [fix[at % len(fix)], fix[(at + 1) % len(fix)]]
        at += 2
        nodes += nd; noises += list(0.05 + 0.25 * rng.random(len(nd))); sidx += [s] * len(nd)
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    P = len(nodes)
    noise_pred = np.where(np.arange(P) % 2 == 0, 0.3 * noises, 0.02 + 0.1 * rng.random(P))
    for a in (noises, sidx, noise_pred, *qs, *held):
        a.setflags(write=False)
    return series, qs, held, nodes, noises, sidx, noise_pred


@functools.lru_cache(maxsize=None)
def ragged_references():
    """[(ref, S)] of every particle of ragged_case() under its per-particle noise_pred, by _pred_logpdf_ref.reference — (0.0, 0.0)
    where nothing is held out.  Every particle is factored: reference() raises where it cannot.  Computed once, shared by the CPU
    and the GPU tests, never modified."""
    import _pred_logpdf_ref as PR
    series, qs, held, nodes, noises, sidx, noise_pred = ragged_case()
    out = []
    for p, nd in enumerate(nodes):
        s = int(sidx[p])
        ref, S = PR.reference(nd.to_tuple(), float(noises[p]), *series[s], qs[s], held[s], noise_pred=float(noise_pred[p]))
        assert math.isfinite(ref) and (S > 0.0 or len(qs[s]) == 0), p
        out.append((ref, S))
    return tuple(out)


# 1-based positions on the JOINT index of 512 times split at BAD_SPLIT: K11's first, a block boundary, both sides of the short cap's
# block, the last training row, the first query row (leading minor 1 of the predictive covariance), a block boundary among the query
# rows, the only row of the last block a fourth wave owns first, the last row
BAD_SPLIT = 300
BAD_POSITIONS = (1, 16, 177, 300, 301, 316, 497, 512)


@functools.lru_cache(maxsize=None)
def bad_pivot_case():
    """the construction of tests/test_gpu_long_series_predict.bad_pivot_case on joint times: changepoint_particle(pos - 1) on cp_ts(),
    whose first BAD_SPLIT points train and whose other 212 are held out, both noises CP_NOISE; a good particle sits between the failing
    ones.  Every position is asserted with first_bad_minor on the oracle's joint matrix.  (ts, xs, tq, y, nodes, noises, at)"""
    import __graft_entry__ as g
    import test_gpu_long_series as TL
    from oracle import oracle as O
    pkg = g.load_package()
    t = TL.cp_ts()
    assert t.size == N_CAP
    rng = np.random.default_rng(31)
    v = 0.3 * rng.standard_normal(t.size)
    nodes = [TL.changepoint_particle(pkg, pos - 1) for pos in BAD_POSITIONS]
    for pos, nd in zip(BAD_POSITIONS, nodes):
        K = O.compute_cov_matrix_vectorized(nd.to_tuple(), TL.CP_NOISE, t)
        assert SC.first_bad_minor(K[:pos, :pos]) == pos, pos      # (the leading minors up to pos - 1 factor, minor pos does not)
    at = 3                                                        # the good particle sits between the failing ones
    nodes.insert(at, pkg.SquaredExponential(0.3, 0.8))
    noises = np.full(len(nodes), TL.CP_NOISE); noises[at] = 0.1
    for a in (t, v, noises):
        a.setflags(write=False)
    return t[:BAD_SPLIT], v[:BAD_SPLIT], t[BAD_SPLIT:], v[BAD_SPLIT:], nodes, noises, at
