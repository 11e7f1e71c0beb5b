"""TEST INFRASTRUCTURE: a NumPy restatement of the predictive stages of k_series_predict (csrc/agp_series_kernel.hpp, P1-P2) on the
kernel's own data layout — packed lower 16 x 16 blocks, block (rb, cb) at blk_idx(rb, cb), identity padding past n, beta = L^-1 x
with zero padding — in the kernel's order of operations: the diagonal blocks' inverse transposes in place, then per block of 16 query
times the block row VT(jb) = (K21(jb) - sum_{k<jb} VT(k) L(jb,k)') L(jb,jb)^-T for jb = 0 .. nb - 1 with K21's columns past n masked,
the mean and the sum of squares accumulated block by block, rows past m evaluated at the last query and never written.  Covariance
entries come from the oracle (oracle.eval_cov): this pins the index algebra and the masks on a machine without a GPU, not the device's
arithmetic.  Also the shared ragged case of tests/test_gpu_series_predict.py and the Python twin of the kernel's LDS map."""
import functools

import numpy as np

import _series_grad_ref as R
from oracle import oracle as O

BS = R.BS
blk_idx = R.blk_idx


def series_pred_lds_total(n, n_ops, n_prm, n_cp):
    """series_pred_lds(...).total of csrc/agp_args.hpp: the value kernel's map"""
    return R.series_lds_total(n, n_ops, n_prm, n_cp)


def cp_chain_fits(k, n):
    """tests' cp_chain(G, k) — 2k + 1 nodes, 3k + 1 parameters, k tables — under the predictive kernel's map at n points"""
    return 8 * series_pred_lds_total(n, 2 * k + 1, 3 * k + 1, k) <= R.LDS_BYTES


def series_predict_blocks(tree, noise, ts, xs, tq, noise_pred=None):
    """(mean[m], var[m]) by the kernel's block algorithm"""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); tq = np.asarray(tq, dtype=np.float64)
    noise_pred = noise if noise_pred is None else noise_pred
    n, m = ts.shape[0], tq.shape[0]
    nb = (n + BS - 1) // BS
    npad = nb * BS
    K = O.eval_cov(tree, np.concatenate([ts, tq]))
    Kp = np.eye(npad)
    Kp[:n, :n] = K[:n, :n] + noise * np.eye(n)
    L = np.linalg.cholesky(Kp) if npad else Kp
    xp = np.zeros(npad); xp[:n] = xs
    beta = np.linalg.solve(L, xp) if npad else xp
    blk = R.pack_lower(L, nb)
    for i in range(nb):      # P1: the diagonal slots hold L(i,i)^-T
        blk[blk_idx(i, i)] = np.linalg.inv(blk[blk_idx(i, i)]).T.copy()
    mean = np.full(m, np.nan); var = np.full(m, np.nan)
    for qb in range((m + BS - 1) // BS):
        rows = qb * BS + np.arange(BS)
        at = n + np.minimum(rows, m - 1)                 # rows past m: the last query again
        VT = []
        ms = np.zeros(BS); ss = np.zeros(BS)
        for jb in range(nb):
            cols = jb * BS + np.arange(BS)
            real = cols < n
            K21 = np.full((BS, BS), np.nan)              # (a padding column must never be read with a weight)
            K21[:, real] = K[np.ix_(at, cols[real])]
            acc = np.zeros((BS, BS))
            for k in range(jb):
                acc += VT[k] @ blk[blk_idx(jb, k)].T
            res = (np.where(real[None, :], K21, 0.0) - acc) @ blk[blk_idx(jb, jb)]
            VT.append(res)
            ms += res @ beta[cols]
            ss += (res * res).sum(axis=1)
        kd = K[at, at]
        ok = rows < m
        mean[rows[ok]] = ms[ok]
        var[rows[ok]] = (kd[ok] - ss[ok]) + noise_pred
    return mean, var


def queries_for(ts_full, ts, m):
    """m query times past the end of the full 256-point series; from three queries on (and a point to train on) the first is a
    training time and the second the midpoint of the first two training times"""
    lo, hi = ts_full.min(), ts_full.max()
    tq = hi + (hi - lo) * np.arange(1, m + 1) / 40.0
    if m >= 3 and len(ts) >= 1:
        tq[0] = ts[0]
        if len(ts) >= 2:
            tq[1] = 0.5 * (ts[0] + ts[1])
    return tq


RAGGED_N = (0, 1, 2, 15, 16, 17, 33, 126, 144, 176)
RAGGED_M = (5, 0, 1, 15, 16, 17, 33, 12, 36, 65)      # 65: a wave takes a second query block


def close(a, ref, tol=1e-8):
    """|d| <= tol max(1, max|ref|), the whole vector (a particle's mean or variance block)"""
    a = np.asarray(a, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return a.size == 0
    return bool(np.isfinite(a).all() and np.abs(a - ref).max() <= tol * max(1.0, np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The shared case: ten ragged series with ragged query sets, six prior particles each, and the oracle's predictive means and
    variances (computed once, never modified).  (series, queries, nodes, noises, sidx, ref_mean, ref_var)"""
    import __graft_entry__ as g
    pkg = g.load_package()
    rng = np.random.default_rng(20261019)
    series, queries, nodes, noises, sidx = [], [], [], [], []
    for s, (n, m) in enumerate(zip(RAGGED_N, RAGGED_M)):
        ts, xs = pkg.prior.synthetic_series(256, seed=300 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        queries.append(queries_for(ts, ts[:n], m))
        nd, nz = pkg.prior.sample_particles(rng, 6, max_depth=3)
        nodes += nd; noises += list(nz); sidx += [s] * 6
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    ref_mean, ref_var = [], []
    for nd, nz, s in zip(nodes, noises, sidx):
        mu, cov = O.predict_mvn(nd.to_tuple(), float(nz), *series[s], queries[s])
        ref_mean.append(mu); ref_var.append(np.diag(cov).copy())
    for a in (noises, sidx, *ref_mean, *ref_var, *queries):
        a.setflags(write=False)
    return series, queries, nodes, noises, sidx, ref_mean, ref_var
