"""TEST INFRASTRUCTURE of the long-series forecast (agp_predict_long_series_batch; stage P of csrc/agp_long_series_kernel.hpp):

  * long_series_predict_blocks: a NumPy restatement of stage P on the kernel's own data layout and in its order — the packed factor,
    one inverse W(j) = L(j, j)^-1 per block column, alpha = L^-1 x with zero padding; query blocks of 16 times dealt to four waves
    (qb % 4), each wave in rounds of C chains, chain u of wave w in scratch row w + 4 u; per block column j
        S(q, j) = K21(q, j) - sum_{k<j} VT(q, k) L(j, k)',  VT(q, j) = S(q, j) W(j)',  mean += VT alpha_j,  ss += rowsums(VT^2)
    with K21's columns past n masked, VT(q, k) read back from the scratch row, rows past m evaluated at the last query and never
    written.  Scratch rows and padding are NaN-poisoned.  Covariance entries come from the oracle (oracle.eval_cov): this pins the
    index algebra, the masks and the scratch rows' life on a machine without a GPU, not the device's arithmetic.  `fault` plants
    one of three mistakes (tests/test_long_series_predict_cpu.py shows each is caught).
  * the Python twin of the kernel's LDS map and workspace size (agp_args.hpp: long_series_pred_lds, long_series_pred_ws_blocks);
  * the shared ragged case of tests/test_gpu_long_series_predict.py: test_gpu_long_series.ragged_case()'s series and particles with
    ragged query sets, and the oracle's predictive means and variances (computed once, never modified)."""
import functools

import numpy as np

import _series_grad_ref as R
import _series_predict_ref as SP
from oracle import oracle as O

BS = R.BS
blk_idx = R.blk_idx
LONG_SERIES_MAX_N = 512
LONG_PRED_C = 2                                  # chains (query blocks) per wave and round
LONG_PRED_QSLOT = LONG_SERIES_MAX_N
LONG_PRED_SIG_STRIDE = LONG_PRED_QSLOT + 4 * LONG_PRED_C * BS
ROUND = 4 * LONG_PRED_C * BS                     # query times of one round of the four waves
FAULTS = ("neighbour_W", "padding_weight", "stale_scratch")


def long_series_lds_total(n, n_ops, n_prm, n_cp, stride=LONG_SERIES_MAX_N):
    """long_series_lds(...).total of csrc/agp_args.hpp, in doubles (stride: entries of one per-point table)"""
    nb = (n + BS - 1) // BS
    o_etab = 512 + 4 * nb * BS
    o_prm = o_etab + 128
    o_ops = o_prm + ((n_prm + 3) & ~1)
    o_sig = o_ops + (((n_ops + 1) // 2 + 1) & ~1)
    return o_sig + n_cp * stride


def long_series_pred_lds_total(n, n_ops, n_prm, n_cp):
    """long_series_pred_lds(...).total: the value kernel's map with tables of LONG_PRED_SIG_STRIDE entries"""
    return long_series_lds_total(n, n_ops, n_prm, n_cp, LONG_PRED_SIG_STRIDE)


def long_series_pred_ws_blocks(nb):
    """blocks of 256 doubles per workgroup: the triangle, 4 C scratch rows in its packing, nb inverses"""
    r = nb + 4 * LONG_PRED_C
    return r * (r + 1) // 2 + nb


def cp_chain_fits(k, n):
    """tests' cp_chain(G, k) — 2k + 1 nodes, 3k + 1 parameters, k tables — under the long predictive kernel's map at n points"""
    return 8 * long_series_pred_lds_total(n, 2 * k + 1, 3 * k + 1, k) <= R.LDS_BYTES


def long_series_predict_blocks(tree, noise, ts, xs, tq, noise_pred=None, fault=None):
    """(mean[m], var[m]) by stage P's block algorithm"""
    assert fault is None or fault in FAULTS
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); tq = np.asarray(tq, dtype=np.float64)
    noise_pred = noise if noise_pred is None else noise_pred
    n, m = ts.shape[0], tq.shape[0]
    C = LONG_PRED_C
    nb = (n + BS - 1) // BS
    npad = nb * BS
    K = O.eval_cov(tree, np.concatenate([ts, tq]))
    Kp = np.eye(npad)
    Kp[:n, :n] = K[:n, :n] + noise * np.eye(n)
    L = np.linalg.cholesky(Kp)
    xp = np.zeros(npad); xp[:n] = xs
    alpha = np.linalg.solve(L, xp)
    blk = R.pack_lower(L, nb)
    W = [np.linalg.inv(blk[blk_idx(j, j)]) for j in range(nb)]                     # per block column, behind the triangle
    scratch = [[np.full((BS, BS), np.nan) for _ in range(nb + 1)] for _ in range(4 * C)]      # rows nb + w + 4 u, blocks 0 .. nb
    mean = np.full(m, np.nan); var = np.full(m, np.nan)
    n_qb = (m + BS - 1) // BS
    for rnd in range((n_qb + 4 * C - 1) // (4 * C)):
        for w in range(4):
            for u in range(C):
                qb = w + 4 * (u + C * rnd)
                if qb >= n_qb:
                    continue
                row = scratch[w + 4 * u]
                rows = qb * BS + np.arange(BS)
                at = n + np.minimum(rows, m - 1)                 # rows past m: the last query again
                ms = np.zeros(BS); ss = np.zeros(BS)
                for j in range(nb):
                    cols = j * BS + np.arange(BS)
                    real = cols < n
                    K21 = np.full((BS, BS), np.nan)              # (a padding column must never be read with a weight ...
                    K21[:, real] = K[np.ix_(at, cols[real])]
                    if fault == "padding_weight":                # ... as here: the kernel's own padding time, the last training point)
                        K21[:, ~real] = K[np.ix_(at, np.full((~real).sum(), n - 1))]
                        S_ = K21.copy()
                    else:
                        S_ = np.where(real[None, :], K21, 0.0)
                    for k in range(j):
                        S_ = S_ - row[k] @ blk[blk_idx(j, k)].T
                    Wj = W[j]
                    if fault == "neighbour_W" and nb > 1:
                        Wj = W[j + 1 if j + 1 < nb else j - 1]
                    VT = S_ @ Wj.T
                    if not (fault == "stale_scratch" and rnd > 0):      # (the fault: a later round reads the first round's blocks)
                        row[j] = VT
                    ms += VT @ alpha[cols]
                    ss += (VT * VT).sum(axis=1)
                row[nb] = np.repeat(K[at, at][:, None], BS, axis=1)      # "block" nb: k(t*, t*), every column alike
                kd = row[nb][:, 0]
                ok = rows < m
                mean[rows[ok]] = ms[ok]
                var[rows[ok]] = (kd[ok] - ss[ok]) + noise_pred
    return mean, var


RAGGED_M = (5, 0, 1, 15, 16, 17, 33, 12, 65, 16, 529, 36, 1, 129, 36, 257)      # 529: 34 query blocks, more than any round holds


@functools.lru_cache(maxsize=None)
def ragged_case():
    """(series, queries, nodes, noises, sidx, ref_mean, ref_var, ref_logpdf): test_gpu_long_series.ragged_case() with query sets"""
    import test_gpu_long_series as TL
    import __graft_entry__ as g
    pkg = g.load_package()
    series, nodes, noises, sidx, ref_lp = TL.ragged_case()
    assert len(RAGGED_M) == len(TL.LENS)
    queries = []
    for s, (n, m) in enumerate(zip(TL.LENS, RAGGED_M)):
        ts_full, _ = pkg.prior.synthetic_series(512, seed=300 + s, shuffle=True)
        assert np.array_equal(ts_full[:n], series[s][0])
        queries.append(SP.queries_for(ts_full, ts_full[:n], m))
    ref_mean, ref_var = [], []
    for nd, nz, s in zip(nodes, noises, sidx):
        mu, cov = O.predict_mvn(nd.to_tuple(), float(nz), *series[s], queries[s])
        ref_mean.append(np.asarray(mu, dtype=np.float64).reshape(-1)); ref_var.append(np.diag(cov).copy() if len(queries[s]) else np.zeros(0))
    for a in (*ref_mean, *ref_var, *queries):
        a.setflags(write=False)
    return series, queries, nodes, noises, sidx, ref_mean, ref_var, ref_lp
