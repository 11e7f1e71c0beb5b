"""TEST INFRASTRUCTURE: a NumPy restatement of the coded-row stages of k_series_predict_sum (csrc/agp_series_kernel.hpp) on the
kernel's own data layout and in its order of operations.  A particle's model is X = F_1 + .. + F_M + noise, evaluated as ONE
composite program K_1 SEL_1 * K_2 SEL_2 * + .. on coded points: SEL_i's per-point table holds 1 at every training point (code 0)
and (code == 0 or code == i) at a query slot.  Series s with m query times has (M + 1) m joint rows g in the reference's order
F_1(T*) .. F_M(T*), X(T*): component i = g // m at time tq[g % m], code i + 1 (the observable, last, 0), diagonal addend
1e-8 + (noise_pred on the observable rows).  Rows are taken 16 at a time whatever their codes — a block may mix them — through
series_predict_blocks' block rows on the packed factor (tests/_series_predict_ref.py); rows past (M + 1) m evaluate the last row
again and are never written.  Then the read-out of k_sum_readout in the same lanes and the info rule.  Covariance entries come from
the oracle (oracle.eval_cov per component): this pins the row map, the masks and the read-out on a machine without a GPU, not the
device's arithmetic.  Also the shared ragged case of tests/test_gpu_series_sum.py and the Python twin of the LDS need."""
import functools
import math
from statistics import NormalDist

import numpy as np

import _series_grad_ref as R
import _series_predict_ref as RP
from oracle import oracle as O

BS = R.BS
blk_idx = R.blk_idx
JITTER = 1e-8
close = RP.close


def composite_sizes(trees):
    """(n_ops, n_prm, n_cp) of the composite K_1 SEL_1 * K_2 SEL_2 * + .. of the component trees (oracle tuples): every component's
    own nodes and parameters, a selector leaf (one parameter, one per-point table) and a Times per component, M - 1 Plus nodes"""
    M = len(trees)
    n_ops = n_prm = n_cp = 0
    for t in trees:
        ops, prm = O.tree_to_program(t)
        n_ops += len(ops); n_prm += len(prm)
        n_cp += sum(1 for o in ops if o == 8)             # OP_CP: a ChangePoint node's sigma table
    return n_ops + 2 * M + (M - 1), n_prm + M, n_cp + M


def series_sum_lds_bytes(n, trees):
    """the LDS need of one particle: series_pred_lds (the value kernel's map) with the M selector tables counted"""
    return 8 * RP.series_pred_lds_total(n, *composite_sizes(trees))


def sel_table(codes, i):
    """SEL_i's per-point table at points of the given component codes"""
    codes = np.asarray(codes)
    return np.where((codes == 0) | (codes == i), 1.0, 0.0)


def series_sum_rows(trees, noise, ts, xs, tq, noise_pred=None, y_transform=(1.0, 0.0), q=()):
    """(mean[(M+1)m], var[(M+1)m], x[(M+1)m, nq], info) by the kernel's coded-row algorithm: raw-space marginals and quantiles"""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64); tq = np.asarray(tq, dtype=np.float64)
    noise_pred = noise if noise_pred is None else noise_pred
    a, b = (np.float64(v) for v in y_transform)      # (NumPy scalars: an overflow gives inf, as on the device, not an exception)
    M, n, m = len(trees), ts.shape[0], tq.shape[0]
    rows = (M + 1) * m
    z = np.array([NormalDist().inv_cdf(float(v)) for v in q])
    nb = (n + BS - 1) // BS
    npad = nb * BS
    Ki = [O.eval_cov(t, np.concatenate([ts, tq])) for t in trees]
    # stages 2-5: every selector's table is 1.0 at the training points, so K11 is the sum of the components
    train = [sel_table(np.zeros(n, dtype=int), i + 1) for i in range(M)]
    Kp = np.eye(npad)
    Kp[:n, :n] = sum(K[:n, :n] * np.outer(s, s) for K, s in zip(Ki, train)) + noise * np.eye(n)
    L = np.linalg.cholesky(Kp) if npad else Kp
    xp = np.zeros(npad); xp[:n] = xs
    beta = np.linalg.solve(L, xp) if npad else xp
    blk = R.pack_lower(L, nb)
    for i in range(nb):      # P1
        blk[blk_idx(i, i)] = np.linalg.inv(blk[blk_idx(i, i)]).T.copy()
    mean = np.full(rows, np.nan); var = np.full(rows, np.nan)
    for qb in range((rows + BS - 1) // BS):
        lane = qb * BS + np.arange(BS)
        g = np.minimum(lane, rows - 1)                   # rows past the end: the last row again
        comp = g // m
        at = n + g % m
        code = np.where(comp < M, comp + 1, 0)
        slot = [sel_table(code, i + 1) for i in range(M)]            # the selectors' entries at the 16 query slots
        VT = []
        ms = np.zeros(BS); ss = np.zeros(BS)
        for jb in range(nb):
            cols = jb * BS + np.arange(BS)
            real = cols < n
            K21 = np.full((BS, BS), np.nan)              # (a padding column must never be read with a weight)
            K21[:, real] = sum(K[np.ix_(at, cols[real])] * np.outer(sq, st[cols[real]]) for K, sq, st in zip(Ki, slot, train))
            acc = np.zeros((BS, BS))
            for k in range(jb):
                acc += VT[k] @ blk[blk_idx(jb, k)].T
            res = (np.where(real[None, :], K21, 0.0) - acc) @ blk[blk_idx(jb, jb)]
            VT.append(res)
            ms += res @ beta[cols]
            ss += (res * res).sum(axis=1)
        kd = sum(K[at, at] * sq * sq for K, sq in zip(Ki, slot))
        addend = JITTER + np.where(comp == M, noise_pred, 0.0)
        ok = lane < rows
        mean[lane[ok]] = ms[ok]
        var[lane[ok]] = (kd[ok] - ss[ok]) + addend[ok]
    # the read-out (k_sum_readout's statements) and the info rule
    with np.errstate(all="ignore"):
        mr = (mean - b) / a
        mr[:m] = mr[:m] + b / a
        vr = (1.0 / (a * a)) * var
        good = np.isfinite(mr) & (vr >= 0.0)
        sd = np.where(good, np.sqrt(np.where(good, vr, 0.0)), np.nan)
        x = sd[:, None] * z[None, :] + mr[:, None]
    if not good.all():
        first = int(np.flatnonzero(~good)[0])
        return np.full(rows, np.nan), np.full(rows, np.nan), np.full((rows, len(z)), np.nan), n + first + 1
    return mr, vr, x, 0


def oracle_rows(trees, noise, ts, xs, tq, noise_pred=None, y_transform=(1.0, 0.0), q=()):
    """(mean, var, x) of the same rows from oracle.infer_gp_sum (an empty series: the prior of every part), mapped to raw space as
    predict_mvn_sum maps them (tests/_sum_decomposition_ref.py), quantiles by oracle.quantile"""
    a, b = (float(v) for v in y_transform)
    tq = np.asarray(tq, dtype=np.float64)
    M, m = len(trees), tq.shape[0]
    npred = noise if noise_pred is None else noise_pred
    if len(ts) == 0:
        Kd = [np.diag(O.eval_cov(t, tq)) for t in trees]
        mu = np.zeros((M + 1) * m)
        v = np.concatenate([k + JITTER for k in Kd] + [sum(Kd) + npred + JITTER])
    else:
        mu, S, _, _ = O.infer_gp_sum(list(trees), float(noise), ts, xs, tq, noise_pred=noise_pred)
        v = np.diag(S).copy()
    mr = (mu - b) / a
    mr[:m] += b / a
    vr = (1.0 / (a * a)) * v
    x = O.quantile(mr, np.diag(vr), list(q)) if len(q) else np.zeros((len(mr), 0))
    return mr, vr, x


RAGGED_N = (0, 1, 15, 16, 17, 33, 126, 144, 176)
RAGGED_M = (5, 0, 1, 6, 16, 22, 11, 12, 36)      # 5: three codes in one block; 6: X straddles two; 22: 66 rows, a second block per wave
Q = (0.025, 0.5, 0.975)
SEED = 20261020


def hand_built(G, ts):
    """two particles for a long series: one whose two parts are both non-trivial and which carries a ChangePoint (split by
    Periodic), one with WhiteNoise — its queries include a training time (queries_for) — split by WhiteNoise"""
    mid = float(np.median(ts))
    cp = G.ChangePoint(G.Periodic(0.4, 0.3, 0.6) + G.SquaredExponential(0.3, 0.5), G.Linear(0.2, 0.1, 0.4) * G.Periodic(0.7, 0.25, 0.5), mid, 0.08)
    wn = G.SquaredExponential(0.25, 0.7) + G.WhiteNoise(0.15)
    return [(cp, G.Periodic, 0.07), (wn, G.WhiteNoise, 0.05)]


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The shared case: nine ragged series with ragged query sets, four prior particles each split by Periodic / Linear /
    SquaredExponential in rotation, two hand-built particles on each series of more than 100 points, per-series transforms, and
    the oracle's rows (computed once, never modified).
    (series, queries, splits, noises, sidx, y_transforms, ref_mean, ref_var, ref_x)"""
    import __graft_entry__ as g
    pkg = g.load_package()
    rng = np.random.default_rng(SEED)
    leaf = (pkg.Periodic, pkg.Linear, pkg.SquaredExponential)
    series, queries, splits, noises, sidx = [], [], [], [], []
    k = 0
    for s, (n, m) in enumerate(zip(RAGGED_N, RAGGED_M)):
        ts, xs = pkg.prior.synthetic_series(256, seed=300 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        queries.append(RP.queries_for(ts, ts[:n], m))
        nd, nz = pkg.prior.sample_particles(rng, 4, max_depth=3)
        for node, noise in zip(nd, nz):
            splits.append(pkg.split_kernel_sop(node, leaf[k % 3])); noises.append(float(noise)); sidx.append(s)
            k += 1
        if n > 100:
            for node, lt, noise in hand_built(pkg, ts[:n]):
                splits.append(pkg.split_kernel_sop(node, lt)); noises.append(noise); sidx.append(s)
    noises = np.array(noises); sidx = np.array(sidx, dtype=np.int32)
    yts = np.array([(1.0 + 0.25 * s, 0.1 * s - 0.3) for s in range(len(series))])
    yts[3] = (-0.8, 0.4)      # a negative slope
    ref_mean, ref_var, ref_x = [], [], []
    for sp, nz, s in zip(splits, noises, sidx):
        mr, vr, x = oracle_rows([c.to_tuple() for c in sp], float(nz), *series[s], queries[s], y_transform=yts[s], q=Q)
        ref_mean.append(mr); ref_var.append(vr); ref_x.append(x)
    for arr in (noises, sidx, yts, *ref_mean, *ref_var, *ref_x, *queries):
        arr.setflags(write=False)
    return series, queries, splits, noises, sidx, yts, ref_mean, ref_var, ref_x


def ndtri(q):
    return np.array([NormalDist().inv_cdf(float(v)) for v in np.atleast_1d(q)])


def mixture_quantile(means, sds, w, q, lo=-1e6, hi=1e6, iters=200):
    """the q-quantile of sum_j w_j N(means_j, sds_j^2) by bisection on the mixture CDF"""
    cdf = lambda x: sum(wj * 0.5 * (1.0 + math.erf((x - mj) / (sj * math.sqrt(2.0)))) for mj, sj, wj in zip(means, sds, w))
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if cdf(mid) < q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)
