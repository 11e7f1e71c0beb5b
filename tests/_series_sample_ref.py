"""NumPy restatement of the index algebra of the sampling twin's read-out (series_sample_readout, csrc/agp_series_kernel.hpp): the
packed lower 16 x 16 blocks of the JOINT factor as the short-series kernels hold them in LDS, the one masked accessor of the query
rows, the lane -> (row, k, sample) map of v_mfma_f64_16x16x4 including the permuted order of k inside a block of 16 (lane (j, q)
feeds query points 16 kb + 4 q + s4 at step s4: the four words of one Philox block), the split between training and query points
anywhere inside a block, the passes over the row blocks, the per-particle CSR lists of samples and the offsets of the flat outputs
(layout, assemble).  Sums run in the kernel's order over k but in NumPy's arithmetic: results agree with the dense formula to
rounding, not to the bit.

Also the per-series draws of agp_predict_sample_series_batch on tests/_pred_sample_ref.py (series s draws as the resident entry does
under seeds[s]) and the dense reference of the entry's outputs."""
import numpy as np

import _pred_sample_ref as PS

RBP = 6                      # row blocks per pass of the sample loop
LANE = np.arange(64)
L15, LQ = LANE & 15, LANE >> 4


def blk_idx(rb, cb):
    return rb * (rb + 1) // 2 + cb


def pack_blocks(L, junk=np.nan):
    """The N x N lower factor L -> packed blocks: block (rb, cb) column-major at blk_idx(rb, cb) * 256; rows / columns past N are
    identity; above the diagonal inside a diagonal block sits `junk` (the kernel must never let it reach an operand)."""
    N = L.shape[0]
    nb = (N + 15) // 16
    sm = np.zeros(nb * (nb + 1) // 2 * 256)
    for rb in range(nb):
        for cb in range(rb + 1):
            for c in range(16):
                for r in range(16):
                    gi, gj = rb * 16 + r, cb * 16 + c
                    if gj > gi:
                        v = junk
                    elif gi < N:
                        v = L[gi, gj]
                    else:
                        v = 1.0 if gi == gj else 0.0
                    sm[blk_idx(rb, cb) * 256 + c * 16 + r] = v
    return sm


def lq(sm, ntr, m, ir, ic):
    """L22(ir, ic) for arrays of query indices: 0 above the diagonal and for rows past m (a select, after a read at a safe address)"""
    on = (ic <= ir) & (ir < m)
    jr = ntr + np.where(on, ir, 0)
    jc = ntr + np.where(on, ic, 0)
    v = sm[blk_idx(jr >> 4, jc >> 4) * 256 + (jc & 15) * 16 + (jr & 15)]
    return np.where(on, v, 0.0)


def mfma(a, b, c):
    """D = C + A B on 64 lanes: A[i][k] in lane 16 k + i, B[k][j] in lane 16 k + j, D[4 r + q][j] in register r of lane 16 q + j"""
    A = a.reshape(4, 16).T            # [i][k]
    B = b.reshape(4, 16)              # [k][j]
    D = A @ B                         # [i][j]
    out = c.copy()
    for r in range(4):
        out[r] += D[4 * r + LQ, L15]
    return out


def readout(sm, avec, ntr, m, samples, z, slope, icpt):
    """One particle: (x {sample index: column of m}, mean (m,), cov (m, m)) in raw space.  samples: the particle's CSR list
    (ascending sample indices); z[i, j]: the normal of query point i of sample j."""
    mu = np.zeros(m)
    for i in range(m):
        row = ntr + i
        s = 0.0
        for k in range(ntr):
            s += sm[blk_idx(row >> 4, k >> 4) * 256 + (k & 15) * 16 + (row & 15)] * avec[k]
        mu[i] = s
    mean = (mu - icpt) / slope
    sgn = 1.0 if slope > 0 else -1.0
    nqb = (m + 15) >> 4
    x = {}
    cnt = len(samples)
    for g in range((cnt + 15) // 16):            # (group g runs on wave g % 4: no arithmetic depends on it)
        js = g * 16 + L15
        live = js < cnt
        j = np.where(live, np.asarray(samples)[np.minimum(js, cnt - 1)], 0)
        for rb0 in range(0, nqb, RBP):
            acc = []
            for u in range(RBP):
                a4 = np.zeros((4, 64))
                for r in range(4):
                    i = (rb0 + u) * 16 + 4 * r + LQ
                    a4[r] = np.where(i < m, mu[np.minimum(i, m - 1)], 0.0)
                acc.append(a4)
            for kb in range(min(rb0 + RBP, nqb)):
                zz = []
                for s4 in range(4):
                    i = kb * 16 + 4 * LQ + s4
                    zz.append(np.where(live & (i < m), sgn * z[np.minimum(i, m - 1), j], 0.0))
                for u in range(RBP):
                    rb = rb0 + u
                    if rb >= kb and rb < nqb:
                        for s4 in range(4):
                            acc[u] = mfma(lq(sm, ntr, m, rb * 16 + L15, kb * 16 + 4 * LQ + s4), zz[s4], acc[u])
            for u in range(RBP):
                if rb0 + u < nqb:
                    for r in range(4):
                        i = (rb0 + u) * 16 + 4 * r + LQ
                        for lane in np.flatnonzero(live & (i < m)):
                            x.setdefault(int(j[lane]), np.full(m, np.nan))[i[lane]] = (acc[u][r][lane] - icpt) / slope
    cov = np.full((m, m), np.nan)
    for rb in range(nqb):
        for cb in range(rb + 1):
            acc = np.zeros((4, 64))
            for kb in range(cb + 1):
                for s4 in range(4):
                    k = kb * 16 + 4 * s4 + LQ
                    acc = mfma(lq(sm, ntr, m, cb * 16 + L15, k), lq(sm, ntr, m, rb * 16 + L15, k), acc)
            for r in range(4):
                row, col = rb * 16 + L15, cb * 16 + 4 * r + LQ
                for lane in np.flatnonzero((row < m) & (col <= row)):
                    v = acc[r][lane] / (slope * slope)
                    cov[row[lane], col[lane]] = v
                    cov[col[lane], row[lane]] = v
    return x, mean, cov


def layout(m_s, sidx, R):
    """The entry's flat outputs for series of m_s[s] query points and particles of series sidx[p]: (x_off (S + 1), out_off (P + 1),
    cov_off (P + 1)) — series s owns out_x[R q_off[s], R q_off[s + 1]), sample j its m_s values at + j m_s; particle p owns
    out_mean[out_off[p], out_off[p + 1]) (m values) and out_cov[cov_off[p], cov_off[p + 1]) (m x m, column-major)"""
    m_s = np.asarray(m_s, dtype=np.int64)
    q_off = np.concatenate([[0], np.cumsum(m_s)])
    mp = m_s[np.asarray(sidx, dtype=np.int64)] if len(sidx) else np.zeros(0, dtype=np.int64)
    return R * q_off, np.concatenate([[0], np.cumsum(mp)]), np.concatenate([[0], np.cumsum(mp * mp)])


def assemble(m_s, sidx, R, results):
    """results[p] = readout()'s (x, mean, cov) of particle p -> the flat (out_x, out_mean, out_cov) of the entry, through layout()"""
    x_off, out_off, cov_off = layout(m_s, sidx, R)
    ox, om, oc = np.full(x_off[-1], np.nan), np.full(out_off[-1], np.nan), np.full(cov_off[-1], np.nan)
    for p, (x, mean, cov) in enumerate(results):
        s, m = int(sidx[p]), int(m_s[sidx[p]])
        for j, col in x.items():
            ox[x_off[s] + j * m:x_off[s] + (j + 1) * m] = col
        om[out_off[p]:out_off[p + 1]] = mean
        oc[cov_off[p]:cov_off[p + 1]] = cov.ravel(order="F")
    return ox, om, oc


def csr(component, P):
    """component (R,) of one series, in LOCAL particle indices -> the per-particle ascending sample lists"""
    return [np.flatnonzero(np.asarray(component) == p) for p in range(P)]


def dense(mu, Sigma, z, slope, icpt):
    """(mu* + sign(a) chol(Sigma*) z - b) / a for the columns of z"""
    L22 = np.linalg.cholesky(Sigma)
    sgn = 1.0 if slope > 0 else -1.0
    return (mu[:, None] + sgn * (L22 @ z) - icpt) / slope


def draws(seed, weights, m, R):
    """Series-local components and normals of a series' R samples under `seed` (tests/_pred_sample_ref.py): (component (R,), z (m, R))"""
    return PS.components(seed, weights, R), PS.normals(seed, m, range(R))
