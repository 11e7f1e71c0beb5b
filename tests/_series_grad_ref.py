"""TEST INFRASTRUCTURE: a NumPy restatement of the gradient stages of k_series_logpdf_grad (csrc/agp_series_kernel.hpp, G1-G5) on the
kernel's own data layout — packed lower 16 x 16 blocks, block (rb, cb) at blk_idx(rb, cb), identity padding past n — in the kernel's
order of operations: the diagonal blocks' inverses by forward substitution, Z = L^-T in place block column by block column (a column's
results are formed from the old content of its slot row and written afterwards), alpha = Z beta, and per lower block
K^-1(rb, cb) = sum_{k >= rb} Z(rb, k) Z(cb, k)', G = 1/2 (alpha alpha' - K^-1) with weight 2 off the diagonal, 1 on diagonal blocks (evaluated in
full), 0 past n, and tr G from the diagonal elements.  dK / d theta comes from the oracle (oracle.eval_cov_grad): this pins the index
algebra and the weights on a machine without a GPU, not the device's arithmetic.  Also the Python twin of the kernel's LDS map."""
import numpy as np

from oracle import oracle as O

BS = 16
LDS_BYTES = 160 * 1024


def blk_idx(rb, cb):
    return rb * (rb + 1) // 2 + cb


def series_lds_total(n, n_ops, n_prm, n_cp):
    """series_lds(...).total of csrc/agp_args.hpp, in doubles"""
    nb = (n + BS - 1) // BS
    npad = nb * BS
    o_prm = 256 + 3 * npad + 128
    o_ops = o_prm + ((n_prm + 3) & ~1)
    o_sig = o_ops + (((n_ops + 1) // 2 + 1) & ~1)
    o_blk = o_sig + n_cp * 256
    return o_blk + (nb * (nb + 1) // 2) * 256


def series_grad_lds_total(n, n_ops, n_prm, n_cp, g_n_ops, g_n_prm):
    """series_grad_lds(...).total: the complement tables, alpha, the gradient program and the reduction scratch in front of the blocks"""
    nb = (n + BS - 1) // BS
    extra = n_cp * 256 + nb * BS + ((g_n_prm + 4) & ~1) + ((g_n_ops + 1) & ~1) + ((4 * (g_n_prm + 1) + 1) & ~1)
    return series_lds_total(n, n_ops, n_prm, n_cp) + extra


def cp_chain_fits(k, n, grad=True):
    """Does tests' cp_chain(G, k) — k ChangePoint nodes over k + 1 Constant leaves: 2k + 1 nodes, 3k + 1 parameters, k tables — fit
    the 160 KiB at n points?"""
    n_ops, n_prm = 2 * k + 1, 3 * k + 1
    tot = series_grad_lds_total(n, n_ops, n_prm, k, n_ops, n_prm) if grad else series_lds_total(n, n_ops, n_prm, k)
    return 8 * tot <= LDS_BYTES


def pack_lower(A, nb):
    return [A[rb * BS:(rb + 1) * BS, cb * BS:(cb + 1) * BS].copy() for rb in range(nb) for cb in range(rb + 1)]


def series_grad_blocks(tree, noise, ts, xs):
    """(logpdf, grad [program-parameter order], d/dnoise) by the kernel's block algorithm."""
    ts = np.asarray(ts, dtype=np.float64); xs = np.asarray(xs, dtype=np.float64)
    n = ts.shape[0]
    nb = (n + BS - 1) // BS
    npad = nb * BS
    K, dKs = O.eval_cov_grad(tree, ts)
    Kp = np.eye(npad)
    Kp[:n, :n] = K + noise * np.eye(n)
    L = np.linalg.cholesky(Kp)
    xp = np.zeros(npad); xp[:n] = xs
    beta = np.linalg.solve(L, xp)                       # (exactly 0 on the padding: identity rows)
    lp = -0.5 * (n * np.log(2 * np.pi) + 2 * np.log(np.diag(L)).sum() + beta @ beta)
    blk = pack_lower(L, nb)
    # G1: Z(i,i) = L(i,i)^-T, column c of the inverse by forward substitution
    for i in range(nb):
        Lb = blk[blk_idx(i, i)]
        W = np.zeros((BS, BS))
        for c in range(BS):
            for r in range(BS):
                s = 1.0 if r == c else 0.0
                for k in range(r):
                    s -= Lb[r, k] * W[k, c]
                W[r, c] = s / Lb[r, r]
        blk[blk_idx(i, i)] = W.T.copy()
    # G2: column i of Z in slot row i; results are held back until the whole row of L has been read
    for i in range(1, nb):
        Wi = blk[blk_idx(i, i)].T
        res = {}
        for j in range(i):
            acc = np.zeros((BS, BS))
            for k in range(j, i):
                acc += blk[blk_idx(k, j)] @ blk[blk_idx(i, k)].T          # Z(j,k) L(i,k)'
            res[j] = (-acc) @ Wi.T
        for j in range(i):
            blk[blk_idx(i, j)] = res[j]
    # G3: alpha = Z beta
    alpha = np.zeros(npad)
    for j in range(nb):
        for k in range(j, nb):
            alpha[j * BS:(j + 1) * BS] += blk[blk_idx(k, j)] @ beta[k * BS:(k + 1) * BS]
    # G4 / G5: contraction block by block
    g = np.zeros(len(dKs)); gn = 0.0
    idx = np.arange(npad)
    dKp = []
    for dK in dKs:
        D = np.full((npad, npad), np.nan)               # (padding must never be read with a non-zero weight)
        D[:n, :n] = dK
        dKp.append(D)
    for rb in range(nb):
        for cb in range(rb + 1):
            kin = np.zeros((BS, BS))
            for k in range(rb, nb):
                kin += blk[blk_idx(k, rb)] @ blk[blk_idx(k, cb)].T
            ri, ci = idx[rb * BS:(rb + 1) * BS], idx[cb * BS:(cb + 1) * BS]
            valid = (ri[:, None] < n) & (ci[None, :] < n)
            G = np.where(valid, 0.5 * (np.outer(alpha[ri], alpha[ci]) - kin), 0.0)
            gn += G[ri[:, None] == ci[None, :]].sum()
            wgt = (1.0 if rb == cb else 2.0) * G
            for q, D in enumerate(dKp):
                sub = D[rb * BS:(rb + 1) * BS, cb * BS:(cb + 1) * BS]
                g[q] += np.where(valid, wgt * np.where(valid, sub, 0.0), 0.0).sum()
    return float(lp), g, float(gn)
