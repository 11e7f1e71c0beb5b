"""A float64 NumPy twin of the long-series kernel's block algorithm, written from the header comment of
csrc/agp_long_series_kernel.hpp (it calls no engine code), with planted faults: what tests/test_long_series_probe_cpu.py uses to show
that the bounds of tests/test_gpu_long_series_probe.py reject faults the value's 1e-8 comparison cannot see.

Per 16-wide block column j, left-looking on packed blocks:
  (a)/(b) S(ib, j) = K(ib, j) - sum_{k < j} L(ib, k) L(j, k)' for ib >= j, k ascending, each k-step as four 4-deep slices
          (v_mfma_f64_16x16x4);
  (c)     L(j, j) = chol S(j, j) with reciprocal roots, W = L(j, j)^-1 formed explicitly; a non-positive pivot stops (LAPACK info);
  (d)     panel L(ib, j) = S(ib, j) W';  alpha_j = W r_j, then one refinement step alpha_j += W (r_j - L(j, j) alpha_j);
  (e)     r_ib -= L(ib, j) alpha_j.
Rows and columns past n are identity.  The value is -(n log 2 pi + 2 sum log L_ii + alpha'alpha) / 2.

fault =
  ("scale", ib, j, i, c, eps)   entry (i, c) of panel block (ib, j), ib > j, is multiplied by 1 + eps as it leaves (d) — the stored
                                block and the registers of (e) alike;
  ("kstep", ib, j, k, i, c)     element (i, c) of S(ib, j) misses the whole contribution of k-step k;
  ("no_refine",)                the refinement step of (d) is left out."""
import numpy as np

import _factor_ref as R

BLK = R.BLK
LOG_2PI = float(np.log(2 * np.pi))


def _factor_block(S):
    """(L, W = L^-1, first non-positive pivot or None) of one 16 x 16 block, four columns at a time as factor16 does
    (csrc/agp_lds_chol.hpp): the 4 x 4 diagonal sub-block is factored with reciprocal roots and its factor inverted (W4), the
    columns are S[:, sub] W4', the trailing columns are updated, and an identity block rides along below — what happens to the rows
    below the diagonal turns it into L^-T, whose transpose is the explicit inverse the panel and the solve multiply by."""
    Y = np.array(S); m = Y.shape[0]
    X = np.eye(m)
    L = np.zeros_like(Y); Xo = np.zeros_like(Y)
    for s in range(0, m, 4):
        D = Y[s:s + 4, s:s + 4].copy()
        L4 = np.zeros((4, 4))
        for c in range(4):
            d = D[c, c]
            if not d > 0:
                return None, None, s + c
            ri = 1.0 / np.sqrt(d)
            L4[c:, c] = D[c:, c] * ri
            D[c + 1:, c + 1:] -= np.outer(L4[c + 1:, c], L4[c + 1:, c])
        W4 = R.tri_inv(L4)
        Lc = Y[:, s:s + 4] @ W4.T
        Lc[:s] = 0.0
        Lc[s:s + 4] = L4
        Xc = X[:, s:s + 4] @ W4.T
        L[:, s:s + 4] = Lc; Xo[:, s:s + 4] = Xc
        Y[:, s + 4:] -= Lc @ Lc[s + 4:].T
        X[:, s + 4:] -= Xc @ Lc[s + 4:].T
    return L, np.ascontiguousarray(Xo.T), None


def long_factor(K, y=None, fault=None):
    """-> (L (n, n), alpha (n), (2 sum log L_ii, alpha'alpha), logpdf, info); after a bad pivot L and alpha are None, logpdf NaN"""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]; nb = (n + BLK - 1) // BLK; npad = nb * BLK
    A = np.eye(npad); A[:n, :n] = np.tril(K) + np.tril(K, -1).T
    r = np.zeros(npad)
    if y is not None:
        r[:n] = y
    L = np.zeros((npad, npad)); alpha = np.zeros(npad)
    kind = fault[0] if fault else None
    for j in range(nb):
        j0, j1 = j * BLK, (j + 1) * BLK
        S = A[j0:, j0:j1].copy()
        for k in range(j):
            k0 = k * BLK
            for s in range(0, BLK, 4):
                upd = L[j0:, k0 + s:k0 + s + 4] @ L[j0:j1, k0 + s:k0 + s + 4].T
                if kind == "kstep" and fault[2] == j and fault[3] == k:
                    upd[(fault[1] - j) * BLK + fault[4], fault[5]] = 0.0
                S -= upd
        Ljj, W, bad = _factor_block(S[:BLK])
        if bad is not None:
            return None, None, (np.nan, np.nan), np.nan, j0 + bad + 1
        L[j0:j1, j0:j1] = Ljj
        P = S[BLK:] @ W.T
        if kind == "scale" and fault[2] == j:
            P[(fault[1] - j - 1) * BLK + fault[3], fault[4]] *= 1.0 + fault[5]
        L[j1:, j0:j1] = P
        a = W @ r[j0:j1]
        if kind != "no_refine":
            a = a + W @ (r[j0:j1] - Ljj @ a)
        alpha[j0:j1] = a
        r[j1:] -= P @ a
    ld = float(2.0 * np.log(np.diag(L)).sum()); ss = float(alpha @ alpha)
    return L[:n, :n], alpha[:n], (ld, ss), -0.5 * (n * LOG_2PI + ld + ss), 0
