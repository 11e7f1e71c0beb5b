"""NumPy restatement of the engine's factor update for removed observations (csrc/agp_remove_kernel.hpp), test infrastructure.

Deleting the run [a, b) of r rows from a factored series replaces the trailing triangle S = L[b:, b:] by S' with
S' S'^T = S S^T + W W^T, W = L[b:, a:b].  The update runs on the NEW row grid in 128-wide panels: per panel the
triangular-pentagonal LQ of [S_JJ | W_J] (row j's Householder reflector folds W_J[j, :] into the diagonal entry, which is
taken positive), the compact-WY factor T of the panel's reflectors, and [S_IJ | W_I] <- [S_IJ | W_I] (I - V T V^T),
V = [I; V_w], for the rows below.  A pass handles at most `rmax` columns of W; a wider run takes several passes.  The
forward-solve vector alpha = L^-1 x rides along as one more row.  Several runs are handled first to last."""
import numpy as np

NB = 128
RMAX = 32
NEGLIGIBLE = 1e-40


def runs_of(idx):
    """The ascending positions as runs (a, r), each in the coordinates left by the runs before it."""
    idx = [int(i) for i in idx]
    runs, gone, i = [], 0, 0
    while i < len(idx):
        j = i + 1
        while j < len(idx) and idx[j] == idx[j - 1] + 1:
            j += 1
        runs.append((idx[i] - gone, j - i))
        gone += j - i
        i = j
    return runs


def touched_prefix(n_f, idx):
    """(touched, new prefix length) of a factor resident on the prefix n_f when the positions idx leave the series."""
    cnt = int(np.searchsorted(np.asarray(idx, dtype=np.int64), n_f, side="left"))
    return cnt > 0, n_f - cnt


def panel_lq(S, W):
    """Reflectors of the panel [S | W] (S lower triangular nb x nb, W nb x rc), applied to its own rows: returns
    (S', V_w (rc x nb), tau, T) with [S | W] Q = [S' | 0], Q = I - V T V^T, diag(S') > 0."""
    nb, rc = W.shape
    S = S.copy(); W = W.copy()
    Vw = np.zeros((rc, nb)); tau = np.zeros(nb)
    for j in range(nb):
        xn = float(W[j] @ W[j])
        al = S[j, j]
        if xn > al * al * NEGLIGIBLE:      # (underflowed rows of W: 1 / xn would overflow, folding them changes nothing)
            beta = np.sqrt(al * al + xn)          # the positive root: no sign flip afterwards, no cancellation (al > 0)
            apb = al + beta
            tau[j] = xn / (apb * beta)
            Vw[:, j] = -W[j] * (apb / xn)
            S[j, j] = beta
            s = S[j + 1:, j] + W[j + 1:] @ Vw[:, j]
            S[j + 1:, j] -= tau[j] * s
            W[j + 1:] -= np.outer(tau[j] * s, Vw[:, j])
            W[j] = 0.0
    # compact WY, forward columnwise (dlarft): V^T V's strictly upper part is V_w^T V_w (the unit parts are orthogonal)
    T = np.zeros((nb, nb))
    G = Vw.T @ Vw
    for j in range(nb):
        T[j, j] = tau[j]
        if j > 0:
            T[:j, j] = -tau[j] * (T[:j, :j] @ G[:j, j])
    return S, Vw, tau, T


def apply_wy(S, W, Vw, T):
    """[S | W] <- [S | W] (I - V T V^T) for rows outside the panel: the three products of the apply kernel."""
    M = S + W @ Vw
    N = M @ T
    return S - N, W - N @ Vw.T


def remove_run(L, alpha, a, r, rmax=RMAX, nb=NB):
    """Factor and forward-solve vector of the series without rows [a, a + r)."""
    n_old = L.shape[0]
    n_new = n_old - r
    o = np.concatenate([np.arange(a), np.arange(a + r, n_old)])
    Ln = np.tril(L[np.ix_(o, o)])
    al = alpha[o].copy()
    J0 = (a // nb) * nb
    for c0 in range(0, r, rmax):
        rc = min(rmax, r - c0)
        W = np.zeros((n_new, rc))
        W[a:] = L[a + r:, a + c0:a + c0 + rc]
        g = alpha[a + c0:a + c0 + rc].copy()
        for j0 in range(J0, n_new, nb):
            j1 = min(j0 + nb, n_new)
            Sj, Vw, tau, T = panel_lq(Ln[j0:j1, j0:j1], W[j0:j1])
            Ln[j0:j1, j0:j1] = Sj
            W[j0:j1] = 0.0
            if j1 < n_new:
                Ln[j1:, j0:j1], W[j1:] = apply_wy(Ln[j1:, j0:j1], W[j1:], Vw, T)
            ar, gr = apply_wy(al[None, j0:j1], g[None, :], Vw, T)
            al[j0:j1] = ar[0]; g = gr[0]
    return Ln, al


def remove_rows(L, alpha, idx, rmax=RMAX, nb=NB):
    for a, r in runs_of(idx):
        L, alpha = remove_run(L, alpha, a, r, rmax, nb)
    return L, alpha
