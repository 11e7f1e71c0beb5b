"""Host reference of the factor probe tests (tests/test_factor_ref_cpu.py, tests/test_gpu_factor_probe.py): backward-error
metrics of a Cholesky factor and of a forward substitution in np.longdouble (64-bit significand on x86-64), the seeded matrix
families the tests feed the engine, and matrices with a known first non-positive pivot.  Plain NumPy, no engine code.

With u = 2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.):
  omega(K, L)          = max_ij |K - L L'|_ij / (|L| |L|')_ij      <= gamma_{n+1} for any standard Cholesky (Theorem 10.3)
  omega_solve(L, b, y) = max_i |L b - y|_i / (|L| |b|)_i          <= gamma_n for substitution (Theorem 8.5)
  kappa_blk(L)         = max over the 16 x 16 diagonal blocks of || |L_bb^-1| |L_bb| ||_inf: the factor by which an algorithm that
                         multiplies by explicit inverses of those blocks may legitimately exceed the two bounds."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FAMILIES = ("wishart", "graded", "spec", "se_grid", "se_irreg")
BLK = 16


def gamma(k):
    return k * U / (1.0 - k * U)


def _ratio_max(num, den):
    """max num / den over the entries; an entry with den = 0 must have num = 0 (else inf)."""
    num = np.asarray(num, dtype=LD); den = np.asarray(den, dtype=LD)
    if not np.isfinite(num).all() or not np.isfinite(den).all():
        return float("inf")
    pos = den > 0
    if (num[~pos] != 0).any():
        return float("inf")
    return float((num[pos] / den[pos]).max()) if pos.any() else 0.0


def omega(K, L):
    """Componentwise backward error of the factor L (lower) of K; only the lower triangle of the residual is looked at (both
    sides are symmetric)."""
    K = np.asarray(K, dtype=LD); L = np.asarray(L, dtype=LD)
    A = np.abs(L)
    il = np.tril_indices(K.shape[0])
    return _ratio_max(np.abs(K - L @ L.T)[il], (A @ A.T)[il])


def omega_solve(L, beta, y):
    L = np.asarray(L, dtype=LD); beta = np.asarray(beta, dtype=LD); y = np.asarray(y, dtype=LD)
    return _ratio_max(np.abs(L @ beta - y), np.abs(L) @ np.abs(beta))


def tri_inv(T):
    """Inverse of a lower triangular matrix by substitution, in the dtype of T."""
    m = T.shape[0]
    X = np.zeros_like(T)
    for j in range(m):
        X[j, j] = 1 / T[j, j]
        for i in range(j + 1, m):
            X[i, j] = -(T[i, j:i] @ X[j:i, j]) / T[i, i]
    return X


def kappa_blk(L, blk=BLK):
    L = np.asarray(L, dtype=LD); n = L.shape[0]
    worst = 0.0
    for b0 in range(0, n, blk):
        T = L[b0:b0 + blk, b0:b0 + blk]
        worst = max(worst, float((np.abs(tri_inv(T)) @ np.abs(T)).sum(axis=1).max()))
    return worst


def ref_chol(K):
    """Lower Cholesky factor in longdouble (outer-product form); raises ArithmeticError at a non-positive pivot."""
    A = np.array(K, dtype=LD); n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j]
        if not d > 0:
            raise ArithmeticError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def ref_forward(L, y, skip_block=None, blk=BLK):
    """beta = L^-1 y by blocked substitution in the dtype of L; skip_block = (ib, jb): the contribution of block (ib, jb) of L to
    rows ib is left out (a planted fault)."""
    n = L.shape[0]
    beta = np.zeros(n, dtype=L.dtype)
    for i0 in range(0, n, blk):
        i1 = min(n, i0 + blk)
        r = np.array(y[i0:i1], dtype=L.dtype)
        for j0 in range(0, i0, blk):
            if skip_block == (i0 // blk, j0 // blk):
                continue
            r -= L[i0:i1, j0:j0 + blk] @ beta[j0:j0 + blk]
        for i in range(i0, i1):
            beta[i] = (r[i - i0] - L[i, i0:i] @ beta[i0:i]) / L[i, i]
    return beta


# ---- matrix families (float64, exactly symmetric, positive definite at every size the tests use) ----------------------------
def _sym(K):
    return np.ascontiguousarray(0.5 * (K + K.T))


def _wishart(n, rng):
    M = rng.standard_normal((n, n))
    return _sym(M @ M.T / n + 0.5 * np.eye(n))


def family(name, n, seed=0):
    rng = np.random.default_rng([seed, n, FAMILIES.index(name)])
    if name == "wishart":
        return _wishart(n, rng)
    if name == "graded":                      # condition number ~ 2e12, benign diagonal blocks
        d = np.logspace(0.0, -6.0, n)
        return _sym(d[:, None] * _wishart(n, rng) * d[None, :])
    if name == "spec":                        # prescribed spectrum 1 .. 1e-10
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        return _sym((Q * np.logspace(0.0, -10.0, n)) @ Q.T)
    if name == "se_grid":                     # squared exponential on a regular grid, noise 1e-8
        t = np.linspace(0.0, 1.0, n)
        return _sym(np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.09) + 1e-8 * np.eye(n))
    if name == "se_irreg":                    # squared exponential on irregular times, noise 1e-6
        t = np.sort(rng.random(n))
        return _sym(np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.04) + 1e-6 * np.eye(n))
    raise ValueError(name)


def batch_of_nine(n):
    """[(label, K)] x 9: the five families, then two more seeds each of wishart and se_irreg."""
    out = [(f, family(f, n, 0)) for f in FAMILIES]
    out += [("wishart", family("wishart", n, s)) for s in (1, 2)]
    out += [("se_irreg", family("se_irreg", n, s)) for s in (1, 2)]
    return out


def batch_rhs(n):
    """right-hand sides of the batch of nine, (9, n)"""
    return np.random.default_rng(1000 + n).standard_normal((9, n))


def indefinite(n, js, seed=0):
    """L0 D L0' with L0 unit lower triangular (small random sub-diagonal part) and D = I except D[j] = -1 for j in js: the
    pivots of an elimination are D's entries up to rounding (~1e-16), so the first non-positive one is min(js)."""
    rng = np.random.default_rng([seed, n, 977])
    L0 = np.eye(n, dtype=LD) + np.tril(rng.standard_normal((n, n)) * (0.3 / np.sqrt(n)), -1).astype(LD)
    d = np.ones(n, dtype=LD)
    d[list(js)] = -1
    return _sym(((L0 * d) @ L0.T).astype(np.float64))


def zero_pivot(n, j):
    K = np.eye(n)
    K[j, j] = 0.0
    return K
