"""Host reference of the removal-update probe (tests/test_remove_probe_cpu.py, tests/test_gpu_remove_probe.py,
tools/gpu_remove_probe_accuracy.py): the factors the probe is fed, the removal patterns, the 80-bit target of an update, its
row-wise backward-error metrics, the reference routes that set the bound, and a copy of the reference route with planted faults.
Plain NumPy, no engine code.

The target of an update is the caller's factor itself, not its matrix: with keep = the positions that stay,
    M = (L0 L0')[keep, keep]   and   y = (L0 alpha0)[keep]     (np.longdouble)
are what the updated pair must reproduce, L' L'' = M and L' alpha' = y.  A Householder update is stable row-wise, not
componentwise, so the metrics are (gamma_k of _factor_ref)
    eta(L')           = max_ij |M - L' L''|_ij / sqrt(M_ii M_jj)
    eta_s(L', alpha') = max_i |L' alpha' - y|_i / (||L'_i||_2 ||alpha'||_2)
and the bound of a case comes from two float64 routes of tests/_chol_remove_ref.py on the same input — reflector by reflector
(nb = 1, rmax = 32), and with the run's columns also taken one at a time (nb = 1, rmax = 1): with R, R_s the larger of the two
routes' eta, eta_s the device must meet eta <= 4 max(R, 2 gamma_{n'+1}) and eta_s <= 4 max(R_s, 2 gamma_{n'}) (two bits for a
summation order that is neither route's; the floor keeps a case where the routes happen to be exact from demanding exactness)."""
import numpy as np

import _chol_remove_ref as C
import _factor_ref as F

LD = F.LD
FAMILIES = F.FAMILIES + ("se_short",)
SENTINEL = -7.0
NB = 128


def matrix(fam, n):
    if fam == "se_short":      # length scale 0.01 on a regular grid, noise 1e-6: a factor with exact zeros and denormals far from the diagonal
        t = np.linspace(0.0, 1.0, n)
        return np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.01 ** 2) + 1e-6 * np.eye(n)
    return F.family(fam, n, 0)


_FACTORS = {}


def factor(fam, n):
    """(L0, alpha0): numpy's Cholesky factor of the family's matrix and L0^-1 z, z standard normal (read-only, computed once)"""
    if (fam, n) not in _FACTORS:
        L0 = np.linalg.cholesky(matrix(fam, n))
        z = np.random.default_rng([11, n, FAMILIES.index(fam)]).standard_normal(n)
        a0 = np.linalg.solve(L0, z)
        L0.setflags(write=False); a0.setflags(write=False)
        _FACTORS[(fam, n)] = (L0, a0)
    return _FACTORS[(fam, n)]


PATTERNS = {
    2: {"first": [0], "last": [1]},
    17: {"first": [0], "scattered": [2, 9, 15], "all_but_first": list(range(1, 17))},
    129: {"first": [0], "last": [128], "across_tile": [126, 127, 128]},
    257: {"first": [0], "last": [256]},                              # both leave exactly two tile rows
    384: {"tile_row": list(range(256, 384))},                        # a whole tile row at the end: the update returns early
    300: {"first": [0], "front2": [0, 1], "front3": list(range(3)), "front8": list(range(8)), "front9": list(range(9)),
          "front32": list(range(32)),
          "r33": list(range(3, 36)),                                 # 32 + 1: the second pass has one column
          "r40": list(range(5, 45)),                                 # 32 + 8
          "r128": list(range(1, 129)),                               # four passes
          "across_tile": [126, 127, 128], "tile_start": [128], "last": [299], "tail5": list(range(295, 300)),
          "three_runs": [40, 41, 130, 250, 251, 252], "all_but_first": list(range(1, 300)),
          "comb64": list(range(0, 128, 2))},                         # 64 runs one after another: the accumulation case
}
CASES = [(n, name) for n in (2, 17, 129, 257, 300, 384) for name in PATTERNS[n]]


# Replaced case (the reference routes must stay within 2 gamma / 4 gamma on every case, tests/test_remove_probe_cpu.py): spec at
# n = 2 has L0_11 ~ 1e-5, so alpha0 = L0^-1 z is ~1e5 long while alpha' after removing position 0 is of order 1 — the reflector's
# rounding scales with ||alpha0|| and eta_s measures against ||alpha'||: both reference routes sit near 1.5e5 gamma_1 there.  That
# case keeps its factor and takes alpha0 = z itself.
ALPHA_IS_Z = {("spec", 2, "first")}


def inputs(fam, n, name):
    """(L0, alpha0) of a case"""
    L0, a0 = factor(fam, n)
    if (fam, n, name) in ALPHA_IS_Z:
        a0 = np.random.default_rng([11, n, FAMILIES.index(fam)]).standard_normal(n)
        a0.setflags(write=False)
    return L0, a0


def batch_inputs(n, name):
    """the six families' factors of a case stacked: (L0 (6, n, n), alpha0 (6, n))"""
    both = [inputs(fam, n, name) for fam in FAMILIES]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def keep_of(n, idx):
    return np.setdiff1d(np.arange(n), np.asarray(idx, dtype=np.int64))


def returns_early(n, idx):
    """whether every run of the removal finds its first tile row beyond the new grid (the update then leaves the slot as it is)"""
    n_cur = n
    for a, r in C.runs_of(idx):
        if a // NB < -(-(n_cur - r) // NB):
            return False
        n_cur -= r
    return True


def target(L0, alpha0, idx):
    """(M, y) in longdouble"""
    keep = keep_of(L0.shape[0], idx)
    Lk = np.asarray(L0, dtype=LD)[keep]
    return Lk @ Lk.T, Lk @ np.asarray(alpha0, dtype=LD)


def eta(M, L):
    L = np.asarray(L, dtype=LD)
    d = np.sqrt(np.diag(M))
    return F._ratio_max(np.abs(M - L @ L.T), np.outer(d, d))


def eta_s(L, alpha, y):
    L = np.asarray(L, dtype=LD); alpha = np.asarray(alpha, dtype=LD)
    rows = np.sqrt((L * L).sum(axis=1)) * np.sqrt((alpha * alpha).sum())
    return F._ratio_max(np.abs(L @ alpha - y), rows)


def route_reflector(L0, alpha0, idx):
    return C.remove_rows(np.array(L0), np.array(alpha0), idx, rmax=32, nb=1)


def route_column(L0, alpha0, idx):
    return C.remove_rows(np.array(L0), np.array(alpha0), idx, rmax=1, nb=1)


def route_blocked(L0, alpha0, idx):
    return C.remove_rows(np.array(L0), np.array(alpha0), idx, rmax=8, nb=16)


def route_wy128(L0, alpha0, idx):
    return C.remove_rows(np.array(L0), np.array(alpha0), idx)


def route_lapack(M, y):
    """numpy's Cholesky of the rounded target and a solve with it: for information, never part of a bound"""
    L = np.linalg.cholesky(np.asarray(M, dtype=np.float64))
    return L, np.linalg.solve(L, np.asarray(y, dtype=np.float64))


_REFS = {}


def reference(fam, n, name):
    """dict(M, y, n_new, R, R_s, bound, bound_s) of a case, computed once and never modified"""
    key = (fam, n, name)
    if key not in _REFS:
        L0, a0 = inputs(fam, n, name)
        idx = PATTERNS[n][name]
        M, y = target(L0, a0, idx)
        n_new = n - len(idx)
        R = Rs = 0.0
        for route in (route_reflector, route_column):
            L, al = route(L0, a0, idx)
            R = max(R, eta(M, L)); Rs = max(Rs, eta_s(L, al, y))
        M.setflags(write=False); y.setflags(write=False)
        _REFS[key] = dict(M=M, y=y, n_new=n_new, R=R, R_s=Rs, bound=4 * max(R, 2 * F.gamma(n_new + 1)),
                          bound_s=4 * max(Rs, 2 * F.gamma(n_new)))
    return _REFS[key]


# ---- a copy of _chol_remove_ref.remove_run with planted faults ------------------------------------------------------------------
def faulty_rows(L, alpha, idx, fault=None, rmax=32, nb=1, taus=None):
    """_chol_remove_ref.remove_rows statement by statement (fault = None: the same bits), with one of
      ("skip_row", run, pass, j, i)   the reflectors of the panel at column j of that pass are not applied to row i below it
      ("tau", run, pass, j, s)        the compact-WY factor T of the panel at column j scaled by s (nb = 1: tau_j itself)
      ("src_row",)                    first run: the source row at a taken from old row a + r - 1
      ("drop_carried",)               first run: the run's alpha entries read zero from the second pass on
      ("skip_w", c)                   first run, first pass: column c of W zero in the second tile row
    taus: a list that receives (tau, run, pass, j) of every reflector."""
    kind = fault[0] if fault else None
    for ri, (a, r) in enumerate(C.runs_of(idx)):
        n_old = L.shape[0]
        n_new = n_old - r
        o = np.concatenate([np.arange(a), np.arange(a + r, n_old)])
        orow = o.copy()
        if kind == "src_row" and ri == 0 and a < n_new:
            orow[a] = a + r - 1
        Ln = np.tril(L[np.ix_(orow, o)])
        al = alpha[o].copy()
        J0 = (a // nb) * nb
        for pi, c0 in enumerate(range(0, r, rmax)):
            rc = min(rmax, r - c0)
            W = np.zeros((n_new, rc))
            W[a:] = L[orow[a:] if pi == 0 else o[a:], a + c0:a + c0 + rc]
            g = alpha[a + c0:a + c0 + rc].copy()
            if kind == "drop_carried" and ri == 0 and pi > 0:
                g[:] = 0.0
            if kind == "skip_w" and ri == 0 and pi == 0 and fault[1] < rc:
                W[NB:2 * NB, fault[1]] = 0.0
            for j0 in range(J0, n_new, nb):
                j1 = min(j0 + nb, n_new)
                Sj, Vw, tau, T = C.panel_lq(Ln[j0:j1, j0:j1], W[j0:j1])
                if taus is not None:
                    taus.extend((float(t), ri, pi, j0 + q) for q, t in enumerate(tau))
                if kind == "tau" and fault[1:4] == (ri, pi, j0):
                    T = T * fault[4]
                Ln[j0:j1, j0:j1] = Sj
                W[j0:j1] = 0.0
                if j1 < n_new:
                    hit = kind == "skip_row" and fault[1:4] == (ri, pi, j0) and j1 <= fault[4] < n_new
                    if hit:
                        keep_s, keep_w = Ln[fault[4], j0:j1].copy(), W[fault[4]].copy()
                    Ln[j1:, j0:j1], W[j1:] = C.apply_wy(Ln[j1:, j0:j1], W[j1:], Vw, T)
                    if hit:
                        Ln[fault[4], j0:j1], W[fault[4]] = keep_s, keep_w
                ar, gr = C.apply_wy(al[None, j0:j1], g[None, :], Vw, T)
                al[j0:j1] = ar[0]; g = gr[0]
        L, alpha = Ln, al
    return L, alpha
