"""Host reference of the Schur (Toeplitz) kernel probe (tests/test_toeplitz_probe_cpu.py, tests/test_gpu_toeplitz_probe.py,
tools/gpu_toeplitz_probe_accuracy.py): first-column families, first columns with chosen reflection coefficients, the 80-bit
targets, the float64 routes that set the bounds, the same routes with planted faults, metrics and bounds.  Plain NumPy, no engine
code.

A case is (mode, n, m): n consecutive grid points, m future points behind them (mode 2), N = n + m.  The first column the kernel
works on is  r_eff[0] = noise + Constant + WhiteNoise + tables[0],  r_eff[g] = Constant + tables[g]  (effective_column: the
kernel's own order of additions).  The right-hand sides are [x, e_first, 1, tau], tau_j = (rank0 + j - grid_mid) grid_h.

Targets (np.longdouble): up to 513 points ref_chol of the dense matrix; above, the O(n^2) Schur recursion in longdouble
(schur(..., dtype=LD): validated against the dense target and the closed forms by the CPU test).
Routes (float64): schur(mixed, recur) for the four combinations of
    direct rotation  vn = c (v - rho u)      |  mixed  vn = -rho un + sqrt(1 - rho^2) v
    pivot from u with a division             |  pivot and reciprocal carried as recurrences (the kernel header's)
R of a quantity is the largest error of the four on the same input; the bounds (gamma_k of _factor_ref):
    eta(T, L) = max |T - L L'|_ij / r0            <= 4 max(R, 2 gamma_{n+1})        (normwise: the algorithm is not componentwise stable)
    omega_solve(L_dev, fwd, rhs)                  <= 4 max(R_s, 2 gamma_n)
    omega_solve(L_dev', sol, fwd)                 <= 4 max(R_b, 2 gamma_n)          (R_b: plain substitution with the route's factor)
    end quantities (log|T|, b_x'b_x, logpdf, rows of pacc, sol) against the target:
        error <= 8 max(R, 2 gamma_{n+2} sum|terms|)   and   error <= the first-order effect of |dT|_ij <= 8 gamma_{n+1} r0."""
from decimal import Decimal, localcontext

import numpy as np

import _factor_ref as F
from _remove_probe_ref import eta

LD = F.LD
gamma = F.gamma
SENTINEL = -7.0
LGUARD = 16
LOG2PI = LD("1.8378770664093454835606594728112")
FAMILIES = ("ar1", "ar1_alt", "ma1", "ge1", "se_noise", "se_stiff", "per", "se_per", "const_wn", "refl")
BIG_FAMILIES = ("ar1", "ge1", "se_per", "refl")
DENSE_MAX = 513

SIZES_01 = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 17, 255, 256, 257, 300, 513)
SIZES_0_BIG = (2048, 2049, 4096)
SIZES_2 = ((1, 1), (5, 3), (17, 0), (17, 40), (255, 2), (256, 1), (300, 213), (511, 2), (512, 1))
T_REF = 0.4
RANK0_MODE0 = 5


# ---- families ---------------------------------------------------------------------------------------------------------------
def family(fam, n, N=None):
    """dict(tab (N,), noise, const, wn): the family's first column on t = g / (n - 1), g = 0 .. N-1, as the probe is given it"""
    N = n if N is None else N
    g = np.arange(N, dtype=np.float64)
    t = g / max(n - 1, 1)
    d = dict(noise=0.0, const=np.nan, wn=np.nan)
    if fam == "ar1":
        d["tab"] = 0.9 ** g
    elif fam == "ar1_alt":
        d["tab"] = (-0.99) ** g
    elif fam == "ma1":
        tab = np.zeros(N); tab[0] = 1.81
        if N > 1:
            tab[1] = -0.9
        d["tab"] = tab
    elif fam == "ge1":
        d["tab"] = np.exp(-t / 0.2); d["noise"] = 1e-6
    elif fam == "se_noise":
        d["tab"] = np.exp(-0.5 * (t / 0.1) ** 2); d["noise"] = 1e-6
    elif fam == "se_stiff":
        d["tab"] = np.exp(-0.5 * (t / 0.3) ** 2); d["noise"] = 1e-8
    elif fam == "per":
        d["tab"] = np.exp(-2.0 * np.sin(np.pi * t / 0.13) ** 2 / 0.25); d["noise"] = 1e-4
    elif fam == "se_per":
        d["tab"] = np.exp(-0.5 * (t / 0.5) ** 2) * np.exp(-2.0 * np.sin(np.pi * t / 0.17) ** 2 / 0.6); d["noise"] = 1e-5
    elif fam == "const_wn":
        d["tab"] = np.zeros(N); d["const"] = 2.0; d["wn"] = 0.01
    elif fam == "refl":
        d["tab"] = refl_column(N); d["noise"] = 0.05
    else:
        raise ValueError(fam)
    return d


_REFL = {}


def refl_column(N):
    """A column defined by its reflection coefficients, not by a kernel: +-0.4 at columns 1, 2 and at 256 q - 1, 256 q, 256 q + 1,
    seeded values in +-0.02 elsewhere (the family adds a noise of 0.05, which
    bounds the condition number at every size and takes a little off every coefficient).  The kernel families' coefficients have decayed to rounding level by column 256 (a rotation
    there is the identity, and a fault in the indexing at a register boundary changes nothing): this one rotates where the owner of
    the pivot changes register.  Nested: the first n entries are the column of size n."""
    if not _REFL or _REFL["r"].size < N:
        M = max(N, 4096)
        rho = np.random.default_rng([8, 8]).uniform(-0.02, 0.02, M).astype(LD)
        k = np.arange(M)
        big = (k == 1) | (k == 2) | ((k >= 255) & np.isin(k % 256, (255, 0, 1)))
        rho[big] = np.where(k[big] % 2 == 0, LD("0.4"), LD("-0.4"))
        _REFL["r"] = np.asarray(inverse_schur(rho), dtype=np.float64)
    return _REFL["r"][:N].copy()


def effective_column(tab, noise, const=np.nan, wn=np.nan, tab2=None):
    """the first column the kernel forms, in its order of additions (float64)"""
    r_all = 0.0 if np.isnan(const) else float(const)
    r_zero = 0.0 if np.isnan(wn) else float(wn)
    r = r_all + np.asarray(tab, dtype=np.float64)
    r0 = noise + r_all + r_zero + tab[0]
    if tab2 is not None:
        r = r + tab2
        r0 = r0 + tab2[0]
    r = np.array(r); r[0] = r0
    return r


def split_tables(tab):
    """(a, b) with a + b == tab bit for bit in either order: a = tab rounded to float32"""
    a = np.asarray(tab, dtype=np.float32).astype(np.float64)
    b = tab - a
    assert np.array_equal(a + b, tab) and np.array_equal(0.0 + a + b, tab)
    return a, b


def rhs_x(n):
    return np.random.default_rng(4000 + n).standard_normal(n)


def grid_of(n):
    """(grid_h, grid_mid): the points of a case sit at t - t_ref = (rank0 + j - grid_mid) grid_h, roughly on [-T_REF, 1 - T_REF]"""
    return 1.0 / max(n - 1, 1), T_REF * max(n - 1, 1) + 0.25


def tau_of(n, N, rank0):
    h, mid = grid_of(n)
    return ((np.arange(N, dtype=np.float64) + rank0) - mid) * h


# Linear leaves of the four variants of every family in a call (centre, bias, amp): none; one centred at t_ref; two, left of and far
# right of t_ref; one with zero amplitude (C has one non-zero entry) — that variant also gets its table split in two
VARIANTS = ((), ((T_REF, 0.5, 1.2),), ((T_REF - 0.7, 0.2, 0.8), (T_REF + 50.0, 0.0, 1e-3)), ((T_REF + 0.1, 0.3, 0.0),))
SPLIT_VARIANT = 3


def lin_C(leaves, dtype=np.float64):
    C00 = C01 = C11 = dtype(0)
    for c, b, a in leaves:
        cc = dtype(c) - dtype(T_REF)
        C00 = C00 + (dtype(b) + dtype(a) * cc * cc); C01 = C01 - dtype(a) * cc; C11 = C11 + dtype(a)
    return C00, C01, C11


# ---- first columns with chosen reflection coefficients -------------------------------------------------------------------------
def inverse_schur(rho):
    """first column r (r[0] = 1, longdouble -> float64 and longdouble) of the Toeplitz matrix whose Schur parameters are
    rho[1 .. N-1] (rho[0] unused): the step-up recursion of Levinson-Durbin with k_m = -rho_m"""
    rho = np.asarray(rho, dtype=LD)
    N = rho.size
    r = np.zeros(N, dtype=LD); r[0] = 1
    a = np.zeros(N, dtype=LD)          # a[1 .. m-1]: predictor of order m - 1
    E = LD(1)
    for m in range(1, N):
        k = -rho[m]
        r[m] = -(k * E + (a[1:m] @ r[m - 1:0:-1] if m > 1 else LD(0)))
        new = a[1:m] + k * a[m - 1:0:-1]
        a[1:m] = new; a[m] = k
        E = E * (1 - k * k)
    return r


def planted_rho(N, k, value, quiet):
    """reflection coefficients with rho_k = value; before k zeros (quiet: the planted value is then exactly what the arithmetic
    sees) or seeded values in +-0.05 (small enough for the map from the column to rho_k to stay
    well conditioned up to k = 600: a planted 1 + 1e-9 must survive float64 rounding); zeros after k"""
    rho = np.zeros(N, dtype=LD)
    if not quiet and k > 1:
        rho[1:k] = np.random.default_rng([7, N, k]).uniform(-0.05, 0.05, k - 1)
    rho[k] = value
    return rho


# ---- the recursion: target above DENSE_MAX points (dtype LD), routes (float64), planted faults ---------------------------------
FAULTS_FORWARD = ("u_unshifted", "rho_sign", "pivot_late", "skip_rlo", "ge_gt", "e_zero")
FAULTS_LIN = ("c01_sign", "tau_no_rank0", "be_from_nm1")
FAULTS_BACK = ("tri_transposed", "missing_zero_pivot")
NT = 256


def schur(r_eff, x, n, N, rank0=0, dtype=np.float64, mixed=False, recur=True, store=False, fault=None):
    """The kernel's algorithm column by column.  -> dict(ok, bad_col, rho (N), diag (n: the pivots the solve used), L (n, n) if
    store, fwd (4, n), logdet, pacc (4, N - n))."""
    T_ = dtype
    r_eff = np.asarray(r_eff, dtype=T_)
    r0 = r_eff[0]
    ir0 = 1 / np.sqrt(r0)
    uu = r_eff * ir0
    v = uu.copy(); v[0] = 0
    tau = np.asarray(tau_of(n, N, 0 if fault == "tau_no_rank0" else rank0), dtype=T_)
    b = np.zeros((4, N), dtype=T_)
    b[0, :n] = np.asarray(x, dtype=T_); b[1, 0] = 0 if fault == "e_zero" else 1; b[2, :n] = 1; b[3, :n] = tau[:n]
    be = np.zeros(N, dtype=T_)
    babs = np.zeros((4, N), dtype=T_)          # sum |terms| of the rows of b (the floors of pacc)
    pu, ipu = r0 * ir0, ir0
    L = np.zeros((n, n), dtype=T_) if store else None
    fwd = np.zeros((4, n), dtype=T_)
    diag = np.zeros(n, dtype=T_); rhos = np.zeros(N, dtype=T_)
    out = dict(ok=False, bad_col=-1, rho=rhos, diag=diag, L=L, fwd=fwd)
    pub = v[0]                       # the published pivot entry of the coming step
    for k in range(N):
        vk = pub if fault == "pivot_late" else v[k]
        rho = vk * ipu if recur else vk / uu[0]
        om = (1 - rho) * (1 + rho)
        rhos[k] = rho
        if not om > 0:
            out["bad_col"] = k
            return out
        cs = 1 / np.sqrt(om)
        vv = v[k:]
        un = cs * (uu - rho * vv)
        if mixed:
            vn = -rho * un + (om * cs) * vv
        elif fault == "rho_sign":
            vn = cs * (vv + rho * uu)
        else:
            vn = cs * (vv - rho * uu)
        if recur:
            il = ipu * cs
            pu = pu * om * cs; ipu = il
            dk = pu
            un[0] = dk               # (entry k of the column is the recurrence's pivot wherever it is stored or summed)
        else:
            dk = un[0]; il = 1 / dk
        st = un                      # what is stored and summed; a skipped element stays as it was and stores nothing (reads 0)
        if fault == "ge_gt":
            un[0] = uu[0]; vn[0] = vv[0]
            st = un.copy(); st[0] = 0
        if fault == "skip_rlo" and k > 0 and k % NT == 0:
            un[:NT] = uu[:NT]; vn[:NT] = vv[:NT]
            st = un.copy(); st[:NT] = 0
        if k + 1 < N:
            pub = v[k + 1]           # (what a late publication leaves in the slot: the entry before this step's rotation)
        v[k:] = vn
        if k < n:
            diag[k] = dk
            y = b[:, k] * il
            fwd[:, k] = y
            if store:
                L[k:, k] = st[:n - k]
            b[:, k + 1:] -= np.outer(y, un[1:])
            if N > n:
                babs[:, n:] += np.outer(np.abs(y), np.abs(un[n - k:]))
            if fault == "be_from_nm1" and k == n - 1:
                be[k:] += st * st
        else:
            be[k:] += st * st
        uu = un[1:] if fault == "u_unshifted" else un[:-1]      # (element j + 1 reads what element j wrote)
    out["ok"] = True
    out["logdet"] = 2 * np.log(diag).sum()
    pacc = np.zeros((4, N - n), dtype=T_)
    pacc[0] = -b[0, n:]; pacc[1] = -b[2, n:]; pacc[2] = -b[3, n:]; pacc[3] = be[n:]
    out["pacc"] = pacc
    out["pacc_terms"] = babs[[0, 2, 3], n:]
    return out


def back_plain(L, fwd):
    """L' S = F by column-oriented substitution in the dtype of L"""
    n = L.shape[0]
    f = np.array(fwd); s = np.zeros_like(f)
    for k in range(n - 1, -1, -1):
        s[:, k] = f[:, k] / L[k, k]
        f[:, :k] -= np.outer(s[:, k], L[k, :k])
    return s


def back_blocked(L, fwd, fault=None):
    """the same in k_toep_back's order: blocks of four columns from the last one down, the dot products with the rows below the
    block first, then the block's triangle"""
    n = L.shape[0]
    y = np.zeros_like(fwd)
    for kb in range(n - 1, -1, -4):
        yb = np.zeros((4, 4), dtype=L.dtype)
        for c in range(4):
            col = kb - c
            ex = col >= 0
            if not ex and fault != "missing_zero_pivot":
                continue
            cc = max(col, 0)
            t = (fwd[:, cc] - y[:, kb + 1:] @ L[kb + 1:, cc]) if ex else np.zeros(4, dtype=L.dtype)
            for i in range(c):
                tri = L[kb - c, kb - i] if fault == "tri_transposed" else L[kb - i, cc]
                t = t - (tri if ex else 0) * yb[i]
            with np.errstate(all="ignore"):
                yb[c] = t / (L[cc, cc] if ex else L.dtype.type(0))
            y[:, cc] = yb[c]
    return y


def logpdf_from(n, logdet, fwd, leaves, dtype=np.float64, fault=None):
    """the kernel's closing statement: log N(x; 0, T + U C U') from log|T| and L^-1 [x, ., 1, tau]"""
    T_ = dtype
    yx, y1, yt = fwd[0], fwd[2], fwd[3]
    qf = yx @ yx; ld = logdet
    C00, C01, C11 = lin_C(leaves, T_)
    if fault == "c01_sign":
        C01 = -C01
    if C00 != 0 or C01 != 0 or C11 != 0:
        n00, n01, n11, w0, w1 = y1 @ y1, y1 @ yt, yt @ yt, y1 @ yx, yt @ yx
        m00 = 1 + n00 * C00 + n01 * C01; m01 = n00 * C01 + n01 * C11
        m10 = n01 * C00 + n11 * C01; m11 = 1 + n01 * C01 + n11 * C11
        det = m00 * m11 - m01 * m10
        z0 = (m11 * w0 - m01 * w1) / det; z1 = (m00 * w1 - m10 * w0) / det
        corr = w0 * (C00 * z0 + C01 * z1) + w1 * (C01 * z0 + C11 * z1)
        qf = qf - corr; ld = ld + np.log(det)
        extra = abs(np.log(det)) + abs(corr)
    else:
        extra = 0
    lp = -(T_(n) * T_(LOG2PI) + ld + qf) / 2
    return lp, extra


# ---- targets ---------------------------------------------------------------------------------------------------------------------
def toeplitz(r):
    r = np.asarray(r)
    i = np.arange(r.size)
    return r[np.abs(i[:, None] - i[None, :])]


def forward_ld(L, B):
    """L^-1 B (B: (k, n) rows) by column-oriented substitution in longdouble"""
    n = L.shape[0]
    f = np.array(B, dtype=LD); y = np.zeros_like(f)
    for k in range(n):
        y[:, k] = f[:, k] / L[k, k]
        f[:, k + 1:] -= np.outer(y[:, k], L[k + 1:, k])
    return y


def rhs_rows(x, n, N, rank0):
    tau = tau_of(n, N, rank0)
    B = np.zeros((4, n)); B[0] = x; B[1, 0] = 1.0; B[2] = 1.0; B[3] = tau[:n]
    return B


def target(r_eff, x, n, N, rank0=0, keep_L=True):
    """dict(L, fwd, sol, logdet, qxx, pacc, r0, rhs, dense): longdouble; ref_chol of the dense joint matrix up to DENSE_MAX points,
    the longdouble recursion above.  Raises ArithmeticError where the matrix is not positive definite."""
    r_ld = np.asarray(r_eff, dtype=LD)
    rhs = rhs_rows(x, n, N, rank0)
    pacc_terms = np.zeros((3, N - n), dtype=LD)
    if N <= DENSE_MAX:
        Lj = F.ref_chol(toeplitz(r_ld))
        L = Lj[:n, :n]
        fwd = forward_ld(L, rhs)
        pacc = np.zeros((4, N - n), dtype=LD)
        if N > n:
            L21, L22 = Lj[n:, :n], Lj[n:, n:]
            pacc[:3] = (L21 @ fwd[[0, 2, 3]].T).T
            pacc[3] = (L22 * L22).sum(axis=1)
            pacc_terms = (np.abs(L21) @ np.abs(fwd[[0, 2, 3]]).T).T
        logdet = 2 * np.log(np.diag(L)).sum()
    else:
        s = schur(r_ld, x, n, N, rank0, dtype=LD, recur=False, store=keep_L)
        if not s["ok"]:
            raise ArithmeticError(f"column {s['bad_col']}: |rho| >= 1")
        L, fwd, pacc, logdet = s["L"], s["fwd"], s["pacc"], s["logdet"]
        big_diag = s["diag"]; pacc_terms = s["pacc_terms"]
    sol = back_plain(L, fwd) if L is not None else None
    return dict(pacc_terms=pacc_terms, L=L, fwd=fwd, sol=sol, logdet=logdet, qxx=fwd[0] @ fwd[0], pacc=pacc, r0=r_ld[0], rhs=rhs, dense=N <= DENSE_MAX,
                diag=np.diag(L).copy() if L is not None else big_diag, n=n, N=N)


def target_hp(r_eff, x, n, N, rank0=0, digits=80):
    """target() in decimal arithmetic of `digits` digits (the recursion with the pivot from u), handed back in longdouble.  For
    columns whose condition number is beyond the longdouble recursion: with |rho_k| = 1 - 1e-12 planted, that recursion leaves the
    Schur complement's diagonal 4e-11 relative off (2^-64 times a condition number of 1e12 and the amplification of the future
    rows), forty times the bound it is the target of."""
    def dec(a):
        a = np.asarray(a, dtype=np.float64)
        return np.array([Decimal(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)

    def ld(a):
        a = np.asarray(a, dtype=object)
        return np.array([LD(str(v)) for v in a.ravel()], dtype=LD).reshape(a.shape)
    with localcontext() as ctx:
        ctx.prec = digits
        zero = Decimal(0)
        r = dec(r_eff)
        ir0 = 1 / r[0].sqrt()
        uu = r * ir0
        v = uu.copy(); v[0] = zero
        rhs = rhs_rows(x, n, N, rank0)
        b = dec(np.concatenate([rhs, np.zeros((4, N - n))], axis=1))
        babs = dec(np.zeros((4, N))); be = dec(np.zeros(N))
        L = dec(np.zeros((n, n))); fwd = dec(np.zeros((4, n))); diag = dec(np.zeros(n))
        for k in range(N):
            rho = v[k] / uu[0]
            om = (1 - rho) * (1 + rho)
            if not om > 0:
                raise ArithmeticError(f"column {k}: |rho| >= 1")
            cs = 1 / om.sqrt()
            vv = v[k:]
            un = cs * (uu - rho * vv)
            v[k:] = cs * (vv - rho * uu)
            if k < n:
                diag[k] = un[0]
                y = b[:, k] / un[0]
                fwd[:, k] = y
                L[k:, k] = un[:n - k]
                b[:, k + 1:] = b[:, k + 1:] - np.outer(y, un[1:])
                if N > n:
                    babs[:, n:] = babs[:, n:] + np.outer(np.abs(y), np.abs(un[n - k:]))
            else:
                be[k:] = be[k:] + un * un
            uu = un[:-1]
        f = fwd.copy(); sol = dec(np.zeros((4, n)))
        for k in range(n - 1, -1, -1):
            sol[:, k] = f[:, k] / L[k, k]
            f[:, :k] = f[:, :k] - np.outer(sol[:, k], L[k, :k])
        logdet = 2 * sum(d.ln() for d in diag)
        qxx = sum(fwd[0] * fwd[0])
        pacc = np.zeros((4, N - n), dtype=LD)
        if N > n:
            pacc[0], pacc[1], pacc[2], pacc[3] = ld(-b[0, n:]), ld(-b[2, n:]), ld(-b[3, n:]), ld(be[n:])
        return dict(pacc_terms=ld(babs[[0, 2, 3], n:]) if N > n else np.zeros((3, 0), dtype=LD), L=ld(L), fwd=ld(fwd), sol=ld(sol),
                    logdet=LD(str(logdet)), qxx=LD(str(qxx)), pacc=pacc, r0=LD(str(r[0])), rhs=rhs, dense=False, diag=ld(diag), n=n, N=N)


def target_logpdf(tg, leaves):
    """(logpdf, sum |terms|) of T + U C U' from a target"""
    lp, extra = logpdf_from(tg["n"], tg["logdet"], tg["fwd"], leaves, dtype=LD)
    abs_ld = 2 * np.abs(np.log(tg["diag"])).sum()
    return lp, (tg["n"] * LOG2PI + abs_ld + tg["qxx"] + extra) / 2


def dense_logpdf(r_eff, x, n, rank0, leaves):
    """log N(x; 0, T + U C U') by a dense longdouble Cholesky of the full matrix (validates the update form the targets use)"""
    tau = np.asarray(tau_of(n, n, rank0), dtype=LD)
    C00, C01, C11 = lin_C(leaves, LD)
    one = np.ones(n, dtype=LD)
    K = toeplitz(np.asarray(r_eff, dtype=LD)) + C00 * np.outer(one, one) + C01 * (np.outer(one, tau) + np.outer(tau, one)) + C11 * np.outer(tau, tau)
    L = F.ref_chol(K)
    y = forward_ld(L, np.asarray(x, dtype=LD)[None, :])[0]
    return -(n * LOG2PI + 2 * np.log(np.diag(L)).sum() + y @ y) / 2


# ---- metrics -----------------------------------------------------------------------------------------------------------------------
def eta_full(r_eff, L, blk=64):
    """eta of _remove_probe_ref on the lower triangle, block by block (a longdouble product has no BLAS: rows of block I times rows
    of block J <= I need only the columns up to the end of J)"""
    n = L.shape[0]
    if n <= 2 * blk:
        return eta(toeplitz(np.asarray(r_eff, dtype=LD)[:n]), L)
    Ll = np.asarray(L, dtype=LD)
    if not np.isfinite(Ll).all():
        return float("inf")
    T = toeplitz(np.asarray(r_eff, dtype=LD)[:n])
    worst = LD(0)
    for i0 in range(0, n, blk):
        for j0 in range(0, i0 + 1, blk):
            j1 = min(n, j0 + blk)
            worst = max(worst, np.abs(T[i0:i0 + blk, j0:j1] - Ll[i0:i0 + blk, :j1] @ Ll[j0:j1, :j1].T).max())
    return float(worst / T[0, 0])


def sample_entries(n):
    """the fixed sample of entries (i, j), i >= j, of the large cases: the diagonal, the last row, rows 255 to 257 and 2047, and 4096
    seeded random pairs"""
    i = [np.arange(n)]; j = [np.arange(n)]
    for row in (n - 1, 255, 256, 257, 2047):
        if row < n:
            i.append(np.full(row + 1, row)); j.append(np.arange(row + 1))
    rng = np.random.default_rng([99, n])
    a, b = rng.integers(0, n, 4096), rng.integers(0, n, 4096)
    i.append(np.maximum(a, b)); j.append(np.minimum(a, b))
    return np.concatenate(i), np.concatenate(j)


def eta_sampled(r_eff, L, chunk=512):
    r_ld = np.asarray(r_eff, dtype=LD)
    Ll = np.asarray(L, dtype=LD)
    if not np.isfinite(Ll).all():
        return float("inf")
    i, j = sample_entries(L.shape[0])
    worst = LD(0)
    for c0 in range(0, i.size, chunk):
        ii, jj = i[c0:c0 + chunk], j[c0:c0 + chunk]
        prod = np.einsum("ek,ek->e", Ll[ii], Ll[jj])
        worst = max(worst, np.abs(r_ld[ii - jj] - prod).max())
    return float(worst / r_ld[0])


def eta_of(r_eff, L):
    return eta_full(r_eff, L) if L.shape[0] <= DENSE_MAX else eta_sampled(r_eff, L)


def rel_max(a, b):
    """max |a - b| / max |b| (sol: a normwise figure per right-hand side would hide nothing the entries do not show at these sizes)"""
    a = np.asarray(a, dtype=LD); b = np.asarray(b, dtype=LD)
    if not np.isfinite(a).all():
        return float("inf")
    return float(np.abs(a - b).max() / np.abs(b).max())


def quantities(tg, res, leaves_list, lin_rows):
    """errors of a result (a route's or the device's: dict(L, fwd, sol, logdet or None, qxx, lps, pacc)) against the target:
    dict name -> error.  lin_rows: whether rows 1 and tau of fwd / sol / pacc were solved (a particle with Linear leaves)."""
    n = tg["n"]
    e = {}
    rows = [0, 1, 2, 3] if lin_rows else [0, 1]
    if res.get("L") is not None:
        Ld = np.asarray(res["L"], dtype=LD)
        e["solve_f"] = F.omega_solve(Ld, np.asarray(res["fwd"], dtype=LD)[rows].T, tg["rhs"][rows].T)
        if res.get("sol") is not None:
            e["solve_b"] = F.omega_solve(Ld.T, np.asarray(res["sol"], dtype=LD)[rows].T, np.asarray(res["fwd"], dtype=LD)[rows].T)
            for m in rows:
                e[f"sol{m}"] = rel_max(res["sol"][m], tg["sol"][m])
    if res.get("logdet") is not None:
        e["logdet"] = float(abs(LD(res["logdet"]) - tg["logdet"]))
    if res.get("qxx") is not None:
        e["qxx"] = float(abs(LD(res["qxx"]) - tg["qxx"]))
    for vi, lp in res.get("lps", {}).items():
        e[f"lp{vi}"] = float(abs(LD(lp) - target_logpdf(tg, leaves_list[vi])[0]))
    if res.get("pacc") is not None and tg["N"] > n:
        pr = [0, 1, 2, 3] if lin_rows else [0, 3]
        for m in pr:
            e[f"pacc{m}"] = float(np.abs(np.asarray(res["pacc"][m], dtype=LD) - tg["pacc"][m]).max()) if np.isfinite(res["pacc"][m]).all() else float("inf")
    return e


def floors(tg, leaves_list):
    """2 gamma_{n+2} sum|terms| of every end quantity"""
    n = tg["n"]
    g2 = 2 * gamma(n + 2)
    f = {"qxx": g2 * float(tg["qxx"])}
    f["logdet"] = g2 * float(2 * np.abs(np.log(tg["diag"])).sum())
    for vi, lv in enumerate(leaves_list):
        f[f"lp{vi}"] = g2 * float(target_logpdf(tg, lv)[1])
    for m in range(4):
        f[f"sol{m}"] = g2
    return f


def caps(r_eff, tg):
    """first-order effect of a perturbation |dT|_ij <= 8 gamma_{n+1} r0 on log|T|, b_x'b_x, sol (per right-hand side, in the metric of
    rel_max) and the log density WITHOUT Linear leaves (lp0); the rows of pacc get theirs from pacc_floor_cap.  Not capped: the log
    densities of the variants with Linear leaves (lp1 to lp3: 8 max(R, floor) alone), and every quantity of mode 0 above DENSE_MAX
    points, where no factor is kept.  The inverse is float64 at every size (its own error, cond u relative — 3e-6 at most on these
    families — is far inside the factor 8; a longdouble inverse at 513 points costs seconds per family and case)."""
    n = tg["n"]
    eps = 8 * gamma(n + 1) * float(tg["r0"])
    Ti = np.abs(np.linalg.inv(toeplitz(np.asarray(r_eff, dtype=np.float64)[:n])))
    c = {"logdet": eps * Ti.sum()}
    s = np.abs(np.asarray(tg["sol"], dtype=np.float64))
    c["qxx"] = eps * s[0].sum() ** 2
    row = Ti.sum(axis=1).max()
    for m in range(4):
        c[f"sol{m}"] = eps * row * s[m].sum() / s[m].max() if s[m].max() > 0 else np.inf
    c["lp0"] = (c["logdet"] + c["qxx"]) / 2
    return c


def pacc_floor_cap(r_eff, tg):
    """floors (2 gamma_{n+2} sum|terms|) and caps of the rows of pacc, per row the largest over the future points (dense targets)"""
    n, N = tg["n"], tg["N"]
    g2 = 2 * gamma(n + 2)
    eps = 8 * gamma(n + 1) * float(tg["r0"])
    fl, cp = {}, {}
    Tf = toeplitz(np.asarray(r_eff, dtype=np.float64))
    W = np.abs(np.linalg.solve(Tf[:n, :n], Tf[:n, n:]).T)            # |T21 T11^-1|
    s = np.abs(np.asarray(tg["sol"], dtype=np.float64))
    for m, row in ((0, 0), (1, 2), (2, 3)):
        cp[f"pacc{m}"] = eps * ((W.sum(axis=1) + 1) * s[row].sum()).max()
        fl[f"pacc{m}"] = g2 * float(tg["pacc_terms"][m].max())
    cp["pacc3"] = eps * ((W.sum(axis=1) + 1) ** 2).max()
    fl["pacc3"] = g2 * float(np.abs(tg["pacc"][3]).max())
    return fl, cp


ROUTES = ((False, False), (False, True), (True, False), (True, True))      # (mixed, recur)
ROUTE_NAMES = ("direct/div", "direct/rec", "mixed/div", "mixed/rec")


def run_route(r_eff, x, n, N, rank0, mixed, recur, leaves_list, fault=None, store=True):
    """a route's result in the form quantities() takes (None where the route refuses)"""
    s = schur(r_eff, x, n, N, rank0, mixed=mixed, recur=recur, store=store, fault=fault if fault not in FAULTS_BACK else None)
    if not s["ok"]:
        return None
    res = dict(L=s["L"], fwd=s["fwd"], logdet=s["logdet"], qxx=s["fwd"][0] @ s["fwd"][0], pacc=s["pacc"], rho=s["rho"])
    if store:
        res["sol"] = back_blocked(s["L"], s["fwd"], fault) if fault in FAULTS_BACK else back_plain(s["L"], s["fwd"])
    res["lps"] = {vi: logpdf_from(n, s["logdet"], s["fwd"], lv, fault=fault)[0] for vi, lv in enumerate(leaves_list)}
    return res


_REFS = {}


def case_column(fam, n, N):
    d = family(fam, n, N)
    return d, effective_column(d["tab"], d["noise"], d["const"], d["wn"])


def build_reference(r_eff, x, n, m, rank0, store, leaves_list=VARIANTS, hp=False):
    """dict(r_eff, x, tg, R (name -> largest route error), routes (per route errors), bound (name -> bound), max_rho, admitted) of
    one first column.  store False: the logpdf quantities only (no factor is kept above DENSE_MAX points)."""
    N = n + m
    tg = target_hp(r_eff, x, n, N, rank0) if hp else target(r_eff, x, n, N, rank0, keep_L=store or N <= DENSE_MAX)
    R, per_route, max_rho, admitted = {}, [], 0.0, True
    for mixed, recur in ROUTES:
        res = run_route(r_eff, x, n, N, rank0, mixed, recur, leaves_list, store=store)
        if res is None:
            admitted = False
            per_route.append(None)
            continue
        max_rho = max(max_rho, float(np.abs(res["rho"]).max()))
        e = quantities(tg, res if store else {k: v for k, v in res.items() if k != "L"}, leaves_list, True)
        if store:
            e["eta"] = eta_of(r_eff, res["L"])
        per_route.append(e)
        for k, v in e.items():
            R[k] = max(R.get(k, 0.0), v)
    bound = {}
    if admitted:
        fl = floors(tg, leaves_list)
        cp = caps(r_eff, tg) if tg["sol"] is not None else {}
        if m > 0 and tg["sol"] is not None:
            f2, c2 = pacc_floor_cap(r_eff, tg)
            fl.update(f2); cp.update(c2)
        for k, v in R.items():
            if k == "eta":
                bound[k] = 4 * max(v, 2 * gamma(n + 1))
            elif k in ("solve_f", "solve_b"):
                bound[k] = 4 * max(v, 2 * gamma(n))
            else:
                bound[k] = min(8 * max(v, fl.get(k, 0.0)), cp.get(k, np.inf))
    return dict(r_eff=r_eff, x=x, tg=tg, R=R, routes=per_route, bound=bound, max_rho=max_rho, admitted=admitted, n=n, N=N, rank0=rank0)


def reference(fam, mode, n, m=0, rank0=0):
    """build_reference of a family's case, computed once and never modified (mode 0: without the factor)"""
    key = (fam, mode, n, m, rank0)
    if key not in _REFS:
        d, r_eff = case_column(fam, n, n + m)
        ref = build_reference(r_eff, rhs_x(n), n, m, rank0, mode >= 1)
        ref["fam"] = d
        _REFS[key] = ref
    return _REFS[key]


def unpack_columns(packed, n):
    """the packed columns of L (column k at k n - k (k - 1) / 2 - k + j, rows j = k .. n-1) as a dense lower triangle, and whether
    the entries after the triangle's end still hold the sentinel"""
    L = np.zeros((n, n))
    for k in range(n):
        off = k * n - k * (k - 1) // 2 - k
        L[k:, k] = packed[off + k:off + n]
    return L, bool((packed[n * (n + 1) // 2:] == SENTINEL).all())
