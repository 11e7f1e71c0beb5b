"""TEST INFRASTRUCTURE: a NumPy / fp64 restatement of agp_hmc_series_batch's chain (include/autogp_hip.h) on the oracle's value and
gradient — the reference's rejuvenate_particle_parameters (src/inference_smc_anneal_data.jl:33-76) with Gen.hmc taken literally, in the
latent space of src/Model.jl:24-49, with the entry's own Philox counters (tests/_pred_sample_ref.py).  The same code runs on mpmath
numbers (ops=MP, evalfn=eval_mp): that replay of the same draws is what makes this reference trustworthy
(tests/test_series_hmc_cpu.py).  Also the Python twin of the HMC kernel's LDS map."""
import math

import numpy as np
from scipy.special import ndtri

import _pred_sample_ref as PR
import _series_cases as S
import _series_grad_ref as GR
from oracle import oracle as O

TAG = 0x484D43
U_BLOCK = 1 << 32
HMC_ST_N = 32


class F64:
    """the arithmetic of the chain: Python floats"""
    num = staticmethod(float)
    exp = staticmethod(lambda x: math.exp(x) if x < 709.0 else math.inf)
    log = staticmethod(math.log)
    isfinite = staticmethod(lambda x: math.isfinite(x))


def momentum(seed, it, mv, k):
    return float(ndtri(PR.uniform(PR.philox_block(seed, k // 4, it, mv, TAG)[k % 4])))


def log_u(seed, it, mv):
    return math.log(PR.uniform(PR.philox_block(seed, U_BLOCK, it, mv, TAG)[0]))


def transform(z, c, tf, ops=F64):
    if c < 0:
        return z
    mu, sigma, scale = (ops.num(v) for v in tf[c])
    x = mu + sigma * z
    return ops.exp(x) if scale == 0 else scale / (1 + ops.exp(-x))


def dtheta(th, c, tf, ops=F64):
    mu, sigma, scale = (ops.num(v) for v in tf[c])
    return sigma * th if scale == 0 else sigma * th * (1 - th / scale)


def tree_with(tree, params):
    """the oracle's tuple tree with the numeric parameters replaced, in program order (left, right, node)"""
    it = iter(params)

    def rec(t):
        tag = t[0]
        if tag in ("+", "*"):
            a = rec(t[1]); b = rec(t[2])
            return (tag, a, b)
        if tag == "CP":
            a = rec(t[1]); b = rec(t[2])
            return ("CP", a, b, next(it), next(it))
        return (tag,) + tuple(next(it) for _ in t[1:])
    out = rec(tree)
    assert next(it, None) is None
    return out


def eval_oracle(ts, xs):
    """(tree, noise) -> (logpdf, grad, grad_noise, info) by the fp64 oracle; info = the first bad minor"""
    def f(tree, noise):
        try:
            lp, g, gn = O.gp_logpdf_grad(tree, noise, ts, xs)
        except np.linalg.LinAlgError:
            return math.nan, None, math.nan, max(1, S.first_bad_minor(O.compute_cov_matrix_vectorized(tree, noise, ts)) or 1)
        except (ValueError, ZeroDivisionError, OverflowError, FloatingPointError):      # (a covariance that is not finite: no factor)
            return math.nan, None, math.nan, 1
        return lp, [float(v) for v in g], gn, 0
    return f


def hmc_chain(tree, z, z_noise, cls, tf, seed, n_hmc, evalfn, L_param=10, eps_param=0.02, L_noise=10, eps_noise=0.02, n_exit=None,
              noise_class=0, jitter=1e-5, ops=F64):
    """One particle's chain.  Returns dict(z, z_noise, prm, noise, logpdf, counts[4], info, trace[n_hmc][2][2], evals)."""
    num = ops.num
    z = [num(v) for v in z]; zn = num(z_noise)
    cls = [int(c) for c in cls]
    sel = [i for i, c in enumerate(cls) if c >= 0]
    n_exit = n_hmc if n_exit is None else n_exit
    nan = math.nan
    trace = [[[nan, nan], [nan, nan]] for _ in range(n_hmc)]
    counts = [0, 0, 0, 0]
    evals = [0]

    def state():
        th = [transform(v, c, tf, ops) for v, c in zip(z, cls)]
        return th, transform(zn, noise_class, tf, ops) + num(jitter)

    def evaluate(noise_move):
        """(ok, U, gradient in z of the move's selection, logpdf, info)"""
        th, nz = state()
        evals[0] += 1
        if not (all(ops.isfinite(v) for v in th) and ops.isfinite(nz)):
            return False, nan, None, nan, 0
        lp, g, gn, info = evalfn(tree_with(tree, th), nz)
        if info != 0 or not ops.isfinite(lp):
            return False, nan, None, lp, info
        if noise_move:
            gz = [gn * dtheta(nz - num(jitter), noise_class, tf, ops) - zn]
            zz = zn * zn
        else:
            gz = [g[i] * dtheta(th[i], cls[i], tf, ops) - z[i] for i in sel]
            zz = sum((z[i] * z[i] for i in sel), num(0))
        if not all(ops.isfinite(v) for v in gz):
            return False, nan, None, lp, 0
        return True, lp - zz / 2, gz, lp, 0

    th0, nz0 = state()
    lp0, _, _, info0 = evalfn(tree_with(tree, th0), nz0) if all(ops.isfinite(v) for v in th0) else (nan, None, nan, 1)
    evals[0] += 1
    out = dict(z=z, z_noise=zn, prm=th0, noise=nz0, logpdf=lp0, counts=counts, info=info0, trace=trace, evals=evals)
    if info0 != 0:
        out["logpdf"] = nan
        return out
    nrej, stop, moved = 0, False, False
    for it in range(n_hmc):
        if stop:
            break
        pmade = pacc = False
        for mv in (0, 1):
            if (mv == 0 and not sel) or (mv == 1 and L_noise == 0):
                continue
            L, eps = (L_param, num(eps_param)) if mv == 0 else (L_noise, num(eps_noise))
            moved = True
            lu = log_u(seed, it, mv)
            ok, U0, g, _, _ = evaluate(mv == 1)
            alpha, accept = -math.inf, False
            if ok:
                k = len(sel) if mv == 0 else 1
                m = [num(momentum(seed, it, mv, j)) for j in range(k)]
                K0 = -sum((v * v for v in m), num(0)) / 2
                saved = (list(z), zn)
                U = U0
                for step in range(L):
                    m = [a + (eps / 2) * b for a, b in zip(m, g)]
                    if mv == 0:
                        for j, i in enumerate(sel):
                            z[i] = z[i] + eps * m[j]
                    else:
                        zn = zn + eps * m[0]
                    ok, U, g, _, _ = evaluate(mv == 1)
                    if not ok:
                        break
                    m = [a + (eps / 2) * b for a, b in zip(m, g)]
                if ok:
                    K1 = -sum((v * v for v in m), num(0)) / 2
                    alpha = (U - U0) + (K1 - K0)
                    accept = lu < alpha
                if not accept:
                    z[:] = saved[0]; zn = saved[1]
            if not ok:
                counts[3] += 1
            trace[it][mv] = [float(alpha), lu]
            if mv == 0:
                counts[1] += 1; counts[0] += int(accept); pmade, pacc = True, accept
            else:
                counts[2] += int(accept)
        if pmade:
            nrej = 0 if pacc else nrej + 1
            if n_exit > 0 and nrej >= n_exit:
                stop = True
    th, nz = state()
    if moved:
        lp, _, _, info = evalfn(tree_with(tree, th), nz)
        evals[0] += 1
    else:
        lp, info = lp0, 0
    out.update(z=z, z_noise=zn, prm=th, noise=nz, logpdf=lp, info=info)
    return out


# ---- the 60-digit replay ----
def mp_backend():
    import mpmath as mp
    from oracle import oracle_mp as OM

    class MP:
        num = staticmethod(lambda x: x if isinstance(x, mp.mpf) else mp.mpf(float(x)))
        exp = staticmethod(mp.exp)
        log = staticmethod(mp.log)
        isfinite = staticmethod(lambda x: mp.isfinite(x))

    def eval_mp(ts, xs):
        def f(tree, noise):
            def val(params, nz):
                return OM.gp_logpdf_mp(tree_with(tree, params), nz, ts, xs)
            prm = [mp.mpf(v) for v in _params(tree)]
            try:
                lp = val(prm, noise)
            except (ValueError, ZeroDivisionError):
                return math.nan, None, math.nan, 1
            g = []
            for i in range(len(prm) + 1):      # central differences at 60 digits: error ~ h^2
                full = prm + [noise]
                h = mp.mpf(10) ** -20 * max(1, abs(full[i]))
                up = list(full); dn = list(full)
                up[i] += h; dn[i] -= h
                g.append((val(up[:-1], up[-1]) - val(dn[:-1], dn[-1])) / (2 * h))
            return lp, g[:-1], g[-1], 0
        return f
    return MP, eval_mp


def _params(tree):
    tag = tree[0]
    if tag in ("+", "*"):
        return _params(tree[1]) + _params(tree[2])
    if tag == "CP":
        return _params(tree[1]) + _params(tree[2]) + [tree[3], tree[4]]
    return list(tree[1:])


# ---- the LDS map ----
def series_hmc_lds_total(n, n_ops, n_prm, n_cp, g_n_ops, g_n_prm, C):
    """series_hmc_lds(...).total of csrc/agp_args.hpp, in doubles"""
    npc = (g_n_prm + 1) & ~1
    return GR.series_grad_lds_total(n, n_ops, n_prm, n_cp, g_n_ops, g_n_prm) + 6 * npc + ((3 * C + 1) & ~1) + HMC_ST_N


def cp_chain_fits_hmc(k, n, C=3):
    """tests' cp_chain(G, k) under the HMC kernel's map (see _series_grad_ref.cp_chain_fits)"""
    n_ops, n_prm = 2 * k + 1, 3 * k + 1
    return 8 * series_hmc_lds_total(n, n_ops, n_prm, k, n_ops, n_prm, C) <= GR.LDS_BYTES
