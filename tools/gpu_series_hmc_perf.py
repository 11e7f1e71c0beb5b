"""Many short series, HMC rejuvenation: the fused entry (agp_hmc_series_batch: the whole chain of a (series, particle) pair in one
workgroup, one call) against the two routes a caller had before it, on the same inputs, in the same process —
  host route   1 + L calls of agp_logpdf_grad_series_batch per move, the transforms, momenta and accept step in NumPy on the host,
               every particle riding along on every leapfrog step (programs encoded once; only the parameter array changes);
  series loop  the same chain with a loop over the series of agp_set_data + agp_logpdf_grad_batch as its evaluation.
    python tools/gpu_series_hmc_perf.py [--reps R] [--loop-reps Q] [--out profiles/series_hmc_perf.txt]
One line per shape (S series x n points x particles per series) and n_hmc (1, 10) at the reference's defaults L = 10, eps = 0.02,
n_exit = 0 (no early exit: every route makes the same 2 n_hmc (1 + L) + 2 evaluations): median [min, max] ms over R alternating
repeats (10 R for the single series; the series loop over Q repeats, and over ONE at n_hmc = 10: it takes seconds); the fused call's
kernel time (HIP events of one profiled call) in all and per evaluation, beside the gradient entry's kernel time on the same particles —
the difference is the loop's own overhead; and the fused call with the noise moves' shortcut (d / d noise from |L^-T|_F^2, no reverse
pass) switched off.  The host routes draw their own normals: the routes' chains differ, their work does not.  Nothing is asserted."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402

L, EPS = 10, 0.02


def spread(t):
    t = np.asarray(t)
    return f"{np.median(t):9.3f} [{t.min():.3f}, {t.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = g.load_package()
    pr = pkg.prior
    eng = pkg.GPEngine(0)
    tf = pr.hmc_transform_table()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say("    S     n  P/S n_hmc | fused ms median [min, max] (kernels ms, per evaluation us; gradient entry's kernels us) | shortcut off ms (kernels ms) | "
        "host route ms | host / fused | series loop ms | loop / fused")
    for S, n, pps in ((64, 144, 8), (256, 126, 2), (1, 144, 8)):
        series, nodes, noises = [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            series.append(pr.synthetic_series(n, seed=1000 + s, shuffle=True))
            nd, nz = pr.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises += list(nz)
        P = len(nodes)
        op_off, ops, prm_off, prm0 = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)
        cls = np.concatenate([pr.hmc_classes(nd) for nd in nodes])
        z0 = np.array([pr.hmc_untransform(v, c, tf) for v, c in zip(prm0, cls)])
        zn0 = np.array([pr.hmc_untransform(v - pr.JITTER, 0, tf) for v in noises])
        split = lambda a: [a[prm_off[i]:prm_off[i + 1]] for i in range(P)]
        seeds = np.arange(1, P + 1, dtype=np.uint64)
        mu, sg, sc = (np.where(cls >= 0, tf[np.maximum(cls, 0), k], 0.0) for k in range(3))
        owner = np.repeat(np.arange(P), np.diff(prm_off))
        per_series = [(np.flatnonzero(sidx == s), ) for s in range(S)]

        def theta(z):
            x = mu + sg * z
            with np.errstate(over="ignore"):
                return np.where(cls < 0, z, np.where(sc == 0.0, np.exp(x), sc / (1.0 + np.exp(-x))))

        def eval_batched(z, zn):
            th = theta(z); nz = np.exp(-1.5 + zn) + pr.JITTER
            lp, gr, gn, info = eng.logpdf_grad_series_batch(series, None, nz, sidx, check=False, programs=(op_off, ops, prm_off, th))
            return lp, np.concatenate(gr), gn, th, nz

        def eval_loop(z, zn):
            th = theta(z); nz = np.exp(-1.5 + zn) + pr.JITTER
            lp = np.empty(P); gn = np.empty(P); gr = np.empty(prm0.size)
            for s in range(S):
                sel = per_series[s][0]
                a, b = prm_off[sel[0]], prm_off[sel[-1] + 1]
                eng.set_data(*series[s])
                r = eng.logpdf_grad_batch(None, nz[sel], check=False,
                                          programs=(op_off[sel[0]:sel[-1] + 2] - op_off[sel[0]], ops[op_off[sel[0]]:op_off[sel[-1] + 1]],
                                                    prm_off[sel[0]:sel[-1] + 2] - a, th[a:b]))
                lp[sel] = r[0]; gr[a:b] = np.concatenate(r[1]); gn[sel] = r[2]
            return lp, gr, gn, th, nz

        def host_chain(evaluate, n_hmc):
            """every particle's chain side by side: Gen.hmc on the parameters, then on the noise, n_hmc times"""
            hr = np.random.default_rng(1)
            z, zn = z0.copy(), zn0.copy()
            mov = cls >= 0
            for _ in range(n_hmc):
                for noise_move in (False, True):
                    def U_and_grad():
                        lp, gr, gn, th, nz = evaluate(z, zn)
                        if noise_move:
                            return lp - 0.5 * zn * zn, gn * (nz - pr.JITTER) - zn
                        d = np.where(sc == 0.0, sg * th, sg * th * (1.0 - th / np.where(sc == 0.0, 1.0, sc)))
                        return lp - 0.5 * np.bincount(owner, np.where(mov, z * z, 0.0), P), np.where(mov, gr * d - z, 0.0)
                    U0, gz = U_and_grad()
                    m = hr.standard_normal(P if noise_move else z.size)
                    K0 = -0.5 * (m * m if noise_move else np.bincount(owner, np.where(mov, m * m, 0.0), P))
                    saved = (zn if noise_move else z).copy()
                    for _ in range(L):
                        m = m + 0.5 * EPS * gz
                        if noise_move:
                            zn = zn + EPS * m
                        else:
                            z = z + EPS * np.where(mov, m, 0.0)
                        U1, gz = U_and_grad()
                        m = m + 0.5 * EPS * gz
                    K1 = -0.5 * (m * m if noise_move else np.bincount(owner, np.where(mov, m * m, 0.0), P))
                    with np.errstate(invalid="ignore"):
                        acc = np.log(hr.random(P)) < (U1 - U0) + (K1 - K0)
                    if noise_move:
                        zn = np.where(acc, zn, saved)
                    else:
                        z = np.where(acc[owner], z, saved)
            return evaluate(z, zn)[0]

        eng.set_profiling(True)
        eng.logpdf_grad_series_batch(series, None, np.array(noises), sidx, check=False, programs=(op_off, ops, prm_off, prm0))
        grad_k = eng.timing()["total_ms"]
        eng.set_profiling(False)
        for n_hmc in (1, 10):
            def fused(flags=0):
                return eng.hmc_series_batch(series, None, split(z0), zn0, split(cls), tf, sidx, n_hmc, seeds, L_param=L, eps_param=EPS, L_noise=L,
                                            eps_noise=EPS, n_exit=0, flags=flags, check=False, programs=(op_off, ops, prm_off, prm0))
            evals = 2 * n_hmc * (1 + L) + 2
            r = fused(); fused(1); host_chain(eval_batched, 1)
            reps = args.reps if S > 1 else 10 * args.reps
            t_f, t_o, t_h = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter(); fused(); t_f.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter(); fused(1); t_o.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter(); host_chain(eval_batched, n_hmc); t_h.append(1e3 * (time.perf_counter() - t0))
            t_l = []
            for _ in range(args.loop_reps if n_hmc == 1 else 1):
                t0 = time.perf_counter(); host_chain(eval_loop, n_hmc); t_l.append(1e3 * (time.perf_counter() - t0))
            eng.set_profiling(True)
            fused(); k_on = eng.timing()["total_ms"]
            fused(1); k_off = eng.timing()["total_ms"]
            eng.set_profiling(False)
            say(f"{S:5d} {n:5d} {pps:4d} {n_hmc:5d} | {spread(t_f)} ({k_on:8.3f}, {1e3 * k_on / evals:7.1f}; {1e3 * grad_k:7.1f}) | {spread(t_o)} ({k_off:8.3f}) | "
                f"{spread(t_h)} | {np.median(t_h) / np.median(t_f):6.2f} | {spread(t_l)} | {np.median(t_l) / np.median(t_f):7.1f}"
                f"   [accepted {int(r.counts[:, 0].sum())}/{int(r.counts[:, 1].sum())} parameter, {int(r.counts[:, 2].sum())} noise moves, "
                f"{int(r.counts[:, 3].sum())} not PD, {int((r.info != 0).sum())} particles not factored]")
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
