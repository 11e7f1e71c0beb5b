"""Posterior predictive samples: the device entry (agp_predict_sample_batch: the joint factorisation of predict_logpdf, then the MFMA
read-out x = mu2 + [L21 L22] [a; z]) against the host route (agp_predict_batch with the m x m covariances copied out, then one numpy
Cholesky and L @ Z per particle) on the same inputs.
    python tools/gpu_predict_sample_perf.py [--reps R] [--quick] [--out profiles/predict_sample_perf.txt]
Prints one line per shape: median ms of both routes over R timed repeats after a warm-up; the device entry split into the factor pass
and the read-out (HIP events of the profiled call: normals + read-out kernels; factor = total - both); the read-out's fp64 TF/s for
2 S m (n + m / 2) flops; and the largest disagreement between the routes given the same components and normals, relative to
|mu| + |L||z| per row."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return r, np.array(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="P = 8 shapes only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    peak, _ = eng.debug_mfma_peak()
    say(f"fp64 MFMA peak measured: {peak:.1f} TF/s")
    say("    n     m    P      S | device ms  (factor  read-out  normals) | read-out TF/s | host route ms | speed-up | max rel diff")
    n = 2048
    shapes = [(m, P, 1024) for m in (18, 512, 2048) for P in (8, 128)] + [(2048, 8, 16384)]
    if args.quick:
        shapes = [s for s in shapes if s[1] == 8]
    for m, P, S in shapes:
        ts, xs = pkg.prior.synthetic_series(n + m, seed=n + m, shuffle=False)
        eng.set_data(ts[:n], xs[:n])
        tp = ts[n:]
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(P + m), P, max_depth=4)
        npred = 0.05 + noises        # (every particle's predictive positive definite)
        w = np.full(P, 1.0 / P)
        (x, comp, info), t_dev = timed(lambda: eng.predict_sample_batch(nodes, noises, tp, w, S, seed=1, noise_pred=npred, check=False),
                                       args.reps)
        eng.set_profiling(True)
        t0 = time.perf_counter()
        eng.predict_sample_batch(nodes, noises, tp, w, S, seed=1, noise_pred=npred, check=False)
        t_prof = 1e3 * (time.perf_counter() - t0)
        tm = eng.timing()
        eng.set_profiling(False)
        t_norm, t_read = tm["sample_normals_ms"], tm["sample_readout_ms"]
        t_fac = t_prof - t_norm - t_read
        flops = 2.0 * S * m * (n + m / 2)
        tf = flops / (t_read * 1e-3) / 1e12 if t_read > 0 else float("nan")
        # the host route on the seeded call's components with normals of numpy's; the device on the same (component, z)
        Z = np.random.default_rng(m + P).standard_normal((m, S))
        xz, _, _ = eng.predict_sample_batch(nodes, noises, tp, w, S, noise_pred=npred, component=comp, z=Z, check=False)
        host_reps = 1 if m * m * P > 512 * 512 * 128 else args.reps

        def host():
            mu, _, cv, _ = eng.predict_batch(nodes, noises, tp, n=n, noise_pred=npred, want_cov=True, check=False)
            out = np.empty((m, S)); scale = np.empty((m, S))
            for p in np.unique(comp):
                L = np.linalg.cholesky(cv[p]); sel = comp == p
                out[:, sel] = mu[p][:, None] + L @ Z[:, sel]
                scale[:, sel] = np.abs(mu[p])[:, None] + np.abs(L) @ np.abs(Z[:, sel])
            return out, scale
        (xh, scale), t_host = timed(host, host_reps)
        err = float(np.max(np.abs(xz - xh) / scale)) if (info == 0).all() else float("nan")
        say(f"{n:5d} {m:5d} {P:4d} {S:6d} | {np.median(t_dev):9.2f}  ({t_fac:6.2f}  {t_read:8.3f}  {t_norm:7.3f}) | {tf:13.2f} | "
            f"{np.median(t_host):13.1f} | {np.median(t_host) / np.median(t_dev):8.1f} | {err:.1e}")
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
