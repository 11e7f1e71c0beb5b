"""Mixture predictive quantiles (predict_quantile): the device entry (agp_predict_quantile_batch: marginal pass, host staging of the
m x P components, k_mixture_pack + k_mixture_quantile) against the host route (agp_predict_batch marginal + the numpy restatement
(b) of tests/_mixture_quantile_ref.py) on the same inputs, q = (0.025, 0.5, 0.975).
    python tools/gpu_predict_quantile_perf.py [--reps R] [--one]
Per shape: median ms of the device entry, of its marginal pass alone (agp_predict_batch), of the search alone on the staged
components (agp_mixture_quantile: upload + pack + search + download), of the host route (its numpy search timed on a seeded sample
of 256 points and scaled to m — the points are independent), the iterations per (point, q) (median / max), and how many sampled
points the device and (b) agree on bitwise.  --one: only n = 2048, m = 4096, P = 128, tol = 1e-6 (for a rocprofv3 run)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g      # noqa: E402
import _mixture_quantile_ref as R      # noqa: E402

QS = (0.025, 0.5, 0.975)


def timed(fn, reps):
    r = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); ts.append(1e3 * (time.perf_counter() - t0))
    return r, float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one", action="store_true")
    a = ap.parse_args()
    pkg = g.load_package()
    n = 2048
    ts, xs = pkg.prior.synthetic_series(n + 4096, seed=8)
    eng = pkg.GPEngine(0)
    eng.set_data(ts[:n], xs[:n])
    yt = (0.8, 0.1)
    shapes = [(4096, 128, 1e-6)] if a.one else [(m, P, tol) for m in (512, 4096) for P in (8, 128, 512) for tol in (1e-5, 1e-6)]
    print(f"{'n':>5} {'m':>5} {'P':>4} {'tol':>6} {'entry_ms':>9} {'marginal_ms':>11} {'search_ms':>9} {'host_ms':>9} "
          f"{'speedup':>8} {'it_med':>6} {'it_max':>6} {'bitwise':>8}", flush=True)
    for m, P, tol in shapes:
        rng = np.random.default_rng(P + m)
        nodes, noises = pkg.prior.sample_particles(rng, P, max_depth=4)
        tp = ts[n:n + m]
        _, _, _, info = eng.predict_batch(nodes, noises, tp, check=False)
        ok = [p for p in range(P) if info[p] == 0]
        while len(ok) < P:          # (keep P particles that all have a predictive)
            nn, nz = pkg.prior.sample_particles(rng, P - len(ok), max_depth=4)
            nodes += nn; noises = np.concatenate([noises, nz])
            _, _, _, info = eng.predict_batch(nodes, noises, tp, check=False)
            ok = [p for p in range(len(nodes)) if info[p] == 0][:P]
        nodes = [nodes[p] for p in ok]; noises = noises[ok]
        w = np.exp(pkg.dist.normalize_weights(rng.standard_normal(P))[1])
        (x, conv, iters, _), t_entry = timed(lambda: eng.predict_quantile_batch(nodes, noises, tp, w, QS, y_transform=yt, tol=tol),
                                             a.reps)
        (mean, var, _, info), t_marg = timed(lambda: eng.predict_batch(nodes, noises, tp, check=False), a.reps)
        mr, vr, _ = pkg.raw_components(mean, var, info, n, yt)
        _, t_search = timed(lambda: eng.mixture_quantile(mr, vr, w, QS, tol=tol), a.reps)
        pts = np.sort(np.random.default_rng(1).choice(m, min(256, m), replace=False))
        t0 = time.perf_counter()
        same = 0
        for k, q in enumerate(QS):
            b = R.quantile_search(mr, vr, w, q, tol=tol, points=pts)
            same += int((R.same_bits(b["x"], x[pts, k]) & (b["iters"] == iters[pts, k])).sum())
        t_b = 1e3 * (time.perf_counter() - t0) * m / len(pts)
        t_host = t_marg + t_b
        print(f"{n:5d} {m:5d} {P:4d} {tol:6.0e} {t_entry:9.2f} {t_marg:11.2f} {t_search:9.2f} {t_host:9.1f} {t_host / t_entry:8.1f} "
              f"{int(np.median(iters)):6d} {int(iters.max()):6d} {same:4d}/{3 * len(pts):<4d}", flush=True)
        assert conv.all()
    eng.close()


if __name__ == "__main__":
    main()
