"""Sum-of-GPs decomposition of a population (predict_sum / predict_mvn_sum, src/api.jl:898-1034): the four routes on the same split
kernels (split_kernel_sop(node, Periodic) of P distinct prior particles), time in ms per population:
  loop_cov    a loop of agp_infer_gp_sum over the particles (full covariance each: the only route before the batched entries)
  batch_cov   agp_infer_gp_sum_batch with the covariance
  batch_marg  agp_infer_gp_sum_batch without it (means and marginal variances)
  sum         agp_predict_sum_batch, q = (0.025, 0.5, 0.975): marginal pass + the device read-out (raw transform, quantiles)
and the largest difference of the batch's means to the loop's (relative to max(1, |mean|)).
    python tools/gpu_predict_sum_perf.py [--reps R]
Sizes: the decomposition tutorial's (a 144-point monthly series, n = 115 observed, p = 260 query points, P = 18) and a large one
(n = 1024, p = 1280, P = 64)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402

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
    a = ap.parse_args()
    pkg = g.load_package()
    G = pkg
    eng = pkg.GPEngine(0)
    print(f"{'n':>5} {'p':>5} {'P':>3} {'loop_cov':>9} {'batch_cov':>9} {'batch_marg':>10} {'sum':>8} {'loop/batch_cov':>14} "
          f"{'loop/sum':>8} {'max_rel_diff':>12}", flush=True)
    for n, p, P, seed in ((115, 260, 18, 1), (1024, 1280, 64, 2)):
        ts, xs = pkg.prior.calendar_series(n + p, "M", seed=seed) if n < 200 else pkg.prior.synthetic_series(n + p, seed=seed)
        eng.set_data(ts[:n], xs[:n])
        tp = np.concatenate([ts[:n], ts[n:n + p - n]]) if p > n else ts[:p]
        rng = np.random.default_rng(seed)
        nodes, noises = pkg.prior.sample_particles(rng, P, max_depth=4)
        splits = [list(G.split_kernel_sop(nd, G.Periodic)) for nd in nodes]

        def loop():
            return [eng.infer_gp_sum(s, nz, tp, check=False)[:2] for s, nz in zip(splits, noises)]
        loop_r, t_loop = timed(loop, a.reps)
        (mb, _, _, _, _, _), t_bcov = timed(lambda: eng.infer_gp_sum_batch(splits, noises, tp, want_cov=True, check=False), a.reps)
        _, t_bmarg = timed(lambda: eng.infer_gp_sum_batch(splits, noises, tp, check=False), a.reps)
        _, t_sum = timed(lambda: eng.predict_sum_batch(splits, noises, tp, q=QS, y_transform=(0.8, 0.1), check=False), a.reps)
        ml = np.array([r[0] for r in loop_r])
        fin = np.isfinite(ml).all(axis=1) & np.isfinite(mb).all(axis=1)
        d = float((np.abs(mb[fin] - ml[fin]) / np.maximum(1.0, np.abs(ml[fin]))).max()) if fin.any() else float("nan")
        print(f"{n:5d} {p:5d} {P:3d} {t_loop:9.1f} {t_bcov:9.1f} {t_bmarg:10.1f} {t_sum:8.1f} {t_loop / t_bcov:14.2f} "
              f"{t_loop / t_sum:8.2f} {d:12.1e}", flush=True)
        del loop_r, mb
    eng.close()


if __name__ == "__main__":
    main()
