"""Predictive log-density of held-out values: the device entry (agp_predict_logpdf_batch: one joint factorisation per particle) against
the host route (agp_predict_batch with the m x m covariances copied out, then one numpy Cholesky per particle) on the same inputs.
    python tools/gpu_predict_logpdf_perf.py [--reps R] [--quick]
Prints one line per shape: median / min / max ms of both routes over R timed repeats after a warm-up, the largest disagreement
relative to max(1, |logp|), and the device entry's share of the fp64 MFMA peak measured on this device (agp_debug_mfma_peak) for
(n + m)^3 / 3 flops per particle."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.linalg as sla

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402


def host_route(eng, nodes, noises, tp, y, n):
    mean, _, cov, info = eng.predict_batch(nodes, noises, tp, n=n, want_cov=True, check=False)
    out = np.full(len(nodes), np.nan)
    for p in range(len(nodes)):
        if info[p]:
            continue
        L = np.linalg.cholesky(cov[p])
        a = sla.solve_triangular(L, y - mean[p], lower=True, check_finite=False)
        out[p] = -0.5 * (len(y) * np.log(2 * np.pi) + 2 * np.log(np.diag(L)).sum() + a @ a)
    return out


def timed(fn, reps, sync):
    fn(); sync()
    ts = []
    for _ in range(reps):
        sync(); t0 = time.perf_counter(); r = fn(); sync(); ts.append(1e3 * (time.perf_counter() - t0))
    return r, np.array(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="n = 2048 shapes with P = 8 only, and the tutorial size")
    ap.add_argument("--profile-case", action="store_true",
                    help="the device entry alone at n = m = 2048, P = 128 (for a kernel / memory-copy trace)")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)
    eng = pkg.GPEngine(0)
    peak, _ = eng.debug_mfma_peak()
    print(f"fp64 MFMA peak measured: {peak:.1f} TF/s", flush=True)
    rng = np.random.default_rng(0)
    shapes = [(2048, m, P, grid) for m in (18, 512, 2048) for P in (8, 128) for grid in ("regular", "shuffled")]
    if args.quick:
        shapes = [s for s in shapes if s[2] == 8]
    shapes.append((126, 18, 8, "regular"))        # the overview tutorial's size
    if args.profile_case:
        shapes = [(2048, 2048, 128, "regular")]
    rows = []
    for n, m, P, grid in shapes:
        ts, xs = pkg.prior.synthetic_series(n + m, seed=n + m, shuffle=False)
        tr, tp = ts[:n], ts[n:]
        xtr, y = xs[:n], xs[n:]
        if grid == "shuffled":
            perm = rng.permutation(n); tr, xtr = tr[perm], xtr[perm]
            qp = rng.permutation(m); tp, y = tp[qp], y[qp]
        eng.set_data(tr, xtr)
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(P + m), P, max_depth=4)
        (lp, info), t_dev = timed(lambda: eng.predict_logpdf_batch(nodes, noises, tp, y, check=False), args.reps, sync)
        if args.profile_case:
            print(f"n={n} m={m} P={P}: device {np.median(t_dev):.2f} ms, {int((info == 0).sum())}/{P} ok", flush=True)
            continue
        host_reps = max(1, min(args.reps, 2 if m * m * P > 2048 * 2048 * 8 else args.reps))
        lh, t_host = timed(lambda: host_route(eng, nodes, noises, tp, y, n), host_reps, sync)
        ok = (info == 0) & np.isfinite(lh)
        err = float(np.max(np.abs(lp[ok] - lh[ok]) / np.maximum(1.0, np.abs(lh[ok])))) if ok.any() else float("nan")
        flops = P * (n + m) ** 3 / 3.0
        share = flops / (np.median(t_dev) * 1e-3) / (peak * 1e12)
        row = dict(n=n, m=m, P=P, grid=grid, dev_ms=[float(np.median(t_dev)), float(t_dev.min()), float(t_dev.max())],
                   host_ms=[float(np.median(t_host)), float(t_host.min()), float(t_host.max())], max_rel_diff=err,
                   ok=int(ok.sum()), mfma_share=float(share))
        rows.append(row)
        print(f"n={n:5d} m={m:5d} P={P:4d} {grid:8s}  device {row['dev_ms'][0]:9.2f} ms [{row['dev_ms'][1]:.2f}..{row['dev_ms'][2]:.2f}]"
              f"  host route {row['host_ms'][0]:10.2f} ms [{row['host_ms'][1]:.2f}..{row['host_ms'][2]:.2f}]"
              f"  x{row['host_ms'][0] / row['dev_ms'][0]:7.1f}  max rel diff {err:.1e} ({row['ok']}/{P})  {100 * share:5.1f} % of fp64 peak",
              flush=True)
    eng.close()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps({"peak_tflops": peak, "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
