"""Mixture moments of predict_mvn: the device entry (agp_predict_mixture_batch with covariance: the predictive pass with every chunk's
covariances added into m x m running sums on the device) against the route the entries before it offered (agp_predict_batch with the
P m x m covariances copied out, then a numpy reduction) on the same inputs.
    python tools/gpu_predict_mixture_perf.py [--reps R] [--quick] [--out profiles/predict_mixture_perf.txt]
Prints one line per shape: median [min, max] ms of both routes (host clock around calls that end synchronised) over R timed repeats
after a warm-up of each, the two routes alternating within every repeat; the device entry split into the predictive
pass and the accumulation kernels (HIP events of one profiled call, agp_get_timing slots 14 / 15); the doubles each route brings back
to the host; and the largest disagreement between the routes relative to max(1, |cov|max).  Also the measured errors of the device
exp / expm1 the log-normal components call (ulps against mpmath)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g      # noqa: E402


def alternate(fa, fb, reps):
    """Warm both up, then time them turn by turn: (result a, result b, ms of a, ms of b)."""
    ra, rb = fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fa(); ta.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter(); fb(); tb.append(1e3 * (time.perf_counter() - t0))
    return ra, rb, np.array(ta), np.array(tb)


def spread(t):
    return f"{np.median(t):9.2f} [{t.min():.2f}, {t.max():.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed repeats at the large shape (tutorial shape: 8 times as many)")
    ap.add_argument("--quick", action="store_true", help="the tutorial shape only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    import mpmath as mp
    import _mixture_moments_ref as R
    rng = np.random.default_rng(0)
    arg = np.concatenate([rng.uniform(-3.0, 6.0, 3000), rng.uniform(-60.0, 120.0, 1000), rng.uniform(700.0, 709.78, 500)])
    c = np.concatenate([rng.uniform(-0.6, 0.6, 3000), 10.0 ** rng.uniform(-12, -1, 500), rng.uniform(-40.0, 60.0, 1000)])
    say(f"device exp_f error {R.ulp_err(eng.debug_math(0, arg), arg, mp.exp):.3f} ulp (pinned EXP_ULP_DEV = {R.EXP_ULP_DEV}), "
        f"device expm1 error {R.ulp_err(eng.debug_math(9, c), c, mp.expm1):.3f} ulp (pinned EXPM1_ULP_DEV = {R.EXPM1_ULP_DEV})")
    say("    n     m    P | device ms median [min, max]  (pass  accumulate) | D2H doubles | host route ms median [min, max]  D2H doubles | "
        "speed-up | max rel diff (mean, cov)")
    shapes = [(144, 200, 18)] + ([] if args.quick else [(2048, 1024, 128)])
    for n, m, P in shapes:
        ts, xs = pkg.prior.synthetic_series(n + m, seed=n + m, shuffle=False)
        eng.set_data(ts[:n], xs[:n])
        tp = ts[n:]
        nodes, noises = pkg.prior.sample_particles(np.random.default_rng(P + m), P, max_depth=4)
        w = np.random.default_rng(P).random(P); w /= w.sum()
        yt = (2.0, 0.25)

        def device():
            return eng.predict_mixture_batch(nodes, noises, tp, w, y_transform=yt, want_cov=True, check=False)

        def host():
            mu, _, cv, _ = eng.predict_batch(nodes, noises, tp, n=n, want_cov=True, check=False)
            mr = (mu - yt[1]) / yt[0]
            mbar = w @ mr
            d = mr - mbar
            out = np.einsum("p,pij->ij", w, cv) / (yt[0] * yt[0])
            out += (d * w[:, None]).T @ d
            return mbar, out
        (mean, var, cov, info), (mh, ch), t_dev, t_host = alternate(device, host, args.reps * (1 if m * m * P > 512 * 512 * 64 else 8))
        eng.set_profiling(True)      # (one profiled call of its own: the events serialise the pass)
        device()
        tm = eng.timing()
        eng.set_profiling(False)
        ok = (info == 0).all()
        e_m = float(np.abs(mean - mh).max() / max(1.0, np.abs(mh).max())) if ok else float("nan")
        e_c = float(np.abs(cov - ch).max() / max(1.0, np.abs(ch).max())) if ok else float("nan")
        say(f"{n:5d} {m:5d} {P:4d} | {spread(t_dev)}  ({tm['mixture_pass_ms']:6.2f}  {tm['mixture_accumulate_ms']:8.3f}) | "
            f"{m * m + 2 * m:11d} | {spread(t_host)}  {P * m * m + 2 * P * m:11d} | {np.median(t_host) / np.median(t_dev):8.1f} | "
            f"{e_m:.1e}, {e_c:.1e}")
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
