"""Forecast bands of many short series: the fused entry (agp_predict_quantile_series_batch: the predictive launches of
agp_predict_series_batch, then the ragged pack / search / moments kernels on the same stream, one synchronisation, only the band comes
back) against the route the entries before it offered on the same inputs — predict_series_batch, raw_components on the host, then a
loop over the series of mixture_quantile and mixture_moments.
    python tools/gpu_series_quantile_perf.py [--reps R] [--out profiles/series_quantile_perf.txt]
Prints one line per shape (S series x n points x particles per series, m query times per series, q = 0.025, 0.5, 0.975): median [min,
max] ms of both routes (host clock around calls that end synchronised; programs encoded beforehand for both) over R timed repeats
(10 R for the single series) after a warm-up of each, the routes alternating within every repeat; the ratio of the medians; the fused
call's kernel times (HIP events of profiled calls: agp_get_timing slot 0, the predictive launches, and slot 4, the three read-out
kernels together); the two-step route's predictive call alone; and whether the two routes agree bit for bit."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402

QS = np.array([0.025, 0.5, 0.975])


def spread(t):
    return f"{np.median(t):8.3f} [{t.min():.3f}, {t.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    say("    S     n  P/S     P    m | fused ms median [min, max]  (kernels ms: predictive; read-out) | predict_series_batch + loop of "
        "mixture_quantile + mixture_moments ms median [min, max]  (of which predict_series_batch) | two-step / fused | bitwise equal")
    for S, n, pps, m in ((64, 144, 8, 36), (256, 126, 2, 12), (1, 144, 8, 36)):
        series, queries, nodes, noises = [], [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            ts, xs = pkg.prior.synthetic_series(n, seed=1000 + s, shuffle=True)
            series.append((ts, xs))
            queries.append(ts.max() + (ts.max() - ts.min()) * np.arange(1, m + 1) / (4.0 * m))
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(nz)
        noises = np.concatenate(noises)
        progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)
        _, w = pkg.pack_series_mixture(sidx, S, log_weights=rng.standard_normal(S * pps))
        yt = np.stack([0.5 + rng.random(S), rng.standard_normal(S)], axis=1)

        def fused():
            return eng.predict_quantile_series_batch(series, queries, None, noises, sidx, w, QS, y_transforms=yt, want_moments=True,
                                                     check=False, programs=progs)

        def predictive():
            return eng.predict_series_batch(series, queries, None, noises, sidx, check=False, programs=progs)

        def two_step():
            means, vars_, info = predictive()
            xs_, ms_, vs_ = [], [], []
            for s in range(S):
                sel = slice(s * pps, (s + 1) * pps)
                mr, vr, inf = pkg.raw_components(np.stack(means[sel]), np.stack(vars_[sel]), info[sel], n, tuple(yt[s]))
                if (inf != 0).any():
                    xs_.append(None); ms_.append(None); vs_.append(None)
                    continue
                xs_.append(eng.mixture_quantile(mr, vr, w[sel], QS)[0])
                mu, var, _ = eng.mixture_moments(mr, w[sel], vars=vr, space=0)
                ms_.append(mu); vs_.append(var)
            return xs_, ms_, vs_
        a, b = fused(), two_step()
        same, skipped = True, 0
        for s in range(S):
            if b[0][s] is None:
                skipped += 1
                same = same and bool(np.isnan(a.x[s]).all())
                continue
            same = same and all(np.array_equal(u.view(np.int64), np.ascontiguousarray(v).view(np.int64))
                                for u, v in ((a.x[s], b[0][s]), (a.mean[s], b[1][s]), (a.var[s], b[2][s])))
        reps = args.reps if S > 1 else 10 * args.reps
        tf, tl, tp = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter(); fused(); tf.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); two_step(); tl.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); predictive(); tp.append(1e3 * (time.perf_counter() - t0))
        tf, tl, tp = np.array(tf), np.array(tl), np.array(tp)
        eng.set_profiling(True)
        kp, kr = [], []
        for _ in range(5):
            fused()
            t = eng.timing()
            kp.append(t["total_ms"]); kr.append(t["finish_ms"])
        eng.set_profiling(False)
        say(f"{S:5d} {n:5d} {pps:4d} {S * pps:5d} {m:4d} | {spread(tf)}  ({np.median(kp):7.3f}; {np.median(kr):7.3f}) | {spread(tl)}  "
            f"({np.median(tp):7.3f}) | {np.median(tl) / np.median(tf):8.1f} | {same} ({skipped} series without a predictive)")
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
