"""Many short series, value AND gradient: the fused entry (agp_logpdf_grad_series_batch: one workgroup per (series, particle), factor,
L^-T, alpha and the contraction with dK / d theta in LDS, one call) against the only route the entries before it offered — a loop over
the series of agp_set_data + agp_logpdf_grad_batch — on the same inputs, in the same process.
    python tools/gpu_series_grad_perf.py [--reps R] [--out profiles/series_grad_perf.txt]
Prints one line per shape (S series x n points x particles per series): median [min, max] ms of both routes (host clock around calls
that end synchronised; programs encoded beforehand for both) over R timed repeats after a warm-up of each, the routes alternating
within every repeat; the fused route's kernel time (HIP events of one profiled call, agp_get_timing slot 0); the ratio of the medians;
and the worst disagreement between the routes over every gradient component (d / d noise included) of every particle both routes
factored, as |delta| / S_k with S_k the component's own error scale (oracle/gradcheck.py).  Nothing is asserted."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402
from oracle import gradcheck as GC      # noqa: E402


def spread(t):
    return f"{np.median(t):8.3f} [{t.min():.3f}, {t.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say("    S     n  P/S     P | fused ms median [min, max]  (kernels ms) | loop of set_data + logpdf_grad_batch ms median [min, max] | "
        "loop / fused | worst |delta| / S_k between the routes")
    for S, n, pps in ((64, 144, 8), (256, 126, 2), (1, 144, 8)):
        series, nodes, noises, progs = [], [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            ts, xs = pkg.prior.synthetic_series(n, seed=1000 + s, shuffle=True)
            series.append((ts, xs))
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(nz); progs.append(pkg.encode_batch(nd))
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)

        def fused():
            return eng.logpdf_grad_series_batch(series, None, all_noises, sidx, check=False, programs=all_progs)

        def loop():
            lp, gr, gn, info = [], [], [], []
            for s in range(S):
                eng.set_data(*series[s])
                r = eng.logpdf_grad_batch(None, noises[s], check=False, programs=progs[s])
                lp.append(r[0]); gr += r[1]; gn.append(r[2]); info.append(r[3])
            return np.concatenate(lp), gr, np.concatenate(gn), np.concatenate(info)
        a, b = fused(), loop()
        reps = args.reps if S > 1 else 10 * args.reps
        tf, tl = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); fused(); tf.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); loop(); tl.append(1e3 * (time.perf_counter() - t0))
        tf, tl = np.array(tf), np.array(tl)
        eng.set_profiling(True)
        fused()
        k_ms = eng.timing()["total_ms"]
        eng.set_profiling(False)
        worst, skipped = 0.0, 0
        for s in range(S):
            sel = range(s * pps, (s + 1) * pps)
            refs = GC.references([nodes[i] for i in sel], all_noises[s * pps:(s + 1) * pps], *series[s])
            for i, r in zip(sel, refs):
                if r is None or a[3][i] != 0 or b[3][i] != 0:
                    skipped += 1
                    continue
                ratios = GC.component_ratios(a[1][i], a[2][i], r, against=(b[1][i], b[2][i]))
                worst = max(worst, float(np.max(ratios)))
        say(f"{S:5d} {n:5d} {pps:4d} {S * pps:5d} | {spread(tf)}  ({k_ms:7.3f}) | {spread(tl)} | {np.median(tl) / np.median(tf):8.1f} | "
            f"{worst:.1e} ({skipped} particles not factored by a route or the oracle)")
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
