"""Forecasts of many short series: the fused entry (agp_predict_series_batch: one workgroup per (series, particle), factor and
posterior in LDS and registers, one call) against the only route the entries before it offered — a loop over the series of
agp_set_data + agp_predict_batch — on the same inputs.
    python tools/gpu_series_predict_perf.py [--reps R] [--resources FILE] [--out profiles/series_predict_perf.txt]
    python tools/gpu_series_predict_perf.py --resources-only [--out FILE]      (no GPU: compiles the kernel unit and reports)
Prints one line per shape (S series x n points x particles per series, m query times per series): median [min, max] ms of both routes
(host clock around calls that end synchronised; programs encoded beforehand for the fused route, predict_batch encodes its own) over R
timed repeats after a warm-up of each, the routes alternating within every repeat; the fused route's kernel time (HIP events of one
profiled call, agp_get_timing slot 0) beside the value entry's on the same input — the price of the prediction; the ratio of the
medians; and the largest disagreement between the routes relative to max(1, max|.|) per particle, mean and variance.
--resources-only compiles csrc/agp_kernels_series.hip with the kernel resource remarks on and prints VGPRs, scratch and static LDS of
the predictive instantiations beside k_series_logpdf's; --resources FILE copies such a report behind the timings."""
import argparse
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402


def spread(t):
    return f"{np.median(t):8.3f} [{t.min():.3f}, {t.max():.3f}]"


def resource_report():
    csrc = ROOT / "autogp.jl_amd" / "csrc"
    hipcc = subprocess.run("command -v hipcc || echo /opt/rocm/bin/hipcc", shell=True, capture_output=True, text=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                            "agp_kernels_series.hip", "-o", str(Path(tmp) / "unit.o")], cwd=csrc, capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    out = ["kernel (gfx950, -O3)                    VGPRs  AGPRs  scratch B/lane  static LDS B  waves/SIMD"]
    for want, label in ((r"k_series_logpdfILi4ELb0", "k_series_logpdf<4>"), (r"k_series_logpdfILi8ELb0", "k_series_logpdf<8>"),
                        (r"k_series_predictILi4E", "k_series_predict<4>"), (r"k_series_predictILi8E", "k_series_predict<8>")):
        k = next(x for x in rows if re.search(want, x["name"]))
        out.append(f"{label:40s} {k['VGPRs']:>5s}  {k['AGPRs']:>5s}  {k['ScratchSize [bytes/lane]']:>14s}  "
                   f"{k['LDS Size [bytes/block]']:>12s}  {k['Occupancy [waves/SIMD]']:>10s}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--resources", default="")
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    if args.resources_only:
        for s in resource_report():
            say(s)
        if args.out:
            Path(args.out).write_text("\n".join(lines) + "\n")
        return
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    say("    S     n  P/S     P    m | fused ms median [min, max]  (kernels ms; value entry's kernels ms) | "
        "loop of set_data + predict_batch ms median [min, max] | loop / fused | max rel diff mean, var")
    for S, n, pps, m in ((64, 144, 8, 36), (256, 126, 2, 12), (1, 144, 8, 36)):
        series, queries, nodes, noises, per_nodes = [], [], [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            ts, xs = pkg.prior.synthetic_series(n, seed=1000 + s, shuffle=True)
            series.append((ts, xs))
            queries.append(ts.max() + (ts.max() - ts.min()) * np.arange(1, m + 1) / (4.0 * m))
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(nz); per_nodes.append(nd)
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)

        def fused():
            return eng.predict_series_batch(series, queries, None, all_noises, sidx, check=False, programs=all_progs)

        def value():
            return eng.logpdf_series_batch(series, None, all_noises, sidx, check=False, programs=all_progs)

        def loop():
            means, vars_ = [], []
            for s in range(S):
                eng.set_data(*series[s])
                mu, var, _, _ = eng.predict_batch(per_nodes[s], noises[s], queries[s], check=False)
                means.append(mu); vars_.append(var)
            return np.concatenate(means), np.concatenate(vars_)
        a, b = fused(), loop()
        reps = args.reps if S > 1 else 10 * args.reps
        tf, tl = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); fused(); tf.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); loop(); tl.append(1e3 * (time.perf_counter() - t0))
        tf, tl = np.array(tf), np.array(tl)
        eng.set_profiling(True)
        kp, kv = [], []
        for _ in range(5):
            fused(); kp.append(eng.timing()["total_ms"])
            value(); kv.append(eng.timing()["total_ms"])
        eng.set_profiling(False)
        dm = dv = 0.0
        bad = 0
        for p in range(S * pps):
            fm, fv, rm, rv = a[0][p], a[1][p], b[0][p], b[1][p]
            if not (np.isfinite(fm).all() and np.isfinite(rm).all() and np.isfinite(fv).all() and np.isfinite(rv).all()):
                bad += 1
                continue
            dm = max(dm, np.abs(fm - rm).max() / max(1.0, np.abs(rm).max()))
            dv = max(dv, np.abs(fv - rv).max() / max(1.0, np.abs(rv).max()))
        say(f"{S:5d} {n:5d} {pps:4d} {S * pps:5d} {m:4d} | {spread(tf)}  ({np.median(kp):7.3f}; {np.median(kv):7.3f}) | {spread(tl)} | "
            f"{np.median(tl) / np.median(tf):8.1f} | {dm:.1e}, {dv:.1e} ({bad} particles non-finite)")
    eng.close()
    if args.resources:
        say("")
        for s in Path(args.resources).read_text().splitlines():
            say(s)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
