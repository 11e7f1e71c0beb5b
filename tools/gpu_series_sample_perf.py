"""Sample paths of many short series: the fused entry (agp_predict_sample_series_batch: one workgroup per (series, particle)
factors the joint matrix of training and query points in LDS and reads samples, component means and covariances out of the query
rows, one call) against the only route the entries before it offered — a loop over the series of agp_set_data +
agp_predict_sample_batch — on the same inputs and seeds.
    python tools/gpu_series_sample_perf.py [--reps R] [--resources FILE] [--out profiles/series_sample_perf.txt]
    python tools/gpu_series_sample_perf.py --resources-only [--out FILE]      (no GPU: compiles the kernel unit and reports)
Prints one line per shape (S series x (n training + m query points) x particles per series) and number of samples R per series:
median [min, max] ms of both routes (host clock around calls that end synchronised; programs encoded beforehand for the fused route,
predict_sample_batch encodes its own) over R timed repeats after a warm-up of each, the routes alternating within every repeat; the
fused route's kernel time (HIP events of one profiled call, agp_get_timing slot 0; slot 4 is the NaN-fill read-out) beside the
held-out entry's kernel time on the same input in the same process — the same factorisation, so the difference is the read-out's
cost; the ratio of the medians; whether the components agree; and the largest disagreement between the routes' samples in units of
the tests' bound 1e-8 max(1, max|x|) per sample.
--resources-only compiles csrc/agp_kernels_series.hip with the kernel resource remarks on and prints VGPRs, scratch and static LDS of
the sampling instantiations beside the held-out twin's; --resources FILE copies such a report behind the timings."""
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
sys.path.insert(0, str(ROOT / "tests"))
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
    for want, label in ((r"k_series_predict_logpdfILi4E", "k_series_predict_logpdf<4>"), (r"k_series_predict_logpdfILi8E", "k_series_predict_logpdf<8>"),
                        (r"k_series_predict_sampleILi4E", "k_series_predict_sample<4>"), (r"k_series_predict_sampleILi8E", "k_series_predict_sample<8>"),
                        (r"k_series_sample_fill", "k_series_sample_fill")):
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
    say("    S     n    m  P/S     P     R | fused ms median [min, max]  (kernels ms + NaN-fill ms; held-out entry's kernels ms) | "
        "loop of set_data + predict_sample_batch ms median [min, max] | loop / fused | components equal | max |fused - loop| / bound")
    for S, n, m, pps in ((64, 126, 18, 8), (256, 114, 12, 2), (1, 126, 18, 8)):
        series, queries, held, nodes, noises, per_nodes = [], [], [], [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            ts, xs = pkg.prior.synthetic_series(n + m, seed=1000 + s)      # (in time order: the last m points are the horizon)
            series.append((ts[:n].copy(), xs[:n].copy()))
            queries.append(ts[n:].copy()); held.append(xs[n:].copy())
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(nz); per_nodes.append(nd)
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)
        w = np.full(S * pps, 1.0 / pps)
        ws = np.full(pps, 1.0 / pps)
        seeds = np.arange(500, 500 + S, dtype=np.uint64)
        for R in (100, 1000):
            def fused():
                return eng.predict_sample_series_batch(series, queries, None, all_noises, sidx, w, R, seeds=seeds, check=False,
                                                       programs=all_progs)

            def heldout():
                return eng.predict_logpdf_series_batch(series, queries, held, None, all_noises, sidx, check=False, programs=all_progs)

            def loop():
                xs_, cs_, infos = [], [], []
                for s in range(S):
                    eng.set_data(*series[s])
                    x, c, info = eng.predict_sample_batch(per_nodes[s], noises[s], queries[s], ws, R, seed=int(seeds[s]), check=False)
                    xs_.append(x); cs_.append(c + s * pps); infos.append(info)
                return xs_, np.stack(cs_), np.concatenate(infos)
            a, b = fused(), loop()
            reps = args.reps if S > 1 else 10 * args.reps
            tf, tl = [], []
            for _ in range(reps):
                t0 = time.perf_counter(); fused(); tf.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter(); loop(); tl.append(1e3 * (time.perf_counter() - t0))
            tf, tl = np.array(tf), np.array(tl)
            eng.set_profiling(True)
            kp, kr, kv = [], [], []
            for _ in range(5):
                fused(); t = eng.timing(); kp.append(t["total_ms"]); kr.append(t["finish_ms"])
                heldout(); kv.append(eng.timing()["total_ms"])
            eng.set_profiling(False)
            worst, bad = 0.0, 0
            for s in range(S):
                sel = slice(s * pps, (s + 1) * pps)
                if (a.info[sel] != 0).any() or (b[2][sel] != 0).any():
                    bad += 1
                    continue
                err = np.abs(a.x[s] - b[0][s]).max(axis=0) / (1e-8 * np.maximum(1.0, np.abs(b[0][s]).max(axis=0)))
                worst = max(worst, float(err.max()))
            same = bool(np.array_equal(a.component, b[1]))
            say(f"{S:5d} {n:5d} {m:4d} {pps:4d} {S * pps:5d} {R:5d} | {spread(tf)}  ({np.median(kp):7.3f} + {np.median(kr):6.3f}; {np.median(kv):7.3f}) | "
                f"{spread(tl)} | {np.median(tl) / np.median(tf):8.1f} | {same} | {worst:.1e} ({bad} series with a particle a route could not factor)")
    eng.close()
    if args.resources:
        say("")
        for s in Path(args.resources).read_text().splitlines():
            say(s)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
