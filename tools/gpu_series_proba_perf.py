"""Held-out scores of many short series: the fused entry (agp_predict_logpdf_series_batch: one workgroup per (series, particle)
factors the joint matrix of training and held-out points in LDS, the mixtures are read out on the device, one call) against the only
route the entries before it offered — a loop over the series of agp_set_data + agp_predict_logpdf_batch — on the same inputs.
    python tools/gpu_series_proba_perf.py [--reps R] [--resources FILE] [--out profiles/series_proba_perf.txt]
    python tools/gpu_series_proba_perf.py --resources-only [--out FILE]      (no GPU: compiles the kernel unit and reports)
Prints one line per shape (S series x (n training + m held-out points) x particles per series): median [min, max] ms of both routes
(host clock around calls that end synchronised; programs encoded beforehand for the fused route, predict_logpdf_batch encodes its own)
over R timed repeats after a warm-up of each, the routes alternating within every repeat; the fused route's kernel time (HIP events
of one profiled call, agp_get_timing slot 0; slot 4 is the mixture read-out) beside the value entry's on the CONCATENATED series — the
same factorisation; the ratio of the medians; and the largest disagreement between the routes in units of the error scale S of
tests/_pred_logpdf_ref.reference, over the particles both routes factor.
--resources-only compiles csrc/agp_kernels_series.hip with the kernel resource remarks on and prints VGPRs, scratch and static LDS of
the held-out instantiations beside k_series_logpdf's; --resources FILE copies such a report behind the timings."""
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
    for want, label in ((r"k_series_logpdfILi4ELb0", "k_series_logpdf<4>"), (r"k_series_logpdfILi8ELb0", "k_series_logpdf<8>"),
                        (r"k_series_predict_logpdfILi4E", "k_series_predict_logpdf<4>"),
                        (r"k_series_predict_logpdfILi8E", "k_series_predict_logpdf<8>")):
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
    import _pred_logpdf_ref as PR
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    say("    S     n    m  P/S     P | fused ms median [min, max]  (kernels ms + mixture read-out ms; value entry's kernels ms on n + m) | "
        "loop of set_data + predict_logpdf_batch ms median [min, max] | loop / fused | max |fused - loop| / S")
    for S, n, m, pps in ((64, 126, 18, 8), (256, 114, 12, 2), (1, 126, 18, 8)):
        series, joint, queries, held, nodes, noises, per_nodes = [], [], [], [], [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            ts, xs = pkg.prior.synthetic_series(n + m, seed=1000 + s)      # (in time order: the last m points are held out)
            series.append((ts[:n].copy(), xs[:n].copy())); joint.append((ts, xs))
            queries.append(ts[n:].copy()); held.append(xs[n:].copy())
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(nz); per_nodes.append(nd)
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)
        w = np.full(S * pps, 1.0 / pps)

        def fused():
            return eng.predict_logpdf_series_batch(series, queries, held, None, all_noises, sidx, weights=w, check=False, programs=all_progs)

        def value():
            return eng.logpdf_series_batch(joint, None, all_noises, sidx, check=False, programs=all_progs)

        def loop():
            lps, infos = [], []
            for s in range(S):
                eng.set_data(*series[s])
                lp, info = eng.predict_logpdf_batch(per_nodes[s], noises[s], queries[s], held[s], check=False)
                lps.append(lp); infos.append(info)
            return np.concatenate(lps), np.concatenate(infos)
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
            value(); kv.append(eng.timing()["total_ms"])
        eng.set_profiling(False)
        worst, bad = 0.0, 0
        for p in range(S * pps):
            s = int(sidx[p])
            if a.info[p] != 0 or b[1][p] != 0:
                bad += 1
                continue
            try:
                _, scale = PR.reference(nodes[p].to_tuple(), float(all_noises[p]), *series[s], queries[s], held[s])
            except Exception:      # (the fp64 reference cannot factor what both device routes did: no scale to measure in)
                bad += 1
                continue
            worst = max(worst, abs(a.logpdf[p] - b[0][p]) / scale)
        say(f"{S:5d} {n:5d} {m:4d} {pps:4d} {S * pps:5d} | {spread(tf)}  ({np.median(kp):7.3f} + {np.median(kr):6.3f}; {np.median(kv):7.3f}) | "
            f"{spread(tl)} | {np.median(tl) / np.median(tf):8.1f} | {worst:.1e} ({bad} particles not factored by a route or the reference)")
    eng.close()
    if args.resources:
        say("")
        for s in Path(args.resources).read_text().splitlines():
            say(s)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
