"""Decompositions of many short series: the fused entry (agp_predict_sum_series_batch: one workgroup per (series, particle), factor,
coded query rows and read-out in LDS and registers, one call) against the only route the entries before it offered — a loop over the
series of agp_set_data + agp_predict_sum_batch — on the same inputs.
    python tools/gpu_series_sum_perf.py [--reps R] [--loop-lib LIB] [--resources FILE] [--out profiles/series_sum_perf.txt]
    python tools/gpu_series_sum_perf.py --resources-only [--out FILE]      (no GPU: compiles the kernel unit and reports)
Every particle's kernel is split by split_kernel_sop(node, Periodic) (M = 2), q = (0.025, 0.5, 0.975).  Prints one line per shape
(S series x n points x particles per series, m query times per series): median [min, max] ms of both routes (host clock around calls
that end synchronised; the components encoded beforehand for both routes) over R timed repeats after a warm-up of each, the
routes alternating within every repeat; the fused route's kernel time (HIP events of one profiled call, agp_get_timing slot 0) beside that of
agp_predict_series_batch on the UNSPLIT kernels at 3 m queries per series — the same number of rows solved against the same factor,
the yardstick of what the composite programs and the read-out cost; the ratio of the medians; and the largest disagreement between
the routes relative to max(1, max|.|) per particle, means and quantiles.
--loop-lib LIB runs the loop on another build of the library (the parent commit's: the loop's entries exist there), through a second
context of this process; without it the loop runs on the library under test, whose loop entries are the same code.
--resources-only compiles csrc/agp_kernels_series.hip with the kernel resource remarks on and prints VGPRs, scratch and static LDS of
the new instantiations beside k_series_predict's; --resources FILE copies such a report behind the timings."""
import argparse
import ctypes as C
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

Q = (0.025, 0.5, 0.975)


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
    for want, label in ((r"k_series_predictILi4E", "k_series_predict<4>"), (r"k_series_predictILi8E", "k_series_predict<8>"),
                        (r"k_series_predict_sumILi4E", "k_series_predict_sum<4>"), (r"k_series_predict_sumILi8E", "k_series_predict_sum<8>")):
        k = next(x for x in rows if re.search(want, x["name"]))
        out.append(f"{label:40s} {k['VGPRs']:>5s}  {k['AGPRs']:>5s}  {k['ScratchSize [bytes/lane]']:>14s}  "
                   f"{k['LDS Size [bytes/block]']:>12s}  {k['Occupancy [waves/SIMD]']:>10s}")
    return out


class LoopLibrary:
    """agp_set_data + agp_predict_sum_batch of another build of the library, on a context of its own"""

    def __init__(self, path):
        dp, ip, u8p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
        self.lib = lib = C.CDLL(str(path))
        lib.agp_init.argtypes = [C.POINTER(vp), C.c_int]; lib.agp_init.restype = C.c_int
        lib.agp_destroy.argtypes = [vp]; lib.agp_destroy.restype = None
        lib.agp_set_data.argtypes = [vp, dp, dp, C.c_int64]; lib.agp_set_data.restype = C.c_int
        lib.agp_predict_sum_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, C.c_int32, ip, u8p, ip, dp, dp, dp, C.c_double,
                                              C.c_double, dp, C.c_int64, dp, dp, ip]
        lib.agp_predict_sum_batch.restype = C.c_int
        self.ctx = vp()
        if lib.agp_init(C.byref(self.ctx), 0) != 0:
            raise RuntimeError(f"agp_init failed in {path}")

    def close(self):
        self.lib.agp_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--loop-lib", default="")
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
    other = LoopLibrary(args.loop_lib) if args.loop_lib else None
    lib, ctx = (other.lib, other.ctx) if other else (eng._lib, eng._ctx)
    dp, ip, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    qa = np.array(Q)
    say(f"loop route on: {args.loop_lib or 'the library under test'}")
    say("    S     n  P/S     P    m | fused ms median [min, max]  (kernels ms; predict_series_batch's kernels at 3 m queries ms) | "
        "loop of set_data + predict_sum_batch ms median [min, max] | loop / fused | max rel diff mean, quantiles")
    for S, n, pps, m in ((64, 144, 8, 36), (256, 126, 2, 12), (1, 144, 8, 36)):
        series, queries, queries3, nodes, splits, noises, per = [], [], [], [], [], [], []
        rng = np.random.default_rng(S + n)
        for s in range(S):
            ts, xs = pkg.prior.synthetic_series(n, seed=1000 + s, shuffle=True)
            series.append((np.ascontiguousarray(ts), np.ascontiguousarray(xs)))
            tq = ts.max() + (ts.max() - ts.min()) * np.arange(1, m + 1) / (4.0 * m)
            queries.append(tq); queries3.append(np.tile(tq, 3))
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            sp = [pkg.split_kernel_sop(k, pkg.Periodic) for k in nd]
            nodes += nd; splits += sp; noises.append(np.ascontiguousarray(nz, dtype=np.float64))
            per.append(pkg.encode_batch([c for pair in sp for c in pair]))
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        split_progs = pkg.encode_batch([c for pair in splits for c in pair])
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)
        rows = 3 * m

        def fused():
            return eng.predict_sum_series_batch(series, queries, None, all_noises, sidx, q=Q, check=False, programs=split_progs)

        def yardstick():
            return eng.predict_series_batch(series, queries3, None, all_noises, sidx, check=False, programs=all_progs)

        def loop():
            means, xq = np.empty((S * pps, rows)), np.empty((S * pps, rows, 3))
            info = np.zeros(pps, dtype=np.int32)
            for s in range(S):
                ts, xs = series[s]
                op_off, ops, prm_off, prm = per[s]
                mu, x = means[s * pps:(s + 1) * pps], xq[s * pps:(s + 1) * pps]
                rc = lib.agp_set_data(ctx, ts.ctypes.data_as(dp), xs.ctypes.data_as(dp), n)
                rc = rc or lib.agp_predict_sum_batch(ctx, n, queries[s].ctypes.data_as(dp), m, pps, 2, op_off.ctypes.data_as(ip),
                                                     ops.ctypes.data_as(u8p), prm_off.ctypes.data_as(ip), prm.ctypes.data_as(dp),
                                                     noises[s].ctypes.data_as(dp), None, 1.0, 0.0, qa.ctypes.data_as(dp), 3,
                                                     mu.ctypes.data_as(dp), x.ctypes.data_as(dp), info.ctypes.data_as(ip))
                if rc != 0:
                    raise RuntimeError(f"loop route failed on series {s} ({rc})")
            return means, xq
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
            yardstick(); kv.append(eng.timing()["total_ms"])
        eng.set_profiling(False)
        dm = dx = 0.0
        bad = 0
        for p in range(S * pps):
            fm, fx, rm, rx = a.mean[p], a.x[p], b[0][p], b[1][p]
            if not (np.isfinite(fm).all() and np.isfinite(rm).all() and np.isfinite(fx).all() and np.isfinite(rx).all()):
                bad += 1
                continue
            dm = max(dm, np.abs(fm - rm).max() / max(1.0, np.abs(rm).max()))
            dx = max(dx, np.abs(fx - rx).max() / max(1.0, np.abs(rx).max()))
        say(f"{S:5d} {n:5d} {pps:4d} {S * pps:5d} {m:4d} | {spread(tf)}  ({np.median(kp):7.3f}; {np.median(kv):7.3f}) | {spread(tl)} | "
            f"{np.median(tl) / np.median(tf):8.1f} | {dm:.1e}, {dx:.1e} ({bad} particles non-finite)")
    if other:
        other.close()
    eng.close()
    if args.resources:
        say("")
        for s in Path(args.resources).read_text().splitlines():
            say(s)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
