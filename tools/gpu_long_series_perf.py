"""Series of 177 to 512 points: the long-series entry (agp_logpdf_long_series_batch: one workgroup per (series, particle), the factor
in a per-workgroup HBM workspace, one call for the whole family) against the only route the entries before it offered at these
lengths — a loop over the series of agp_set_data + agp_logpdf_batch — on the same inputs.
    python tools/gpu_long_series_perf.py [--reps R] [--loop-lib PATH] [--out profiles/long_series_perf.txt]
--loop-lib: another build of the library for the loop route (the comparison on record ran the parent commit's build there, so that
the baseline is the code a caller had before this entry existed); default: the library under test.
Prints one line per shape (S series x n points x particles per series; "mixed" cycles 135 / 143 / 442 points): median [min, max] ms of
both routes (host clock around calls that end synchronised; programs encoded beforehand for both) over R timed repeats after a
warm-up of each, the routes alternating within every repeat (10 R repeats for the single series); the long entry's kernel time (HIP
events of one profiled call, agp_get_timing slot 0); the ratio of the medians; and the largest disagreement between the routes
relative to max(1, |logpdf|)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402


class LoopEngine:
    """agp_set_data + agp_logpdf_batch of a library given by path: the two entries the loop route needs, bound by hand (a build from
    before this entry lacks symbols load_library binds)"""

    def __init__(self, path):
        dp, ip, u8p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
        lib = self.lib = C.CDLL(str(path))
        lib.agp_init.argtypes = [C.POINTER(vp), C.c_int]; lib.agp_init.restype = C.c_int
        lib.agp_destroy.argtypes = [vp]; lib.agp_destroy.restype = None
        lib.agp_set_data.argtypes = [vp, dp, dp, C.c_int64]; lib.agp_set_data.restype = C.c_int
        lib.agp_logpdf_batch.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, ip]; lib.agp_logpdf_batch.restype = C.c_int
        self.ctx = vp()
        if lib.agp_init(C.byref(self.ctx), 0) != 0:
            raise RuntimeError(f"agp_init of {path} failed")
        self.dp, self.ip, self.u8p = dp, ip, u8p

    def set_data(self, ts, xs):
        if self.lib.agp_set_data(self.ctx, ts.ctypes.data_as(self.dp), xs.ctypes.data_as(self.dp), ts.shape[0]) != 0:
            raise RuntimeError("agp_set_data failed")

    def logpdf_batch(self, n, programs, noises):
        op_off, ops, prm_off, prm = programs
        P = noises.shape[0]
        out = np.empty(P); info = np.empty(P, dtype=np.int32)
        rc = self.lib.agp_logpdf_batch(self.ctx, n, P, op_off.ctypes.data_as(self.ip), ops.ctypes.data_as(self.u8p),
                                       prm_off.ctypes.data_as(self.ip), prm.ctypes.data_as(self.dp), noises.ctypes.data_as(self.dp),
                                       out.ctypes.data_as(self.dp), info.ctypes.data_as(self.ip))
        if rc != 0:
            raise RuntimeError(f"agp_logpdf_batch failed ({rc})")
        return out

    def close(self):
        self.lib.agp_destroy(self.ctx)


def spread(t):
    return f"{np.median(t):8.3f} [{t.min():.3f}, {t.max():.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    loop_eng = LoopEngine(args.loop_lib or pkg.LIB_PATH)
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"loop route: {'the library given by --loop-lib' if args.loop_lib else 'the library under test'}")
    say("    S      n  P/S     P | long entry ms median [min, max]  (kernels ms) | loop of set_data + logpdf_batch ms median [min, max] | "
        "loop / long | max rel diff")
    for S, lens, pps in ((64, (442,), 8), (16, (512,), 18), (64, (135, 143, 442), 8), (1, (442,), 8)):
        series, nodes, noises, progs = [], [], [], []
        rng = np.random.default_rng(S + sum(lens))
        for s in range(S):
            n = lens[s % len(lens)]
            ts, xs = pkg.prior.synthetic_series(n, seed=2000 + s, shuffle=True)
            series.append((np.ascontiguousarray(ts), np.ascontiguousarray(xs)))
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(np.ascontiguousarray(nz, dtype=np.float64)); progs.append(pkg.encode_batch(nd))
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)

        def fused():
            return eng.logpdf_long_series_batch(series, None, all_noises, sidx, check=False, programs=all_progs)[0]

        def loop():
            out = []
            for s in range(S):
                loop_eng.set_data(*series[s])
                out.append(loop_eng.logpdf_batch(series[s][0].shape[0], progs[s], noises[s]))
            return np.concatenate(out)
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
        ok = np.isfinite(a) & np.isfinite(b)
        diff = float((np.abs(a - b)[ok] / np.maximum(1.0, np.abs(b[ok]))).max())
        name = "mixed" if len(lens) > 1 else f"{lens[0]:5d}"
        say(f"{S:5d} {name:>6} {pps:4d} {S * pps:5d} | {spread(tf)}  ({k_ms:7.3f}) | {spread(tl)} | {np.median(tl) / np.median(tf):8.1f} | "
            f"{diff:.1e} ({int((~ok).sum())} non-finite)")
    loop_eng.close()
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
