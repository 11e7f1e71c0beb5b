"""Forecasts and bands of series of 177 to 512 points: the long-series entries (agp_predict_long_series_batch,
agp_predict_quantile_long_series_batch: one workgroup per (series, particle), factor and solved query blocks in a per-workgroup HBM
workspace, one call for the whole family) against the only route the entries before them offered at these lengths — a loop over the
series of agp_set_data + agp_predict_batch / agp_predict_quantile_batch — on the same inputs.
    python tools/gpu_long_series_predict_perf.py [--reps R] [--loop-lib PATH] [--out profiles/long_series_predict_perf.txt]
--loop-lib: another build of the library for the loop routes (the comparison on record ran the parent commit's build there, so that
the baseline is the code a caller had before these entries existed); default: the library under test.
Prints two lines per shape (S series x n points x particles per series, m queries per series; "mixed" cycles 135 / 143 / 442
points), one for the forecast and one for the band at q = (0.025, 0.5, 0.975): median [min, max] ms of both routes (host clock
around calls that end synchronised; programs encoded beforehand for both) over R timed repeats after a warm-up of each, the routes
alternating within every repeat (10 R repeats for the single series); the long entry's kernel time and, for the band, its read-out
kernels' (HIP events of one profiled call, agp_get_timing slots 0 and 4); the value entry's kernel time on the same input (the
forecast's increment is the difference); the ratio of the medians; and the largest disagreement between the routes relative to
max(1, max|.|) per particle (forecast: mean and variance) or per series (band)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402

QS = np.array([0.025, 0.5, 0.975])


class LoopEngine:
    """agp_set_data + agp_predict_batch / agp_predict_quantile_batch of a library given by path, bound by hand (a build from before
    these entries lacks symbols load_library binds)"""

    def __init__(self, path):
        dp, ip, u8p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
        lib = self.lib = C.CDLL(str(path))
        lib.agp_init.argtypes = [C.POINTER(vp), C.c_int]; lib.agp_init.restype = C.c_int
        lib.agp_destroy.argtypes = [vp]; lib.agp_destroy.restype = None
        lib.agp_set_data.argtypes = [vp, dp, dp, C.c_int64]; lib.agp_set_data.restype = C.c_int
        lib.agp_predict_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp, dp, dp, ip]
        lib.agp_predict_batch.restype = C.c_int
        lib.agp_predict_quantile_batch.argtypes = [vp, C.c_int64, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp,
                                                   C.c_double, C.c_double, dp, C.c_int64, C.c_double, C.c_int64, dp, ip, ip, ip]
        lib.agp_predict_quantile_batch.restype = C.c_int
        self.ctx = vp()
        if lib.agp_init(C.byref(self.ctx), 0) != 0:
            raise RuntimeError(f"agp_init of {path} failed")
        self.dp, self.ip, self.u8p = dp, ip, u8p

    def set_data(self, ts, xs):
        if self.lib.agp_set_data(self.ctx, ts.ctypes.data_as(self.dp), xs.ctypes.data_as(self.dp), ts.shape[0]) != 0:
            raise RuntimeError("agp_set_data failed")

    def _particles(self, programs, noises):
        op_off, ops, prm_off, prm = programs
        return (noises.shape[0], op_off.ctypes.data_as(self.ip), ops.ctypes.data_as(self.u8p), prm_off.ctypes.data_as(self.ip),
                prm.ctypes.data_as(self.dp), noises.ctypes.data_as(self.dp), noises.ctypes.data_as(self.dp), None, None)

    def predict_batch(self, n, programs, noises, tq):
        P, m = noises.shape[0], tq.shape[0]
        mean = np.empty((P, m)); var = np.empty((P, m)); info = np.empty(P, dtype=np.int32)
        rc = self.lib.agp_predict_batch(self.ctx, n, tq.ctypes.data_as(self.dp), m, *self._particles(programs, noises),
                                        mean.ctypes.data_as(self.dp), var.ctypes.data_as(self.dp), None, info.ctypes.data_as(self.ip))
        if rc != 0:
            raise RuntimeError(f"agp_predict_batch failed ({rc})")
        return mean, var

    def predict_quantile_batch(self, n, programs, noises, tq, w):
        P, m, nq = noises.shape[0], tq.shape[0], QS.shape[0]
        x = np.empty(nq * m); conv = np.empty(nq * m, dtype=np.int32); it = np.empty(nq * m, dtype=np.int32); info = np.empty(P, dtype=np.int32)
        rc = self.lib.agp_predict_quantile_batch(self.ctx, n, tq.ctypes.data_as(self.dp), m, *self._particles(programs, noises),
                                                 w.ctypes.data_as(self.dp), 1.0, 0.0, QS.ctypes.data_as(self.dp), nq, 1e-5, 10**6,
                                                 x.ctypes.data_as(self.dp), conv.ctypes.data_as(self.ip), it.ctypes.data_as(self.ip),
                                                 info.ctypes.data_as(self.ip))
        if rc != 0:
            raise RuntimeError(f"agp_predict_quantile_batch failed ({rc})")
        return x.reshape(nq, m).T

    def close(self):
        self.lib.agp_destroy(self.ctx)


def spread(t):
    return f"{np.median(t):8.3f} [{t.min():.3f}, {t.max():.3f}]"


def block_diff(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else 0.0


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

    say(f"loop routes: {'the library given by --loop-lib' if args.loop_lib else 'the library under test'}")
    say("what          S      n  P/S     P    m | long entry ms median [min, max]  (kernels ms; band: + read-out ms; value entry's kernels ms) | "
        "loop ms median [min, max] | loop / long | max diff")
    for S, lens, pps, m in ((64, (442,), 8, 36), (16, (512,), 18, 64), (64, (135, 143, 442), 8, 36), (1, (442,), 8, 36)):
        series, queries, nodes, noises, progs, weights = [], [], [], [], [], []
        rng = np.random.default_rng(S + sum(lens))
        for s in range(S):
            n = lens[s % len(lens)]
            ts, xs = pkg.prior.synthetic_series(n, seed=2000 + s, shuffle=True)
            series.append((np.ascontiguousarray(ts), np.ascontiguousarray(xs)))
            queries.append(np.ascontiguousarray(ts.max() + (ts.max() - ts.min()) * np.arange(1, m + 1) / 40.0))
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(np.ascontiguousarray(nz, dtype=np.float64)); progs.append(pkg.encode_batch(nd))
            w = rng.random(pps) + 0.1
            weights.append(np.ascontiguousarray(w / w.sum()))
        all_noises = np.concatenate(noises); all_w = np.concatenate(weights)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)

        def fused():
            return eng.predict_long_series_batch(series, queries, None, all_noises, sidx, check=False, programs=all_progs)

        def loop():
            out = []
            for s in range(S):
                loop_eng.set_data(*series[s])
                out.append(loop_eng.predict_batch(series[s][0].shape[0], progs[s], noises[s], queries[s]))
            return out

        def fused_band():
            return eng.predict_quantile_long_series_batch(series, queries, None, all_noises, sidx, all_w, QS, check=False, programs=all_progs)

        def loop_band():
            out = []
            for s in range(S):
                loop_eng.set_data(*series[s])
                out.append(loop_eng.predict_quantile_batch(series[s][0].shape[0], progs[s], noises[s], queries[s], weights[s]))
            return out

        reps = args.reps if S > 1 else 10 * args.reps
        name = "mixed" if len(lens) > 1 else f"{lens[0]:5d}"
        eng.set_profiling(True)
        eng.logpdf_long_series_batch(series, None, all_noises, sidx, check=False, programs=all_progs)
        v_ms = eng.timing()["total_ms"]
        eng.set_profiling(False)
        for what, f, l in (("forecast", fused, loop), ("band", fused_band, loop_band)):
            a, b = f(), l()
            tf, tl = [], []
            for _ in range(reps):
                t0 = time.perf_counter(); f(); tf.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter(); l(); tl.append(1e3 * (time.perf_counter() - t0))
            tf, tl = np.array(tf), np.array(tl)
            eng.set_profiling(True)
            f()
            tm = eng.timing()
            eng.set_profiling(False)
            k_ms, r_ms = tm["total_ms"], tm["finish_ms"]      # (slots 0 and 4)
            if what == "forecast":
                diff = max(max(block_diff(a[0][s * pps + k], b[s][0][k]), block_diff(a[1][s * pps + k], b[s][1][k]))
                           for s in range(S) for k in range(pps))
                kern = f"({k_ms:7.3f}; value entry {v_ms:7.3f})"
            else:
                diff = max(block_diff(a.x[s], b[s]) for s in range(S))
                kern = f"({k_ms:7.3f} + read-out {r_ms:6.3f}; value entry {v_ms:7.3f})"
            say(f"{what:9s} {S:5d} {name:>6} {pps:4d} {S * pps:5d} {m:4d} | {spread(tf)}  {kern} | {spread(tl)} | "
                f"{np.median(tl) / np.median(tf):8.1f} | {diff:.1e}")
    loop_eng.close()
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
