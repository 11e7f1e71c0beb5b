"""Held-out scores of series of 177 to 512 joint points: the long entry (agp_predict_logpdf_long_series_batch: one workgroup per
(series, particle) factors the joint matrix of training and held-out points in a per-workgroup HBM workspace, the mixtures are read
out on the device, one call for the whole family) against the only route the entries before it offered at these lengths — a loop over
the series of agp_set_data + agp_predict_logpdf_batch — on the same inputs.
    python tools/gpu_long_series_proba_perf.py [--reps R] [--loop-lib PATH] [--out profiles/long_series_proba_perf.txt]
--loop-lib: another build of the library for the loop route (the comparison on record ran the parent commit's build there, so that
the baseline is the code a caller had before this entry existed); default: the library under test.
Prints one line per shape (S series x (n training + m held-out points) x particles per series; "mixed" cycles 117 + 18 / 125 + 18 /
406 + 36): median [min, max] ms of both routes (host clock around calls that end synchronised; programs encoded beforehand for both)
over R timed repeats after a warm-up of each, the routes alternating within every repeat (10 R repeats for the single series); the
long entry's kernel time and its mixture read-out (HIP events, agp_get_timing slots 0 and 4) beside the long VALUE entry's kernel
time on the CONCATENATED series — the same factorisation —, each the median [min, max] of 9 profiled calls, the two alternating; the
ratio of the medians of the routes; and the largest disagreement between the routes relative to max(1, |logpdf|)."""
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
    """agp_set_data + agp_predict_logpdf_batch of a library given by path, bound by hand (a build from before this entry lacks a
    symbol load_library binds)"""

    def __init__(self, path):
        dp, ip, u8p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
        lib = self.lib = C.CDLL(str(path))
        lib.agp_init.argtypes = [C.POINTER(vp), C.c_int]; lib.agp_init.restype = C.c_int
        lib.agp_destroy.argtypes = [vp]; lib.agp_destroy.restype = None
        lib.agp_set_data.argtypes = [vp, dp, dp, C.c_int64]; lib.agp_set_data.restype = C.c_int
        lib.agp_predict_logpdf_batch.argtypes = [vp, C.c_int64, dp, dp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, dp, dp, dp, ip]
        lib.agp_predict_logpdf_batch.restype = C.c_int
        self.ctx = vp()
        if lib.agp_init(C.byref(self.ctx), 0) != 0:
            raise RuntimeError(f"agp_init of {path} failed")
        self.dp, self.ip, self.u8p = dp, ip, u8p

    def set_data(self, ts, xs):
        if self.lib.agp_set_data(self.ctx, ts.ctypes.data_as(self.dp), xs.ctypes.data_as(self.dp), ts.shape[0]) != 0:
            raise RuntimeError("agp_set_data failed")

    def predict_logpdf_batch(self, n, programs, noises, tq, y):
        op_off, ops, prm_off, prm = programs
        P, m = noises.shape[0], tq.shape[0]
        lp = np.empty(P); info = np.empty(P, dtype=np.int32)
        rc = self.lib.agp_predict_logpdf_batch(self.ctx, n, tq.ctypes.data_as(self.dp), y.ctypes.data_as(self.dp), m, P,
                                               op_off.ctypes.data_as(self.ip), ops.ctypes.data_as(self.u8p), prm_off.ctypes.data_as(self.ip),
                                               prm.ctypes.data_as(self.dp), noises.ctypes.data_as(self.dp), None, None, None,
                                               lp.ctypes.data_as(self.dp), info.ctypes.data_as(self.ip))
        if rc != 0:
            raise RuntimeError(f"agp_predict_logpdf_batch failed ({rc})")
        return lp, info

    def close(self):
        self.lib.agp_destroy(self.ctx)


def spread(t, width=8):
    t = np.asarray(t)
    return f"{np.median(t):{width}.3f} [{t.min():.3f}, {t.max():.3f}]"


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
    say("    S   n + m  P/S     P | long entry ms median [min, max] | its kernels ms | mixture read-out ms | value entry's kernels ms on the "
        "concatenated series | loop ms median [min, max] | loop / long | max diff")
    for S, splits, pps in ((64, ((144, 36),), 8), (64, ((406, 36),), 8), (16, ((448, 64),), 18),
                           (64, ((117, 18), (125, 18), (406, 36)), 8), (1, ((406, 36),), 8)):
        series, joint, queries, held, nodes, noises, progs = [], [], [], [], [], [], []
        rng = np.random.default_rng(S + sum(n + m for n, m in splits))
        for s in range(S):
            n, m = splits[s % len(splits)]
            ts, xs = pkg.prior.synthetic_series(n + m, seed=3000 + s)      # (in time order: the last m points are held out)
            ts, xs = np.ascontiguousarray(ts), np.ascontiguousarray(xs)
            series.append((ts[:n].copy(), xs[:n].copy())); joint.append((ts, xs))
            queries.append(ts[n:].copy()); held.append(xs[n:].copy())
            nd, nz = pkg.prior.sample_particles(rng, pps, max_depth=3)
            nodes += nd; noises.append(np.ascontiguousarray(nz, dtype=np.float64)); progs.append(pkg.encode_batch(nd))
        all_noises = np.concatenate(noises)
        all_progs = pkg.encode_batch(nodes)
        sidx = np.repeat(np.arange(S, dtype=np.int32), pps)
        w = np.full(S * pps, 1.0 / pps)

        def fused():
            return eng.predict_logpdf_long_series_batch(series, queries, held, None, all_noises, sidx, weights=w, check=False,
                                                        programs=all_progs)

        def value():
            return eng.logpdf_long_series_batch(joint, None, all_noises, sidx, check=False, programs=all_progs)

        def loop():
            lps, infos = [], []
            for s in range(S):
                loop_eng.set_data(*series[s])
                lp, info = loop_eng.predict_logpdf_batch(series[s][0].shape[0], progs[s], noises[s], queries[s], held[s])
                lps.append(lp); infos.append(info)
            return np.concatenate(lps), np.concatenate(infos)

        a, b = fused(), loop()
        value()
        reps = args.reps if S > 1 else 10 * args.reps
        tf, tl = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); fused(); tf.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); loop(); tl.append(1e3 * (time.perf_counter() - t0))
        tf, tl = np.array(tf), np.array(tl)
        eng.set_profiling(True)
        kp, kr, kv = [], [], []
        for _ in range(9):
            fused(); t = eng.timing(); kp.append(t["total_ms"]); kr.append(t["finish_ms"])      # (slots 0 and 4)
            value(); kv.append(eng.timing()["total_ms"])
        eng.set_profiling(False)
        ok = (a.info == 0) & (b[1] == 0)
        diff = float((np.abs(a.logpdf[ok] - b[0][ok]) / np.maximum(1.0, np.abs(b[0][ok]))).max())
        name = "mixed" if len(splits) > 1 else f"{splits[0][0]}+{splits[0][1]}"
        say(f"{S:5d} {name:>7} {pps:4d} {S * pps:5d} | {spread(tf)} | {spread(kp, 7)} | {spread(kr, 6)} | {spread(kv, 7)} | {spread(tl)} | "
            f"{np.median(tl) / np.median(tf):8.1f} | {diff:.1e} ({int((~ok).sum())} particles not factored by a route)")
    loop_eng.close()
    eng.close()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
