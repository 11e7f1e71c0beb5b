#!/usr/bin/env python3
"""Crossover of agp_remove_data's factor update against the route a caller had before it: agp_set_data on the reduced series plus
one agp_logpdf_batch_extend (every particle refactored from scratch).  Feeds remove_admits (csrc/agp_host.hpp).

    python tools/gpu_remove_perf.py [--baseline-lib PATH] [--rounds 5] [--out profiles/remove_data_perf.txt]

Legs, per case (n, P, r, placement), interleaved round by round in ONE process, each timed with a host clock around calls that end
in a device synchronise (both entries return after their stream has drained):
  update    remove_data(idx) + logpdf_batch_extend at the new n, from factors resident on the full series (this build);
  baseline  set_data(reduced) + logpdf_batch_extend with an empty store.  --baseline-lib: a library built from the parent commit
            (the leg uses only entries that commit has); without it the leg runs on this build's library.
Untimed between rounds: set_data(full) + logpdf_batch_extend to make the full-series factors resident again.  One warm-up round per
case.  The table gives the median and minimum of each leg and the ratio of the medians; the update is admitted where it took at most
0.8 of the baseline."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as g      # noqa: E402


def positions(n, r, where):
    if where == "leading":
        return list(range(r))
    if where == "middle":
        a = n // 2 - r // 2
        return list(range(a, a + r))
    return sorted(np.random.default_rng(n + r).choice(n, size=r, replace=False).tolist())      # scattered


class Baseline:
    """set_data + logpdf_batch_extend through a second library (the parent commit's build): plain ctypes, the two entries only."""

    def __init__(self, path):
        lib = C.CDLL(str(path))
        dp, ip, u8p, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
        lib.agp_init.argtypes = [C.POINTER(vp), C.c_int]
        lib.agp_destroy.argtypes = [vp]; lib.agp_destroy.restype = None
        lib.agp_set_data.argtypes = [vp, dp, dp, C.c_int64]
        lib.agp_logpdf_batch_extend.argtypes = [vp, C.c_int64, C.c_int32, ip, u8p, ip, dp, dp, dp, ip]
        self.lib, self.ctx = lib, vp()
        assert lib.agp_init(C.byref(self.ctx), 0) == 0

    def set_data(self, ts, xs):
        self.n = ts.shape[0]
        assert self.lib.agp_set_data(self.ctx, ts.ctypes.data_as(C.POINTER(C.c_double)), xs.ctypes.data_as(C.POINTER(C.c_double)), self.n) == 0

    def score(self, progs, noises):
        op_off, ops, prm_off, prm = progs
        P = op_off.shape[0] - 1
        out = np.empty(P); info = np.empty(P, dtype=np.int32)
        as_ = lambda a, t: a.ctypes.data_as(C.POINTER(t))      # noqa: E731
        assert self.lib.agp_logpdf_batch_extend(self.ctx, self.n, P, as_(op_off, C.c_int32), as_(ops, C.c_uint8), as_(prm_off, C.c_int32),
                                                as_(prm, C.c_double), as_(noises, C.c_double), as_(out, C.c_double), as_(info, C.c_int32)) == 0
        return out, info

    def close(self):
        self.lib.agp_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--P", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--r", type=int, nargs="*", default=[1, 8, 32, 128, 512])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.GPEngine(0)
    eng.set_remove_update(2)      # every case is updated, whatever the rule in force says
    base = Baseline(a.baseline_lib) if a.baseline_lib else None
    lines = ["# n P r placement runs | update ms (median, min) | baseline ms (median, min) | ratio | updated dropped | max |dlogpdf| rel",
             f"# baseline leg: {'library ' + Path(a.baseline_lib).name + ' (parent commit build)' if base else 'this build'}; rounds {a.rounds} + 1 warm-up"]
    print("\n".join(lines), flush=True)
    for n in a.n:
        ts, xs = pkg.prior.synthetic_series(n, seed=n, shuffle=True)
        ts = np.ascontiguousarray(ts + 1e-4 * np.random.default_rng(n).uniform(-1, 1, n))      # irregular: the general evaluator on both legs
        for P in a.P:
            nodes, noises = pkg.prior.sample_particles(np.random.default_rng(P), P, max_depth=4, max_size=31)
            noises = np.ascontiguousarray(np.maximum(noises, 1e-2))
            progs = pkg.encode_batch(nodes)
            for r in a.r:
                if r >= n:
                    continue
                for where in ("leading", "middle", "scattered"):
                    idx = positions(n, r, where)
                    keep = np.setdiff1d(np.arange(n), idx)
                    tr, xr = np.ascontiguousarray(ts[keep]), np.ascontiguousarray(xs[keep])
                    runs = 1 + int((np.diff(idx) > 1).sum())
                    tu, tb = [], []
                    err = 0.0
                    s0 = eng.remove_stats()
                    rounds = a.rounds if runs <= 32 else 1      # (hundreds of runs: one shifted copy of the trailing factor each — seconds per call)
                    for rnd in range(rounds + 1):
                        eng.set_data(ts, xs); eng.extend_reset()
                        eng.logpdf_batch_extend(None, noises, check=False, programs=progs)
                        t0 = time.perf_counter()
                        eng.remove_data(idx)
                        lp, info = eng.logpdf_batch_extend(None, noises, check=False, programs=progs)
                        t1 = time.perf_counter()
                        if base:
                            base.set_data(ts, xs)      # another series: empties the baseline's store
                            t2 = time.perf_counter()
                            base.set_data(tr, xr)
                            lb, ib = base.score(progs, noises)
                            t3 = time.perf_counter()
                        else:
                            eng.set_data(ts, xs); eng.extend_reset()
                            t2 = time.perf_counter()
                            eng.set_data(tr, xr)
                            lb, ib = eng.logpdf_batch_extend(None, noises, check=False, programs=progs)
                            t3 = time.perf_counter()
                        ok = (info == 0) & (ib == 0)
                        err = max(err, float((np.abs(lp[ok] - lb[ok]) / np.maximum(1.0, np.abs(lb[ok]))).max()))
                        if rnd > 0:
                            tu.append((t1 - t0) * 1e3); tb.append((t3 - t2) * 1e3)
                    s1 = eng.remove_stats()
                    mu, mb = statistics.median(tu), statistics.median(tb)
                    line = (f"{n} {P} {r} {where} {runs} | {mu:.3f} {min(tu):.3f} | {mb:.3f} {min(tb):.3f} | {mu / mb:.3f} | "
                            f"{(s1['updated'] - s0['updated']) // (rounds + 1)} {(s1['dropped'] - s0['dropped']) // (rounds + 1)} | {err:.2e}")
                    lines.append(line)
                    print(line, flush=True)
                    if a.out:
                        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                        Path(a.out).write_text("\n".join(lines) + "\n")
    eng.close()
    if base:
        base.close()


if __name__ == "__main__":
    main()
