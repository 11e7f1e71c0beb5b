"""A/B of two builds of the library over the resident-series sweeps (csrc/agp_engine.hip logpdf_batch_impl and the entries in front of
it): every output array and counter vector of a fixed, seeded list of calls must be BIT-IDENTICAL, and the calls must not get slower.
The C ABI is the same on both sides, so one Python layer drives either library through AUTOGP_HIP_LIB.

    AUTOGP_HIP_LIB=<library> python tools/gpu_sweep_refactor_ab.py run <label> <out.npz>      one fresh process per run
    python tools/gpu_sweep_refactor_ab.py compare <parent.npz> <new.npz> <parent.npz> <new.npz> ...

Run the processes alternating parent / new / parent / new.  The list names each route through the function at the smallest shape that
reaches it (a 128-point tile: two tiles are n = 129); the builders are the tests' (tests/_sweep_cases.py).  Each case runs with the
default workspace and again limited to three particles per chunk; the counters are read after each.  The class-aware coalesced mode
is driven by threads, so its batches (and with them the gradients' reduction layout and the counters) depend on arrival times: its
arrays are compared where the parent's own processes agree and listed as not reproducible where they do not.
Timing: median and [min, max] of 40 calls after 5 warm-up calls at three shapes.  Acceptance (fixed before the runs): every new
median lies inside the parents' own [min, max] over all parent processes, or below it — host code cannot move kernel time, so the
parent's own spread is the margin."""
import os
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

NB = 128
REPS, WARMUP = 40, 5
TIMED = ((144, 64, False), (144, 64, True), (2048, 512, False))          # n, P, gradient
THREADED = "threaded/"


def run(label, out_path):
    import torch
    import __graft_entry__ as g
    import _sweep_cases as CASES
    pkg = g.load_package()
    G = pkg
    out = {}

    def put(name, vals):
        for i, v in enumerate(vals if isinstance(vals, (tuple, list)) else (vals,)):
            if isinstance(v, (list, tuple)):          # per-particle gradients
                v = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in v]) if len(v) else np.zeros(0)
            out[f"{name}/{i}"] = np.asarray(v)

    def counters(eng, name):
        vals = [int(eng.lag_stats()[0]), eng.lag_stats()[1], eng.lag_rank_sweeps(), *eng.compact_stats().values(), eng.toeplitz_particles(),
                eng.grad_lag_domain_particles(), eng.grad_toeplitz_particles(), eng.grad_structured_particles(),
                *eng.grad_reuse_stats().values(), *eng.extend_stats().values(), *eng.eval_stats().values(), *eng.dedup_stats()]
        out[f"{name}/counters"] = np.array(vals, dtype=np.int64)

    def both_limits(eng, name, n, grad, call, before=None):
        nt = -(-n // NB)
        for tag, lim in (("ws_default", 0), ("ws_3", 3 * (2 if grad else 1) * (nt * (nt + 1) // 2) * NB * NB * 8)):
            if before:
                before()
            eng.set_workspace_limit(lim if n > 0 else 0)
            put(f"{name}/{tag}", call())
            counters(eng, f"{name}/{tag}")
        eng.set_workspace_limit(0)

    def engine(ts, xs, env=None, lag_level=None):
        env = env or {}
        for k, v in env.items():
            os.environ[k] = str(v)
        try:
            eng = pkg.GPEngine(0)
        finally:
            for k in env:
                del os.environ[k]
        if lag_level is not None:
            eng.set_lag_tables(lag_level)
        eng.set_data(ts, xs)
        return eng

    def value(eng, nodes, nz, n=None):
        return lambda: eng.logpdf_batch(nodes, nz, n=n, check=False)

    def gradient(eng, nodes, nz, n=None):
        return lambda: eng.logpdf_grad_batch(nodes, nz, n=n, check=False)

    def irregular(n, seed):
        rng = np.random.default_rng(seed)
        return np.sort(rng.random(n)), 0.5 * rng.standard_normal(n)

    covered, elementwise, n_poly = CASES.grad_shapes(G)
    shapes = covered + elementwise
    shape_nz = np.linspace(0.02, 0.3, len(shapes))
    pop8, pop8_nz = pkg.prior.sample_particles(np.random.default_rng(8), 8, max_depth=3)

    # ---- plain value sweeps (general evaluator), n = 0, the device-output entry ----
    for n in (129, 300):
        ts, xs = irregular(n, n)
        eng = engine(ts, xs)
        both_limits(eng, f"value_plain_{n}", n, False, value(eng, pop8, pop8_nz))
        eng.close()
    ts, xs = irregular(129, 129)
    eng = engine(ts, xs)
    both_limits(eng, "value_n0", 0, False, value(eng, pop8, pop8_nz, n=0))
    both_limits(eng, "grad_n0", 0, True, gradient(eng, pop8, pop8_nz, n=0))

    def device_call():
        d_lp = torch.zeros(8, dtype=torch.float64, device="cuda:0")
        d_info = torch.zeros(8, dtype=torch.int32, device="cuda:0")
        eng.logpdf_batch_device(pkg.encode_batch(pop8), pop8_nz, 129, d_lp.data_ptr(), d_info.data_ptr(), torch.cuda.current_stream().cuda_stream)
        eng.wait()
        torch.cuda.synchronize()
        return d_lp.cpu().numpy(), d_info.cpu().numpy()
    both_limits(eng, "value_device_129", 129, False, device_call)

    # ---- gradient sweeps, n = 129: the launch classes by tree size, a ChangePoint tree, both sides of the fork threshold ----
    SE, PER, GE, LIN = G.SquaredExponential, G.Periodic, G.GammaExponential, G.Linear
    small = SE(0.3, 0.8) * PER(0.7, 0.21, 1.1) + GE(0.4, 1.3, 0.6)                                     # 5 nodes
    mid = small + SE(0.1, 0.5) * LIN(0.3, 0.2, 0.7) + G.Constant(0.4) * PER(0.5, 0.3, 0.9)           # 13 nodes
    big = mid + (SE(0.2, 0.6) + GE(0.3, 1.1, 0.4)) * (PER(0.4, 0.25, 0.8) + G.WhiteNoise(0.05))       # 21 nodes
    cp = G.ChangePoint(SE(0.3, 0.8), PER(0.7, 0.21, 1.1), 0.5, 0.05) + GE(0.4, 1.3, 0.6)
    trees = [small, mid, big, cp, LIN(0.3, 0.2, 0.7), big * SE(0.5, 1.0)]
    trees_nz = np.linspace(0.03, 0.2, len(trees))
    both_limits(eng, "grad_tree_sizes_129", 129, True, gradient(eng, trees, trees_nz))
    pop172, pop172_nz = pkg.prior.sample_particles(np.random.default_rng(172), 172, max_depth=-1, max_size=31)      # 3 tiles x 172 >= 512
    both_limits(eng, "grad_forked_129", 129, True, gradient(eng, pop172, pop172_nz))

    # ---- profiling: which timing slots a value and a gradient sweep fill ----
    eng.set_profiling(True)
    eng.logpdf_batch(pop8, pop8_nz, check=False)
    out["profiling/value_slots"] = np.array(list(eng.timing().values())) != 0
    eng.logpdf_grad_batch(trees, trees_nz, check=False)
    out["profiling/grad_slots"] = np.array(list(eng.timing().values())) != 0
    eng.set_profiling(False)
    eng.close()

    # ---- sorted lag-table sweep on a whole regular grid, with a particle that is not positive definite (the sorted-order repeat) ----
    ts, xs = pkg.prior.synthetic_series(256, seed=11, shuffle=True)
    bad, bad_nz = CASES.non_positive_definite_pair(G)
    eng = engine(ts, xs)
    both_limits(eng, "value_sorted_lag_256", 256, False, value(eng, bad + pop8, np.concatenate([bad_nz, pop8_nz])))
    eng.close()

    # ---- rank-table sweeps: a prefix of a shuffled grid (value and gradient), the same with the switch off ----
    ts, xs = pkg.prior.synthetic_series(300, seed=600, shuffle=True)
    eng = engine(ts, xs)
    both_limits(eng, "value_rank_prefix_129", 129, False, value(eng, pop8, pop8_nz, n=129))
    both_limits(eng, "grad_rank_prefix_129", 129, True, gradient(eng, shapes, shape_nz, n=129))
    eng.set_lag_rank_tables(False)
    both_limits(eng, "value_rank_off_129", 129, False, value(eng, pop8, pop8_nz, n=129))
    eng.close()

    # ---- calendar series: rank tables over a lattice with gaps, compact tables whole in LDS, per-tile windows on the sorted sweep ----
    for freq, n in (("B", 400), ("M", 400), ("M", 1100)):
        ts, xs = CASES.calendar_series(pkg, freq, n, seed=n, shuffle=True)
        eng = engine(ts, xs)
        both_limits(eng, f"calendar_{freq}_{n}/value", n, False, value(eng, pop8 + bad, np.concatenate([pop8_nz, bad_nz])))
        m = (2 * n) // 3
        both_limits(eng, f"calendar_{freq}_{n}/prefix", m, False, value(eng, pop8, pop8_nz, n=m))
        both_limits(eng, f"calendar_{freq}_{n}/grad", n, True, gradient(eng, shapes[:8] + elementwise, np.linspace(0.02, 0.3, 8 + len(elementwise))))
        eng.close()

    # ---- structured value sweep (AGP_LAG = 2, 3): whole series, a prefix in time order, a refused particle ----
    ts, xs = pkg.prior.synthetic_series(300, seed=15, shuffle=True)
    order = np.argsort(ts)
    refused = [SE(5.0, 1.0), SE(0.1, 1.0) + LIN(0.2, 0.1, 1.0), LIN(0.3, 0.2, 0.5)]
    refused_nz = np.array([0.0, 0.05, 0.1])
    for level in (2, 3):
        eng = engine(ts, xs, lag_level=level)
        both_limits(eng, f"structured_value_L{level}/whole_300", 300, False, value(eng, shapes, shape_nz))
        eng.close()
        eng = engine(ts[order], xs[order], lag_level=level)
        both_limits(eng, f"structured_value_L{level}/prefix_250", 250, False, value(eng, shapes, shape_nz, n=250))
        eng.close()
        t2, x2 = pkg.prior.synthetic_series(256, seed=11, shuffle=True)
        eng = engine(t2, x2, lag_level=level)
        both_limits(eng, f"structured_value_L{level}/refused_256", 256, False, value(eng, refused, refused_nz))
        eng.close()
    # (level 2 asks whether the class pays: a prior-sampled population at n = 2048)
    t2, x2 = pkg.prior.synthetic_series(2048, seed=13, shuffle=True)
    pop160, pop160_nz = pkg.prior.sample_particles(np.random.default_rng(31), 160, max_depth=-1, max_size=31)
    eng = engine(t2, x2, lag_level=2)
    both_limits(eng, "structured_value_L2/population_2048", 2048, False, value(eng, pop160, pop160_nz))
    eng.close()

    # ---- gradient sweeps in the lag domain: histograms, spectrum, Toeplitz solves (with a rejected downdate: the repeat), the
    # structured split, the polynomial class ----
    grad_pop = shapes + [CASES.dominated_linear(G)]
    grad_nz = np.linspace(0.02, 0.3, len(grad_pop))
    ts, xs = pkg.prior.synthetic_series(300, seed=377, shuffle=True)
    t6, x6 = pkg.prior.synthetic_series(600, seed=5, shuffle=False)
    for lagdom in (1, 2):
        for fft in (0, 1, 2, 3, 4):
            env = {"AGP_GRAD_LAGDOM": lagdom, "AGP_GRAD_FFT": fft}
            eng = engine(ts, xs, env)
            both_limits(eng, f"grad_lagdom{lagdom}_fft{fft}/whole_300", 300, True, gradient(eng, grad_pop, grad_nz))
            both_limits(eng, f"grad_lagdom{lagdom}_fft{fft}/prefix_250", 250, True, gradient(eng, grad_pop, grad_nz, n=250))
            eng.close()
            eng = engine(t6, x6, env)
            both_limits(eng, f"grad_lagdom{lagdom}_fft{fft}/time_order_400", 400, True, gradient(eng, grad_pop, grad_nz, n=400))
            eng.close()
    # (the power spectrum serves sweeps of more than ~1000 points; the structured split on its own heuristic at n = 2048)
    t11, x11 = pkg.prior.synthetic_series(1100, seed=1100, shuffle=True)
    eng = engine(t11, x11, {"AGP_GRAD_FFT": 1})
    both_limits(eng, "grad_spectrum_1100", 1100, True, gradient(eng, grad_pop, grad_nz))
    eng.close()
    eng = engine(t2, x2, {"AGP_GRAD_FFT": 3})
    both_limits(eng, "grad_structured_population_2048", 2048, True, gradient(eng, pop160, pop160_nz))
    eng.close()

    # ---- gradient after a value call that left factors in the store: some particles resident, in one chunk and in two ----
    for n, (ts, xs) in ((129, pkg.prior.synthetic_series(129, seed=37, shuffle=True)), (300, irregular(300, 301))):
        eng = engine(ts, xs)
        eng.logpdf_batch_extend(pop8[:5], pop8_nz[:5], check=False)
        both_limits(eng, f"grad_store_hits_{n}", n, True, gradient(eng, pop8, pop8_nz))
        eng.close()
    # ... with the Toeplitz class beside resident factors (the structured split's residency lookup)
    ts, xs = pkg.prior.synthetic_series(384, seed=6, shuffle=True)
    for lag_level in (None, 3):
        eng = engine(ts, xs, {"AGP_GRAD_FFT": 4}, lag_level=lag_level)
        eng.logpdf_batch_extend(shapes[:2] + shapes[6:8], np.concatenate([shape_nz[:2], shape_nz[6:8]]), check=False)
        both_limits(eng, f"grad_structured_store_L{lag_level}_384", 384, True, gradient(eng, shapes, shape_nz))
        eng.close()

    # ---- class-aware coalesced mode (AGP_LAG >= 2, single-particle entries from threads): value calls, then gradient calls ----
    T = 24
    ts, xs = pkg.prior.synthetic_series(300, seed=77, shuffle=True)
    tn, tn_nz = pkg.prior.sample_particles(np.random.default_rng(12), T, max_depth=3, max_size=15)
    eng = engine(ts, xs, {"AGP_GRAD_FFT": 4}, lag_level=3)
    eng.extend_reserve(300, 2 * T)

    def phase(fn):
        res = [None] * T
        def work(i):
            res[i] = fn(tn[i], float(tn_nz[i]), check=False)
        th = [threading.Thread(target=work, args=(i,)) for i in range(T)]
        for t in th: t.start()
        for t in th: t.join()
        return res
    for step in range(2):
        out[f"{THREADED}class_aware_300/value/{step}"] = np.array(phase(eng.logpdf))
        gr = phase(eng.logpdf_grad)
        out[f"{THREADED}class_aware_300/grad_lp/{step}"] = np.array([r[0] for r in gr])
        out[f"{THREADED}class_aware_300/grad/{step}"] = np.concatenate([np.append(np.asarray(r[1], dtype=np.float64).reshape(-1), r[2]) for r in gr])
        counters(eng, f"{THREADED}class_aware_300/{step}")
    eng.close()

    # ---- end-to-end time of the batch entries ----
    def timed(name, call):
        for _ in range(WARMUP):
            call()
        t = np.empty(REPS)
        for i in range(REPS):
            t0 = time.perf_counter(); call(); t[i] = time.perf_counter() - t0
        out[f"time/{name}"] = t * 1e3
        print(f"[{label}] {name}: median {np.median(t) * 1e3:.3f} ms [{t.min() * 1e3:.3f}, {t.max() * 1e3:.3f}]", flush=True)

    for n, P, grad in TIMED:
        ts, xs = pkg.prior.synthetic_series(n, seed=n, shuffle=True)
        nodes, nz = pkg.prior.sample_particles(np.random.default_rng(n + P), P, max_depth=-1, max_size=31)
        eng = engine(ts, xs)
        call = gradient(eng, nodes, nz) if grad else value(eng, nodes, nz)
        name = f"{'grad' if grad else 'value'}_{n}_{P}"
        put(f"timed/{name}", call())
        timed(name, call)
        eng.close()

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out_path, **out)
    print(f"[{label}] {sum(not k.startswith('time/') for k in out)} arrays -> {out_path}", flush=True)


def compare(paths):
    runs = [dict(np.load(p)) for p in paths]
    parents, news = runs[0::2], runs[1::2]
    keys = sorted(k for k in runs[0] if not k.startswith("time/"))

    def equal(a, b):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # (threads: only what the parent's own processes reproduce can be compared)
    loose = [k for k in keys if k.startswith(THREADED) and not all(equal(parents[0][k], r[k]) for r in parents[1:])]
    strict = [k for k in keys if k not in loose]
    bad = []
    for r, p in zip(runs[1:], paths[1:]):
        if sorted(k for k in r if not k.startswith("time/")) != keys:
            bad.append((p, "different set of arrays"))
            continue
        for k in strict:
            if not equal(runs[0][k], r[k]):
                bad.append((p, k))
    print(f"bit comparison: {len(strict)} arrays and counter vectors in {len(runs)} processes ({len(parents)} parent, {len(news)} new): "
          + ("ALL BIT-IDENTICAL" if not bad else f"{len(bad)} DIFFER"))
    for p, k in bad:
        print("  differs:", p, k)
    for k in loose:
        worst = max(float(np.max(np.abs(r[k].astype(np.float64) - runs[0][k].astype(np.float64)), initial=0.0)) for r in runs[1:])
        print(f"  not reproducible between the parent's own processes (thread arrival), not compared: {k}  (largest difference over all processes {worst:.3e})")
    ok = not bad
    print("end-to-end batch entries, ms: median [min, max] of %d calls after %d warm-up calls, per process" % (REPS, WARMUP))
    for k in sorted(k for k in runs[0] if k.startswith("time/")):
        lo = min(r[k].min() for r in parents); hi = max(r[k].max() for r in parents)
        print(f"  {k[5:]}   (parents' range [{lo:.3f}, {hi:.3f}])")
        for p, r in zip(paths, runs):
            t = r[k]
            print(f"    {Path(p).stem:>12}: {np.median(t):9.3f} [{t.min():9.3f}, {t.max():9.3f}]")
        for r in news:
            med = float(np.median(r[k]))
            verdict = "below" if med < lo else "inside" if med <= hi else "ABOVE"
            print(f"    new median {med:.3f}: {verdict} the parents' range")
            ok = ok and med <= hi
    print("verdict:", "PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare" and len(sys.argv) % 2 == 0:
        sys.exit(compare(sys.argv[2:]))
    else:
        sys.exit(__doc__)
