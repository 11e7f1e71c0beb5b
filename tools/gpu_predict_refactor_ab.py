"""A/B of two builds of the library over the dense predictive pass (csrc/agp_predict.hip predict_core / predict_logpdf_core and the
entries behind them): every output array and counter of a fixed, seeded list of calls must be BIT-IDENTICAL, and end-to-end
agp_predict_batch must not get slower.  The C ABI is the same on both sides, so one Python layer drives either library through
AUTOGP_HIP_LIB.

    AUTOGP_HIP_LIB=<library> python tools/gpu_predict_refactor_ab.py run <label> <out.npz>      one fresh process per run
    python tools/gpu_predict_refactor_ab.py compare <parent.npz> <new.npz> <parent.npz> <new.npz> ...

Run the processes alternating parent / new / parent / new.  The calls reuse tests/_predict_cases.py, so each route has a name; each
case runs with the default workspace and limited to three particles per chunk.  Timing: median and [min, max] of 40 calls after 5
warm-up calls at three shapes.  Acceptance (fixed before the runs): every new median lies inside the parents' own [min, max] over all
parent processes, or below it — host code cannot move kernel time, so the parent's own spread is the margin."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

NB = 128
CORE_CASES = ("joint_17", "joint_129", "joint_300", "joint_means_129", "joint_noise_pred_17", "train_route_300", "train_route_below_300",
              "lattice_grid_300", "population_300")
TIMED = ("population_300", "train_route_300")
LARGE = (2048, 512, 64)          # n : future points : particles, of tools/gpu_predict_perf.py's defaults
REPS, WARMUP = 40, 5


def joint_bytes(ts_train, tq, split_allowed):
    """bytes per particle of a pass's matrices, (strideA + strideZ) * 8: the joint matrix keeps every query unless the training-point
    route applies (agp_predict.hip split_queries)"""
    n, m = ts_train.shape[0], tq.shape[0]
    dups = int(np.isin(tq, ts_train).sum())
    split = split_allowed and n >= 2 * NB and m >= NB and dups >= NB and 3 * dups >= n
    nt1 = -(-n // NB); nt = nt1 + -(-((m - dups) if split else m) // NB)
    tiles = nt * (nt + 1) // 2 + (nt1 * (nt1 + 1) // 2 if split else 0)
    return tiles * NB * NB * 8


def run(label, out_path):
    import __graft_entry__ as g
    import _predict_cases as PCASES
    pkg = g.load_package()
    out = {}

    def put(name, vals):
        for i, v in enumerate(vals if isinstance(vals, (tuple, list)) else (vals,)):
            if isinstance(v, np.ndarray):
                out[f"{name}/{i}"] = v

    def counters(eng, name):
        r = eng.predict_reuse_stats()
        out[f"{name}/counters"] = np.array([r["reused"], r["factored"], eng.lag_predict_passes(), *eng.dedup_stats(),
                                            eng.predict_structured_particles()], dtype=np.int64)

    def both_limits(eng, name, nbytes, call):
        for tag, lim in (("ws_default", 0), ("ws_3", 3 * nbytes)):
            eng.set_workspace_limit(lim)
            put(f"{name}/{tag}", call())
            counters(eng, f"{name}/{tag}")
        eng.set_workspace_limit(0)

    def engine_for(case):
        eng = pkg.GPEngine(0)
        eng.set_data(case.ts, case.xs)
        return eng

    def predict(eng, case):
        return eng.predict_batch(case.nodes, case.noises, case.tq, n=case.n, noise_pred=case.noise_pred, want_cov=case.want_cov,
                                 check=False, **case.means_kw)

    for name in CORE_CASES:
        case = PCASES.case(name)
        eng = engine_for(case)
        both_limits(eng, name, joint_bytes(case.ts[:case.n], case.tq, not case.want_cov), lambda: predict(eng, case))
        eng.close()

    # resident factors on a prefix, then resident Z on the longer prefix (the training-point route from resident factors), twice:
    # the second pass finds every column of Z in the store
    short, full = PCASES.case("resident_prefix_200"), PCASES.case("train_route_300")
    eng = engine_for(full)
    for case, steps in ((short, 1), (full, 2)):
        eng.logpdf_batch_extend(case.nodes, case.noises, n=case.n, check=False)
        for k in range(steps):
            both_limits(eng, f"resident/{case.name}/{k}", joint_bytes(case.ts[:case.n], case.tq, True), lambda: predict(eng, case))
    eng.close()

    rng = np.random.default_rng(2024)
    for name in ("joint_129", "lattice_grid_300"):
        case = PCASES.case(name)
        eng = engine_for(case)
        y = PCASES.signal(case.tq, rng)
        w = rng.random(len(case.nodes)); w /= w.sum()
        nbytes = joint_bytes(case.ts[:case.n], case.tq, False)
        both_limits(eng, f"logpdf/{name}", nbytes, lambda: eng.predict_logpdf_batch(case.nodes, case.noises, case.tq, y, n=case.n, check=False))
        both_limits(eng, f"sample/{name}", nbytes, lambda: eng.predict_sample_batch(case.nodes, case.noises, case.tq, w, 16, seed=5,
                                                                                   n=case.n, check=False))
        eng.close()

    case = PCASES.case("joint_129")
    eng = engine_for(case)
    w = rng.random(len(case.nodes)); w /= w.sum()
    nbytes = joint_bytes(case.ts[:case.n], case.tq, False)
    both_limits(eng, "mixture_cov/joint_129", nbytes, lambda: eng.predict_mixture_batch(case.nodes, case.noises, case.tq, w, n=case.n,
                                                                                        want_cov=True, check=False))
    # sum-of-GPs entries, M = 2 components per particle; two duplicated particles in the batched calls
    splits = [list(pkg.split_kernel_sop(nd, pkg.Linear)) for nd in case.nodes]
    assert all(len(s) == 2 for s in splits)
    noises = np.maximum(case.noises, 1e-3)
    tp = np.linspace(-0.1, 1.2, 40)
    idx = list(range(len(splits))) + [2, 5]
    sp2 = [splits[i] for i in idx]; nz2 = noises[idx]
    nbytes = joint_bytes(case.ts[:case.n], np.tile(tp, 3), False)
    both_limits(eng, "infer_gp_sum/joint_129", nbytes, lambda: eng.infer_gp_sum(splits[2], noises[2], tp, n=case.n, check=False)[:2])
    both_limits(eng, "infer_gp_sum_batch/joint_129", nbytes, lambda: eng.infer_gp_sum_batch(sp2, nz2, tp, n=case.n, want_cov=True, check=False)[:4])
    both_limits(eng, "predict_sum_batch/joint_129", nbytes, lambda: eng.predict_sum_batch(sp2, nz2, tp, q=[0.05, 0.5, 0.95], n=case.n,
                                                                                          y_transform=(2.0, 0.3), check=False))
    eng.close()

    # ---- end-to-end time of agp_predict_batch ----
    def timed(name, eng, call):
        for _ in range(WARMUP):
            call()
        t = np.empty(REPS)
        for i in range(REPS):
            t0 = time.perf_counter(); call(); t[i] = time.perf_counter() - t0
        out[f"time/{name}"] = t * 1e3
        print(f"[{label}] {name}: median {np.median(t) * 1e3:.3f} ms [{t.min() * 1e3:.3f}, {t.max() * 1e3:.3f}]", flush=True)

    for name in TIMED:
        case = PCASES.case(name)
        eng = engine_for(case)
        timed(name, eng, lambda: predict(eng, case))
        eng.close()
    n, extra, P = LARGE
    ts, xs = pkg.prior.synthetic_series(n, seed=n, shuffle=True)
    gs = np.sort(ts); h = (gs[-1] - gs[0]) / (n - 1)
    tp = np.concatenate([ts, gs[0] + h * np.arange(n, n + extra)])
    nodes, nz = pkg.prior.sample_particles(np.random.default_rng(n + P), P, max_depth=-1, max_size=31)
    eng = pkg.GPEngine(0)
    eng.set_data(ts, xs)
    put("large", eng.predict_batch(nodes, nz, tp, check=False))
    timed(f"large_{n}_{extra}_{P}", eng, lambda: eng.predict_batch(nodes, nz, tp, check=False))
    eng.close()

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out_path, **out)
    print(f"[{label}] {sum(not k.startswith('time/') for k in out)} arrays -> {out_path}", flush=True)


def compare(paths):
    runs = [dict(np.load(p)) for p in paths]
    parents, news = runs[0::2], runs[1::2]
    keys = sorted(k for k in runs[0] if not k.startswith("time/"))
    bad = []
    for r, p in zip(runs[1:], paths[1:]):
        if sorted(k for k in r if not k.startswith("time/")) != keys:
            bad.append((p, "different set of arrays"))
            continue
        for k in keys:
            a, b = runs[0][k], r[k]
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                bad.append((p, k))
    print(f"bit comparison: {len(keys)} arrays and counter vectors in {len(runs)} processes ({len(parents)} parent, {len(news)} new): "
          + ("ALL BIT-IDENTICAL" if not bad else f"{len(bad)} DIFFER"))
    for p, k in bad:
        print("  differs:", p, k)
    ok = not bad
    print("end-to-end agp_predict_batch, ms: median [min, max] of %d calls after %d warm-up calls, per process" % (REPS, WARMUP))
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
