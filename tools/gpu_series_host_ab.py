"""A/B of two builds of the library over the host side of the many-series entries (csrc/agp_series.hip): every output array, every
refusal (return code and message) and the set of non-zero agp_get_timing slots of a fixed, seeded list of calls must be
BIT-IDENTICAL, and the entries must not get slower end to end.  The C ABI is the same on both sides, so one Python layer drives
either library through AUTOGP_HIP_LIB.

    AUTOGP_HIP_LIB=<library> python tools/gpu_series_host_ab.py run <label> <out.npz>      one fresh process per run
    python tools/gpu_series_host_ab.py compare <parent.npz> <new.npz> <parent.npz> <new.npz> ...

Run the processes alternating parent / new / parent / new.  The calls: all nine entries on a ragged family of four series (one
empty) under two assignments of eight particles of mixed depth, one of them not positive definite — one assignment leaves a series
without particles; weights, terms and moments wanted and not; caller-given component and z; calls that launch nothing; P == 0;
profiling on; the long entry under a workspace limit that forces several launches; the refused calls of
tests/test_gpu_series_errors.py and one null-pointer call per entry.  A call that raises is recorded as its message.  Timing: median
and [min, max] of 40 calls after 5 warm-up calls per entry, at 64 series x 126 points x 8 particles x 12 queries and at one such
series.  Acceptance (fixed before the runs): every new median lies inside the parents' own [min, max] over all parent processes, or
below it — host code cannot move kernel time, so the parent's own spread is the margin."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

REPS, WARMUP = 40, 5
ENTRY_SYMBOLS = ("agp_logpdf_series_batch", "agp_logpdf_long_series_batch", "agp_logpdf_grad_series_batch", "agp_hmc_series_batch",
                 "agp_predict_series_batch", "agp_predict_quantile_series_batch", "agp_predict_logpdf_series_batch",
                 "agp_predict_sample_series_batch", "agp_predict_sum_series_batch")
LONG_TRIANGLE_442 = 28 * 29 // 2 * 256 * 8      # bytes of one factor of a 442-point series: 28 block rows of 16


def flatten(name, v, out):
    """every array reachable from a call's result, under a name of its own"""
    if isinstance(v, np.ndarray):
        out[name] = v
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            flatten(f"{name}/{i}", x, out)
    elif hasattr(v, "__dict__"):
        for k, x in sorted(vars(v).items()):
            flatten(f"{name}/{k}", x, out)


def entry_calls(pkg, eng, fam, tf):
    """name -> call, for all nine entries and their option variants on one family"""
    series, queries, heldout, nodes, noises, sidx, w, yts = (fam[k] for k in ("series", "queries", "heldout", "nodes", "noises", "sidx", "w", "yts"))
    S, P = len(series), len(nodes)
    cls = [pkg.prior.hmc_classes(nd) for nd in nodes]
    z = [np.where(k >= 0, 0.1, 0.05) for k in cls]
    split = [[nd, pkg.Linear(0.1, 0.2, 0.3)] for nd in nodes]
    m_s = [len(q) for q in queries]
    R = 5
    rng = np.random.default_rng(11)
    comp = np.zeros((S, R), dtype=np.int32)             # every sample from the series' first particle (0 where it has none: refused)
    for s in range(S):
        comp[s, :] = np.flatnonzero((sidx == s) & (w > 0))[:1].sum()
    zz = [rng.standard_normal((m, R)) for m in m_s]
    kw = dict(check=False)
    return {
        "value": lambda: eng.logpdf_series_batch(series, nodes, noises, sidx, **kw),
        "long": lambda: eng.logpdf_long_series_batch(series, nodes, noises, sidx, **kw),
        "long_all": lambda: eng.logpdf_long_series_batch(series, nodes, noises, sidx, all_long=True, **kw),
        "grad": lambda: eng.logpdf_grad_series_batch(series, nodes, noises, sidx, **kw),
        "hmc": lambda: eng.hmc_series_batch(series, nodes, z, np.full(P, -2.0), cls, tf, sidx, 3, np.arange(P), L_param=3, L_noise=3,
                                            want_trace=True, **kw),
        "predict": lambda: eng.predict_series_batch(series, queries, nodes, noises, sidx, want_logpdf=True, **kw),
        "predict_noise_pred": lambda: eng.predict_series_batch(series, queries, nodes, noises, sidx, noise_pred=np.full(P, 0.05), **kw),
        "band": lambda: eng.predict_quantile_series_batch(series, queries, nodes, noises, sidx, w, [0.1, 0.5, 0.9], y_transforms=yts, **kw),
        "band_moments": lambda: eng.predict_quantile_series_batch(series, queries, nodes, noises, sidx, w, 0.5, want_moments=True,
                                                                  want_logpdf=True, **kw),
        "held_out": lambda: eng.predict_logpdf_series_batch(series, queries, heldout, nodes, noises, sidx, **kw),
        "held_out_weights_terms": lambda: eng.predict_logpdf_series_batch(series, queries, heldout, nodes, noises, sidx, weights=w,
                                                                          y_transforms=yts, want_terms=True, **kw),
        "sample": lambda: eng.predict_sample_series_batch(series, queries, nodes, noises, sidx, w, R, y_transforms=yts, **kw),
        "sample_moments": lambda: eng.predict_sample_series_batch(series, queries, nodes, noises, sidx, w, R, seeds=np.arange(S) + 9,
                                                                  want_moments=True, **kw),
        "sample_component_z": lambda: eng.predict_sample_series_batch(series, queries, nodes, noises, sidx, w, R, component=comp, z=zz,
                                                                      want_moments=True, **kw),
        "sample_R0": lambda: eng.predict_sample_series_batch(series, queries, nodes, noises, sidx, w, 0, want_moments=True, **kw),
        "sum": lambda: eng.predict_sum_series_batch(series, queries, split, noises, sidx, q=[0.05, 0.95], y_transforms=yts,
                                                    want_var=True, want_logpdf=True, **kw),
        "sum_no_q": lambda: eng.predict_sum_series_batch(series, queries, split, noises, sidx, **kw),
    }


def ragged_family(pkg, sidx, lengths=(20, 0, 45, 100), m_s=(3, 2, 4, 5), bad=True):
    rng = np.random.default_rng(2026)
    series, queries, heldout = [], [], []
    for s, (n, m) in enumerate(zip(lengths, m_s)):
        ts, xs = pkg.prior.synthetic_series(256, seed=70 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        queries.append(np.sort(rng.random(m) * 1.3 - 0.1))
        heldout.append(rng.standard_normal(m) * 0.3)
    sidx = np.asarray(sidx, dtype=np.int32)
    P = sidx.shape[0]
    nodes, noises = [], np.zeros(P)
    for p in range(P):                                  # depths 1 .. 4 in turn
        nd, nz = pkg.prior.sample_particles(rng, 1, max_depth=4, min_depth=1 + p % 4)
        nodes.append(nd[0]); noises[p] = nz[0]
    if bad and P:
        chain = pkg.GammaExponential(0.42, 0.58, 1.2)   # right-nested ChangePoints: an evaluation stack of 5, the depth-8 kernels
        for k, leaf in enumerate((pkg.Constant(0.4), pkg.Periodic(0.5, 0.3, 0.7), pkg.Linear(0.2, 0.4, 0.6), pkg.SquaredExponential(0.3, 0.5))):
            chain = pkg.ChangePoint(leaf, chain, 0.65 - 0.15 * k, 0.05)
        nodes[0] = chain
        nodes[-1] = pkg.Constant(1.0); noises[-1] = -0.5      # not positive definite (tests/test_gpu_series.py)
    w = pkg.pack_series_mixture(sidx, len(lengths), log_weights=rng.standard_normal(P))[1] if P else np.zeros(0)
    yts = np.array([(2.0, 0.3), (-0.5, -1.25), (1.5, 0.0), (0.7, 2.0)])[:len(lengths)]
    return dict(series=series, queries=queries, heldout=heldout, nodes=nodes, noises=noises, sidx=sidx, w=w, yts=yts)


def run(label, out_path):
    import __graft_entry__ as g
    import _series_raw as RAW
    pkg = g.load_package()
    tf = np.array(json.loads((ROOT / "tests" / "golden" / "series_hmc_v1.json").read_text())["tf"])
    eng = pkg.GPEngine(0)
    out, raised = {}, 0

    def record(name, call):
        nonlocal raised
        try:
            found = {}
            flatten(name, call(), found)
            assert found, name
            out.update(found)
        except Exception as e:      # a refusal (or the Python layer's own ValueError): its text is the result
            raised += 1
            out[f"{name}/raised"] = np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8)

    families = {"no_particle_series": ragged_family(pkg, [0, 0, 1, 1, 3, 3, 3, 3]), "all_series": ragged_family(pkg, [0, 0, 1, 2, 2, 3, 3, 3]),
                "nothing_launched": ragged_family(pkg, [1, 1, 1], m_s=(3, 0, 4, 5), bad=False),
                "P0": ragged_family(pkg, [])}
    for fname, fam in families.items():
        for name, call in entry_calls(pkg, eng, fam, tf).items():
            record(f"{fname}/{name}", call)
    # profiling: which slots of agp_get_timing an entry fills
    eng.set_profiling(True)
    for name, call in entry_calls(pkg, eng, families["all_series"], tf).items():
        record(f"profiled/{name}", call)
        out[f"profiled/{name}/slots"] = np.array([v != 0.0 for v in eng.timing().values()])
    eng.set_profiling(False)
    # the long entry: 6 long particles under a workspace limit of two factors — several launches
    rng = np.random.default_rng(5)
    ts, xs = pkg.prior.synthetic_series(442, seed=3, shuffle=True)
    lseries = [(ts, xs), (ts[:300].copy(), xs[:300].copy()), (ts[:100].copy(), xs[:100].copy())]
    lnodes, lnz = pkg.prior.sample_particles(rng, 9, max_depth=3)
    lsidx = [0, 0, 0, 0, 1, 1, 2, 2, 0]
    for tag, lim in (("ws_default", 0), ("ws_2", 2 * LONG_TRIANGLE_442)):
        eng.set_workspace_limit(lim)
        record(f"long_442/{tag}", lambda: eng.logpdf_long_series_batch(lseries, lnodes, lnz, lsidx, check=False))
        record(f"long_442_all/{tag}", lambda: eng.logpdf_long_series_batch(lseries, lnodes, lnz, lsidx, all_long=True, check=False))
    eng.set_workspace_limit(0)
    # refusals: (rc, message, every sentinel-filled output)
    fam = RAW.family(pkg)
    for cname, entries, a in RAW.refused_cases(pkg, fam):
        for entry in entries:
            rc, msg, o = RAW.call(pkg, eng, entry, a)
            out[f"refused/{cname}/{entry}/rc_message"] = np.frombuffer(f"{rc}: {msg}".encode(), dtype=np.uint8)
            flatten(f"refused/{cname}/{entry}", [o[k] for k in sorted(o)], out)
    # one null-pointer call per entry: every pointer null, every size 1
    for sym in ENTRY_SYMBOLS:
        fn = getattr(eng._lib, sym)
        args = [1 if t in (C.c_int32, C.c_int64) else 1.0 if t is C.c_double else None for t in fn.argtypes[1:]]
        rc = fn(eng._ctx, *args)
        out[f"null/{sym}"] = np.frombuffer(f"{rc}: {eng._lib.agp_last_error(eng._ctx).decode()}".encode(), dtype=np.uint8)

    # ---- end-to-end time per entry ----
    timed = ("value", "long", "grad", "hmc", "predict", "band", "held_out_weights_terms", "sample", "sum")
    for S in (64, 1):
        sidx = np.repeat(np.arange(S), 8)
        fam = ragged_family(pkg, sidx, lengths=(126,) * S, m_s=(12,) * S, bad=False)
        fam["yts"] = np.tile([(2.0, 0.3)], (S, 1))
        calls = entry_calls(pkg, eng, fam, tf)
        for name in timed:
            call = calls[name]
            for _ in range(WARMUP):
                call()
            t = np.empty(REPS)
            for i in range(REPS):
                t0 = time.perf_counter(); call(); t[i] = time.perf_counter() - t0
            out[f"time/{name}_{S}x126x8x12"] = t * 1e3
            print(f"[{label}] {name} {S}x126x8x12: median {np.median(t) * 1e3:.3f} ms [{t.min() * 1e3:.3f}, {t.max() * 1e3:.3f}]", flush=True)
    eng.close()
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out_path, **out)
    n_msg = sum(k.endswith(("/raised", "/rc_message")) or k.startswith("null/") for k in out)
    print(f"[{label}] {sum(not k.startswith('time/') for k in out)} arrays ({n_msg} of them messages, {raised} from calls that raised) "
          f"-> {out_path}", flush=True)
    for k in sorted(out):
        if k.endswith(("/raised", "/rc_message")) or k.startswith("null/"):
            print(f"[{label}]   {k}: {out[k].tobytes().decode()}")


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
    print(f"bit comparison: {len(keys)} arrays and messages in {len(runs)} processes ({len(parents)} parent, {len(news)} new): "
          + ("ALL BIT-IDENTICAL" if not bad else f"{len(bad)} DIFFER"))
    for p, k in bad:
        print("  differs:", p, k)
    ok = not bad
    print("end to end per entry, ms: median [min, max] of %d calls after %d warm-up calls, per process" % (REPS, WARMUP))
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
