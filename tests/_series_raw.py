"""Raw ctypes calls of the four many-series entries that take per-series transforms or mixture weights — the band
(agp_predict_quantile_series_batch), the held-out scores (agp_predict_logpdf_series_batch), the samples
(agp_predict_sample_series_batch) and the decompositions (agp_predict_sum_series_batch) — on one small family, every output
pre-filled with a sentinel and one element longer than the entry may write: what tests/test_gpu_series_errors.py and
tools/gpu_series_host_ab.py make their refused calls with."""
import ctypes as C
import sys

import numpy as np

ENTRIES = ("band", "held_out", "sample", "sum")
TAKES_INTERCEPT = ("band", "sample", "sum")        # (the held-out entry takes slopes only: the caller has scaled the values)
TAKES_WEIGHTS = ("band", "held_out", "sample")
JOINT = ("held_out", "sample")                     # factor training and query points together: the joint cap applies
FILL = -7
R_SAMPLES = 3
Q_BAND = (0.1, 0.5, 0.9)


def family(pkg, lengths=(5, 7, 9), m=2, per_series=2):
    """series of `lengths` points, m query points each, per_series particles per series, single-leaf kernels; valid as it stands"""
    leafs = [pkg.SquaredExponential(0.3, 0.5), pkg.Linear(0.2, 0.4, 0.6), pkg.Periodic(0.5, 0.3, 0.7), pkg.Constant(0.4),
             pkg.GammaExponential(0.42, 0.58, 1.2), pkg.SquaredExponential(0.47, 0.9)]
    series, queries, heldout = [], [], []
    for s, n in enumerate(lengths):
        ts, xs = pkg.prior.synthetic_series(256, seed=40 + s, shuffle=True)
        series.append((ts[:n].copy(), xs[:n].copy()))
        queries.append(np.linspace(1.02, 1.1, m) + 0.01 * s)
        heldout.append(np.linspace(-0.2, 0.3, m))
    S, P = len(lengths), len(lengths) * per_series
    return dict(series=series, queries=queries, heldout=heldout, nodes=[leafs[p % len(leafs)] for p in range(P)],
                noises=np.linspace(0.1, 0.2, P), sidx=np.repeat(np.arange(S, dtype=np.int32), per_series),
                w=np.full(P, 1.0 / per_series), yts=np.array([(2.0, 0.3), (-0.5, -1.25), (1.5, 0.0)] * S)[:S])


def with_yts(fam, s, k, v):
    """the family with series s's slope (k = 0) or intercept (k = 1) replaced by v"""
    y = np.array(fam["yts"]); y[s, k] = v
    return dict(fam, yts=y)


def with_bad_weights(fam, s):
    """the family with series s's weights summing to 1.1"""
    w = fam["w"].copy(); w[np.flatnonzero(fam["sidx"] == s)[0]] += 0.1
    return dict(fam, w=w)


def over_joint_cap(pkg, fam):
    """series 1 replaced by 170 training and 10 query points: each allowed alone, together 180"""
    ts, xs = pkg.prior.synthetic_series(256, seed=1, shuffle=True)
    return dict(fam, series=[fam["series"][0], (ts[:170], xs[:170])] + fam["series"][2:],
                queries=[fam["queries"][0], np.linspace(1.0, 1.2, 10)] + fam["queries"][2:],
                heldout=[fam["heldout"][0], np.linspace(-0.2, 0.3, 10)] + fam["heldout"][2:])


def refused_cases(pkg, fam):
    """every refused call of tests/test_gpu_series_errors.py: (name, entries, family)"""
    return [("zero_slope", ENTRIES, with_yts(fam, 1, 0, 0.0)),
            ("nan_intercept", TAKES_INTERCEPT, with_yts(fam, 2, 1, np.nan)),
            ("inf_intercept", TAKES_INTERCEPT, with_yts(fam, 2, 1, np.inf)),
            ("weights", TAKES_WEIGHTS, with_bad_weights(fam, 1)),
            ("joint_cap", JOINT, over_joint_cap(pkg, fam)),
            ("weights0_slope1", TAKES_WEIGHTS, with_yts(with_bad_weights(fam, 0), 1, 0, 0.0)),
            ("slope0_weights1", TAKES_WEIGHTS, with_yts(with_bad_weights(fam, 1), 0, 0, 0.0))]


def call(pkg, engine, entry, a, fill=FILL):
    """the entry's C function on the family `a`: (rc, message, {name: flat output})"""
    E = sys.modules[pkg.__name__ + ".engine"]
    lib, ctx = engine._lib, engine._ctx
    S, P = len(a["series"]), len(a["nodes"])
    packed = pkg.series_call_args(a["series"], a["nodes"], a["noises"], a["sidx"])
    qpack = pkg.pack_queries(a["queries"], S, None, P)
    s = E._series_ctypes(packed, qpack)
    Q = int(qpack[0][-1])
    n_out = sum(len(a["queries"][i]) for i in a["sidx"])
    yt = np.asarray(a["yts"], dtype=np.float64)
    sl, ic = E._dp(np.ascontiguousarray(yt[:, 0])), E._dp(np.ascontiguousarray(yt[:, 1]))
    w = E._dp(np.ascontiguousarray(a["w"], dtype=np.float64))
    f64 = lambda n: np.full(n + 1, float(fill))
    i32 = lambda n: np.full(n + 1, fill, dtype=np.int32)
    i64 = lambda n: np.full(n + 1, fill, dtype=np.int64)
    p64 = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_int64))
    o = {"logpdf": f64(P), "info": i32(P)}
    if entry == "band":
        q = np.array(Q_BAND)
        o.update(x=f64(q.size * Q), conv=i32(q.size * Q), iters=i32(q.size * Q), mean=f64(Q), var=f64(Q))
        rc = lib.agp_predict_quantile_series_batch(ctx, *s, w, sl, ic, E._dp(q), q.size, 1e-5, 10 ** 6, E._dp(o["x"]), E._ip(o["conv"]),
                                                   E._ip(o["iters"]), E._dp(o["mean"]), E._dp(o["var"]), E._dp(o["logpdf"]), E._ip(o["info"]))
    elif entry == "held_out":
        y = np.ascontiguousarray(np.concatenate(a["heldout"]), dtype=np.float64)
        o.update(terms=f64(n_out), out_off=i64(P + 1), series_logp=f64(S))
        rc = lib.agp_predict_logpdf_series_batch(ctx, *s[:6], E._dp(y), *s[6:], sl, w, E._dp(o["logpdf"]), E._dp(o["terms"]),
                                                 p64(o["out_off"]), E._dp(o["series_logp"]), E._ip(o["info"]))
    elif entry == "sample":
        R = R_SAMPLES
        seeds = np.arange(S, dtype=np.uint64)
        del o["logpdf"]
        o.update(x=f64(R * Q), component=i32(S * R), mean=f64(n_out), out_off=i64(P + 1),
                 cov=f64(sum(len(a["queries"][i]) ** 2 for i in a["sidx"])), cov_off=i64(P + 1))
        rc = lib.agp_predict_sample_series_batch(ctx, *s, sl, ic, w, R, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), None, None,
                                                 E._dp(o["x"]), E._ip(o["component"]), E._dp(o["mean"]), p64(o["out_off"]), E._dp(o["cov"]),
                                                 p64(o["cov_off"]), E._ip(o["info"]))
    elif entry == "sum":                               # M = 1: every particle's kernel is its one component
        q = np.array(Q_BAND)
        o.update(mean=f64(2 * n_out), var=f64(2 * n_out), x=f64(2 * n_out * q.size), out_off=i64(P + 1))
        rc = lib.agp_predict_sum_series_batch(ctx, *s[:7], 1, *s[7:], sl, ic, E._dp(q), q.size, E._dp(o["mean"]), E._dp(o["var"]),
                                              E._dp(o["x"]), p64(o["out_off"]), E._dp(o["logpdf"]), E._ip(o["info"]))
    else:
        raise ValueError(entry)
    return rc, lib.agp_last_error(ctx).decode(), o


def touched(o, fill=FILL):
    """the names of the outputs in which an element differs from the sentinel"""
    return [name for name, out in o.items() if not (out == fill).all()]
