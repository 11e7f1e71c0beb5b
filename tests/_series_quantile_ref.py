"""TEST INFRASTRUCTURE of agp_predict_quantile_series_batch (forecast bands of many short series): a NumPy restatement of the ragged
layout its read-out kernels index with (csrc/agp_series.hip quant_plan, csrc/agp_series_quantile_kernel.hpp) — the per-series particle
lists, the padded weight and row offsets, the wave -> (series, query, quantile) decode of the search kernel and the thread -> (series,
query) decode of the moments kernel — and the shared band case of tests/test_series_quantile_cpu.py and
tests/test_gpu_series_quantile.py: tests/_series_predict_ref.ragged_case() with per-series weights, transforms and the oracle's raw
components."""
import functools

import numpy as np

import _series_predict_ref as P

QS = (0.025, 0.5, 0.975)


def ragged_layout(series_index, S, m_s):
    """quant_plan's tables: lists[s] (ascending particle indexes), pl_off, w_off (rows padded to Pp_s = ceil(P_s / 64) 64) and row_off
    (series s owns m_s rows of Pp_s entries), each of S + 1 int64."""
    sidx = np.asarray(series_index, dtype=np.int64)
    lists = [np.flatnonzero(sidx == s) for s in range(S)]
    P_s = np.array([len(l) for l in lists], dtype=np.int64)
    Pp = (P_s + 63) // 64 * 64
    z = np.zeros(1, dtype=np.int64)
    pl_off = np.concatenate([z, np.cumsum(P_s)])
    w_off = np.concatenate([z, np.cumsum(Pp)])
    row_off = np.concatenate([z, np.cumsum(np.asarray(m_s, dtype=np.int64) * Pp)])
    return lists, pl_off, w_off, row_off


def series_of(off, scale, g):
    """the kernels' binary search: the largest s with off[s] * scale <= g (g below off[S] * scale)"""
    lo, hi = 0, len(off) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if off[mid] * scale <= g:
            lo = mid
        else:
            hi = mid
    return lo


def decode_wave(wid, q_off, nq):
    """k_series_mix_quantile: wave wid of nq q_off[S] -> (s, i, k); its output slot is wid itself (series s's (nq, m_s) row-major
    block starts at nq q_off[s])"""
    s = series_of(q_off, nq, wid)
    m = int(q_off[s + 1] - q_off[s])
    local = wid - int(q_off[s]) * nq
    return s, local % m, local // m


def decode_thread(g, q_off):
    """k_series_mix_moments: thread g of q_off[S] -> (s, i)"""
    s = series_of(q_off, 1, g)
    return s, g - int(q_off[s])


def row_span(s, i, w_off, row_off):
    """[start, end) of the packed row of (series s, query i)"""
    Pp = int(w_off[s + 1] - w_off[s])
    return int(row_off[s]) + i * Pp, int(row_off[s]) + (i + 1) * Pp


@functools.lru_cache(maxsize=None)
def band_case():
    """The shared band case: ragged_case() (ten series of 0 .. 176 points, 5, 0, 1, 15, 16, 17, 33, 12, 36, 65 queries, six particles
    each) with per-series weights from default_rng(7) (the second particle's set to 0 before normalising), transforms a_s = 0.5 +
    0.4 s, b_s = -1 + 0.3 s, and the ORACLE's raw components per series.
    Returns dict(series, queries, nodes, noises, sidx, weights (P,), yt (S, 2), q, raw_mean / raw_var (lists of (6, m_s) arrays))."""
    import __graft_entry__ as g
    pkg = g.load_package()
    series, queries, nodes, noises, sidx, ref_mean, ref_var = P.ragged_case()
    S = len(series)
    rng = np.random.default_rng(7)
    weights = np.zeros(len(nodes))
    for s in range(S):
        sel = np.flatnonzero(sidx == s)
        w = rng.random(len(sel))
        w[1] = 0.0
        weights[sel] = w / w.sum()
    yt = np.array([[0.5 + 0.4 * s, -1.0 + 0.3 * s] for s in range(S)])
    raw_mean, raw_var = [], []
    for s in range(S):
        sel = np.flatnonzero(sidx == s)
        mo = np.stack([ref_mean[i] for i in sel]); vo = np.stack([ref_var[i] for i in sel])
        mr, vr, info = pkg.raw_components(mo, vo, np.zeros(len(sel), np.int32), len(series[s][0]), tuple(yt[s]))
        assert (info == 0).all()
        mr.setflags(write=False); vr.setflags(write=False)
        raw_mean.append(mr); raw_var.append(vr)
    weights.setflags(write=False); yt.setflags(write=False)
    return dict(series=series, queries=queries, nodes=nodes, noises=noises, sidx=sidx, weights=weights, yt=yt, q=np.array(QS),
                raw_mean=raw_mean, raw_var=raw_var)
