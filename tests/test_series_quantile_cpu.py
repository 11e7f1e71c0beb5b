"""CPU tests of agp_predict_quantile_series_batch's host side: the ragged layout of the read-out kernels covers every (series, query,
quantile) exactly once without overlapping rows; the shared band case converges everywhere with every decision margin above delta(6)
on the oracle's components (so the GPU comparison may demand every point bit for bit); pack_series_mixture."""
import numpy as np
import pytest

import _mixture_quantile_ref as MQ
import _series_quantile_ref as R


@pytest.mark.parametrize("nq", [1, 3])
def test_layout_covers_every_triple_once(nq):
    # particles per series 0, 1, 63, 64, 65, 130, 2, 5; a series without queries among those with particles and among those without
    P_s = [0, 1, 63, 64, 65, 130, 2, 0, 5]
    m_s = [4, 3, 2, 1, 0, 2, 7, 0, 16]
    S = len(P_s)
    rng = np.random.default_rng(3)
    sidx = rng.permutation(np.repeat(np.arange(S), P_s))          # a series' particles interleaved with the others'
    lists, pl_off, w_off, row_off = R.ragged_layout(sidx, S, m_s)
    q_off = np.concatenate([[0], np.cumsum(m_s)])
    for s in range(S):
        assert len(lists[s]) == P_s[s] and (np.diff(lists[s]) > 0).all() and (sidx[lists[s]] == s).all()
        Pp = w_off[s + 1] - w_off[s]
        assert Pp % 64 == 0 and P_s[s] <= Pp < P_s[s] + 64 and (Pp == 0) == (P_s[s] == 0)
        assert row_off[s + 1] - row_off[s] == m_s[s] * Pp
    assert np.array_equal(np.sort(np.concatenate(lists)), np.arange(len(sidx)))
    # every (s, i, k) from exactly one wave, whose output slot is its own index inside the series' (nq, m_s) block
    seen = {}
    for wid in range(nq * int(q_off[-1])):
        s, i, k = R.decode_wave(wid, q_off, nq)
        assert 0 <= i < m_s[s] and 0 <= k < nq
        assert wid == nq * q_off[s] + k * m_s[s] + i
        assert (s, i, k) not in seen
        seen[(s, i, k)] = wid
    assert len(seen) == nq * sum(m_s)
    assert [R.decode_thread(g, q_off) for g in range(int(q_off[-1]))] == [(s, i) for s in range(S) for i in range(m_s[s])]
    # the packed rows tile [0, row_off[S]) without gaps or overlaps
    spans = sorted(R.row_span(s, i, w_off, row_off) for s in range(S) for i in range(m_s[s]) if P_s[s] > 0)
    assert spans[0][0] == 0 and spans[-1][1] == row_off[-1]
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("tol", [1e-5, 1e-10])
def test_band_case_is_in_class_everywhere(tol):
    c = R.band_case()
    assert [len(q) for q in c["queries"]] == [5, 0, 1, 15, 16, 17, 33, 12, 36, 65]
    d = MQ.delta(6)
    worst_it, vmin = 0, np.inf
    for s in range(len(c["series"])):
        sel = np.flatnonzero(c["sidx"] == s)
        w = c["weights"][sel]
        assert len(sel) == 6 and w[1] == 0.0 and abs(w.sum() - 1.0) < 1e-15
        if c["raw_var"][s].size:
            vmin = min(vmin, c["raw_var"][s].min())
        for qk in c["q"]:
            b = MQ.quantile_search(c["raw_mean"][s], c["raw_var"][s], w, qk, tol=tol)
            assert b["converged"].all(), (s, qk)
            assert (b["margin"] > d).all(), (s, qk, b["margin"].min(), d)
            worst_it = max(worst_it, int(b["iters"].max()) if b["iters"].size else 0)
    print(f"[series-quantile] tol {tol:g}: every point converged in <= {worst_it} iterations, every margin > delta(6) = {d:.3e}; "
          f"smallest raw variance {vmin:.3e}")
    assert vmin > 0.0


def test_pack_series_mixture(pkg):
    sidx = np.array([2, 0, 2, 2, 0], dtype=np.int32)
    lw = np.array([0.3, -1.0, 700.0, 701.0, 2.0])
    lists, w = pkg.pack_series_mixture(sidx, 4, log_weights=lw)
    assert [l.tolist() for l in lists] == [[1, 4], [], [0, 2, 3], []]
    for sel in lists:
        if len(sel):
            e = np.exp(lw[sel] - lw[sel].max())
            assert np.array_equal(w[sel], e / e.sum()) and abs(w[sel].sum() - 1.0) < 1e-15
    assert np.isfinite(w).all() and w[0] < 1e-300            # (the shift keeps exp(701) from overflowing)
    given = np.array([0.5, 0.25, 0.5, 0.0, 0.75])
    lists2, w2 = pkg.pack_series_mixture(sidx, 4, weights=given)
    assert np.array_equal(w2, given) and all(np.array_equal(a, b) for a, b in zip(lists, lists2))
    lists0, w0 = pkg.pack_series_mixture(np.zeros(0, dtype=np.int32), 2, weights=np.zeros(0))
    assert [l.size for l in lists0] == [0, 0] and w0.size == 0
    for kw in (dict(), dict(weights=given, log_weights=lw), dict(weights=given[:4]), dict(log_weights=np.zeros((5, 1)))):
        with pytest.raises(ValueError):
            pkg.pack_series_mixture(sidx, 4, **kw)
    with pytest.raises(ValueError):
        pkg.pack_series_mixture(sidx, 2, weights=given)      # a series index outside [0, S)
    with pytest.raises(ValueError):
        pkg.pack_series_mixture(np.zeros((5, 1), dtype=np.int32), 4, weights=given)
