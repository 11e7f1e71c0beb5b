"""Host-side checks of remove_data (agp_remove_data): the NumPy restatement of the blocked factor update (tests/_chol_remove_ref.py)
against numpy.linalg.cholesky of the reduced matrix, the prefix bookkeeping of partially covered factors, OnlineStream.remove with
a fake evaluator, the Python layer's index validation (before any library call) and the declarations of the new entries."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _chol_remove_ref as R      # noqa: E402


def spd(n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 1, n))
    d = t[:, None] - t[None, :]
    K = 1.3 * np.exp(-0.5 * (d / 0.15) ** 2) + 0.4 * np.outer(t, t) + 0.05 * np.eye(n)
    x = rng.standard_normal(n)
    return K, x


def removals(n):
    """front, across a tile boundary, end, scattered — for every r that fits"""
    out = []
    for r in (1, 7, 128, 200):
        if r >= n:
            continue
        out.append(("front", list(range(r))))
        out.append(("end", list(range(n - r, n))))
        if n > 128:
            a = max(0, min(128 - r // 2 - 1, n - r))
            out.append(("boundary", list(range(a, a + r))))
        rng = np.random.default_rng(1000 * n + r)
        out.append(("scattered", sorted(rng.choice(n, size=r, replace=False).tolist())))
    return out


# the update is backward stable: |dL| ~ a modest multiple of eps |L| per reflector chain, far inside the project's parity tolerance
@pytest.mark.parametrize("n", [5, 129, 300, 517])
def test_reference_factor_matches_cholesky_of_reduced_matrix(n):
    K, x = spd(n, n)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L, x)
    for name, idx in removals(n):
        keep = np.setdiff1d(np.arange(n), idx)
        Lr = np.linalg.cholesky(K[np.ix_(keep, keep)])
        ar = np.linalg.solve(Lr, x[keep])
        Lu, au = R.remove_rows(L, alpha, idx)
        assert Lu.shape == Lr.shape, (n, name)
        assert (np.diag(Lu) > 0).all(), (n, name)
        assert np.array_equal(Lu, np.tril(Lu))
        assert np.abs(Lu - Lr).max() <= 1e-11 * max(1.0, np.abs(Lr).max()), (n, name, len(idx), np.abs(Lu - Lr).max())
        assert np.abs(au - ar).max() <= 1e-9 * max(1.0, np.abs(ar).max()), (n, name, len(idx), np.abs(au - ar).max())
        lp_u = -0.5 * (len(keep) * np.log(2 * np.pi) + 2 * np.log(np.diag(Lu)).sum() + au @ au)
        lp_r = -0.5 * (len(keep) * np.log(2 * np.pi) + 2 * np.log(np.diag(Lr)).sum() + ar @ ar)
        assert abs(lp_u - lp_r) <= 1e-8 * max(1.0, abs(lp_r)), (n, name, len(idx))


def test_narrow_passes_equal_one_wide_pass():
    K, x = spd(300, 3)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L, x)
    idx = list(range(40, 110))
    L1, a1 = R.remove_rows(L, alpha, idx, rmax=32)
    L2, a2 = R.remove_rows(L, alpha, idx, rmax=200)
    assert np.abs(L1 - L2).max() < 1e-12 and np.abs(a1 - a2).max() < 1e-10


def test_untouched_rows_are_bit_identical():
    K, x = spd(300, 4)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L, x)
    Lu, au = R.remove_rows(L, alpha, [200, 201, 250])
    assert np.array_equal(Lu[:200], L[:200, :297]) and np.array_equal(au[:200], alpha[:200])
    # the columns before the first removed position only move up
    assert np.array_equal(Lu[200:, :200], L[[i for i in range(200, 300) if i not in (200, 201, 250)], :200])


def test_runs_and_prefix_bookkeeping():
    assert R.runs_of([0]) == [(0, 1)]
    assert R.runs_of([3, 4, 5, 9, 20, 21]) == [(3, 3), (6, 1), (16, 2)]
    idx = [10, 11, 50, 300]
    assert R.touched_prefix(10, idx) == (False, 10)       # all removals at or beyond the prefix
    assert R.touched_prefix(11, idx) == (True, 10)
    assert R.touched_prefix(51, idx) == (True, 48)
    assert R.touched_prefix(300, idx) == (True, 297)      # position 300 lies beyond a prefix of 300 points
    assert R.touched_prefix(301, idx) == (True, 297)


class FakeEngine:
    def __init__(self, n):
        self.n_max = n
        self.calls = []

    def remove_data(self, indexes):
        self.calls.append(list(indexes))
        self.n_max -= len(indexes)
        return self.n_max


class FakeEvaluator:
    def __init__(self, engine):
        self.engine = engine
        self.seen = []

    def __call__(self, nodes, noises, n):
        self.seen.append(n)
        return -1.0 * n * np.ones(len(nodes)), np.zeros(len(nodes), dtype=np.int32)


def test_online_stream_remove(pkg):
    from autogp_jl_amd import stream
    eng = FakeEngine(50)
    ev = FakeEvaluator(eng)
    s = stream.OnlineStream([object()] * 4, np.full(4, 0.1), ev)
    s.step(50)
    st = s.remove([0, 1, 2])
    assert eng.calls == [[0, 1, 2]] and ev.seen == [50, 47] and st["n"] == 47 and not st["resampled"]
    assert np.allclose(s.prev_logpdf, -47.0) and np.allclose(s.log_weights, -47.0)
    with pytest.raises(RuntimeError):
        stream.OnlineStream([object()], np.ones(1), lambda nodes, noises, n: (np.zeros(1), np.zeros(1))).remove([0])


def test_index_validation_before_any_library_call(pkg):
    from autogp_jl_amd import engine as E
    assert E.check_remove_indexes([0, 3, 9], 10).dtype == np.int64
    for bad in ([], [3, 1], [1, 1], [-1, 2], [0, 10], [[0, 1]], [0.5, 1.5]):
        with pytest.raises(ValueError):
            E.check_remove_indexes(bad, 10)

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("the library must not be reached: " + name)

    eng = E.GPEngine.__new__(E.GPEngine)
    eng._lib = NoLib(); eng._ctx = None; eng.n_max = 10
    with pytest.raises(ValueError):
        eng.remove_data([4, 4])
    with pytest.raises(ValueError):
        eng.remove_data([])


def test_entries_declared_and_exported(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert re.search(r"int agp_remove_data\(agp_ctx\* ctx, const int64_t\* idx, int64_t k\);", hdr)
    assert re.search(r"int agp_get_remove_stats\(agp_ctx\* ctx, int64_t\* out, int32_t n_out\);", hdr)
    assert re.search(r"int agp_set_remove_update\(agp_ctx\* ctx, int32_t on\);", hdr)
    for s in ("agp_remove_data", "agp_get_remove_stats", "agp_set_remove_update", "agp_remove_data_multi"):
        assert s in pkg.EXPORTED_SYMBOLS, s
    for m in ("remove_data", "remove_stats", "set_remove_update"):
        assert hasattr(pkg.GPEngine, m), m
    assert hasattr(pkg.GPEngineMulti, "remove_data")
