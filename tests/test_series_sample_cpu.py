"""CPU tests of the index algebra behind agp_predict_sample_series_batch's read-out (tests/_series_sample_ref.py): from a LAPACK
factor of a joint matrix, the restated lane maps, masks, passes, CSR lists and transform must reproduce the dense
x = (mu* + sign(a) L22 z - b) / a, (mu* - b) / a and Sigma* / a^2 for every train / query split n mod 16 in {0, 1, 15} at every block
count 1 .. 11 of the joint points.  Tolerance: the restatement sums the same products in another order, in fp64 — 1e-12 relative to
the largest magnitude of the reference (condition numbers here are below 1e4).  NaN sits above the diagonal of every packed diagonal
block: a read that is not masked shows as NaN."""
import numpy as np
import pytest

import _series_sample_ref as R

TOL = 1e-12


def joint_case(n, m, seed):
    rng = np.random.default_rng(seed)
    N = n + m
    t = np.sort(rng.random(N))
    K = np.exp(-0.5 * ((t[:, None] - t[None, :]) / 0.2) ** 2) + 0.3 * np.eye(N)
    L = np.linalg.cholesky(K)
    xs = rng.standard_normal(n)
    a = np.linalg.solve(L[:n, :n], xs) if n else np.zeros(0)
    avec = np.concatenate([a, rng.standard_normal(16 * ((N + 15) // 16) - n)])      # the query rows' entries are never read
    return L, avec, L[n:, :n] @ a, L[n:, n:] @ L[n:, n:].T


def shapes():
    out = []
    for nb in range(1, 12):
        for split in (0, 1, 15):
            N = 16 * nb - (0 if nb % 2 else 3)          # full and ragged last blocks
            n = max(k for k in range(N) if k % 16 == split)
            if nb > 2:
                n = min(n, 16 * (nb // 2) + split)      # several query blocks where there is room
            if nb >= 9:
                n = split                               # ... more than six of them: a second pass over the row blocks (0: the prior)
            out.append((n, N - n))
    return out


def test_shapes_cover_every_block_count_and_split():
    sh = shapes()
    assert {(n + m + 15) // 16 for n, m in sh} == set(range(1, 12))
    assert {((n + m + 15) // 16, n % 16) for n, m in sh} == {(nb, s) for nb in range(1, 12) for s in (0, 1, 15)}
    assert all(m >= 1 and n + m <= 176 for n, m in sh)
    assert max(m for _, m in sh) > 96                    # a second pass over the row blocks


@pytest.mark.parametrize("n,m", shapes())
def test_readout_matches_dense(n, m):
    L, avec, mu, Sigma = joint_case(n, m, 1000 * n + m)
    rng = np.random.default_rng(n + 7 * m)
    Rn = 21                                              # two groups, the second with five samples
    z = rng.standard_normal((m, Rn))
    comp = rng.integers(0, 3, Rn)                        # three particles share the factor here; only the lists differ
    comp[comp == 1] = 0                                  # ... particle 1 has no sample
    lists = R.csr(comp, 3)
    assert lists[1].size == 0
    sm = R.pack_blocks(L)
    for slope, icpt in ((2.5, -0.75), (-0.4, 1.5)):
        ref = R.dense(mu, Sigma, z, slope, icpt)
        scale = max(1.0, np.abs(ref).max())
        seen = set()
        for p in range(3):
            x, mean, cov = R.readout(sm, avec, n, m, lists[p], z, slope, icpt)
            assert sorted(x) == list(lists[p])
            for j, col in x.items():
                assert np.isfinite(col).all() and np.abs(col - ref[:, j]).max() <= TOL * scale, (n, m, p, j)
                seen.add(j)
            assert np.abs(mean - (mu - icpt) / slope).max() <= TOL * max(1.0, np.abs(mu / slope).max())
            assert np.array_equal(cov, cov.T) and np.isfinite(cov).all()
            assert np.linalg.norm(cov - Sigma / slope ** 2) <= TOL * np.linalg.norm(Sigma / slope ** 2)
        assert seen == set(range(Rn))


def test_flat_layout_of_a_two_series_batch():
    """two series (m = 5 and 18; three and two particles, interleaved in the batch) through readout() and assemble(): the flat out_x,
    out_mean and out_cov hold the dense results at R q_off[s] + j m_s + i, out_off[p] + i and cov_off[p] + c m + r"""
    shapes_, sidx, Rn = ((20, 5), (3, 18)), np.array([0, 1, 0, 1, 0]), 7
    m_s = [m for _, m in shapes_]
    x_off, out_off, cov_off = R.layout(m_s, sidx, Rn)
    assert x_off.tolist() == [0, 35, 161] and out_off.tolist() == [0, 5, 23, 28, 46, 51]
    assert cov_off.tolist() == [0, 25, 349, 374, 698, 723]
    rng = np.random.default_rng(9)
    cases = [joint_case(n, m, 77 + n) for n, m in shapes_]
    zs = [rng.standard_normal((m, Rn)) for m in m_s]
    comp = [np.array([0, 2, 4, 0, 0, 2, 4]), np.array([1, 1, 3, 1, 3, 3, 1])]          # global particle indices
    yts = [(2.5, -0.75), (-0.4, 1.5)]
    results = []
    for p, s in enumerate(sidx):
        L, avec, mu, Sigma = cases[s]
        results.append(R.readout(R.pack_blocks(L), avec, shapes_[s][0], m_s[s], np.flatnonzero(comp[s] == p), zs[s], *yts[s]))
    ox, om, oc = R.assemble(m_s, sidx, Rn, results)
    assert np.isfinite(ox).all() and np.isfinite(om).all() and np.isfinite(oc).all()      # every element is owned by someone
    for s in range(2):
        L, avec, mu, Sigma = cases[s]
        ref = R.dense(mu, Sigma, zs[s], *yts[s])
        m = m_s[s]
        for j in range(Rn):
            for i in range(m):
                assert abs(ox[Rn * sum(m_s[:s]) + j * m + i] - ref[i, j]) <= TOL * max(1.0, np.abs(ref).max())
    for p, s in enumerate(sidx):
        L, avec, mu, Sigma = cases[s]
        a, b = yts[s]
        m = m_s[s]
        assert np.abs(om[out_off[p]:out_off[p] + m] - (mu - b) / a).max() <= TOL * max(1.0, np.abs(mu / a).max())
        for c in (0, m - 1):
            for r_ in (0, 1, m - 1):
                assert abs(oc[cov_off[p] + c * m + r_] - Sigma[r_, c] / a ** 2) <= TOL * np.abs(Sigma / a ** 2).max()


def test_draws_are_the_resident_entrys_per_series():
    """series s draws under seeds[s] what tests/_pred_sample_ref.py draws under that seed: components by the inverse CDF of the
    series' own weights, z[i, j] from word i % 4 of block (i / 4, j, 1, 0)"""
    import _pred_sample_ref as PS
    w = np.array([0.25, 0.0, 0.75])
    comp, z = R.draws(12345, w, 7, 9)
    assert np.array_equal(comp, PS.components(12345, w, 9)) and not (comp == 1).any()
    assert np.array_equal(z, PS.normals(12345, 7, range(9)))
    assert z[5, 3] == PS.normals(12345, 8, [3])[5, 0]    # the normal of (i, j) does not depend on m or on the other samples
