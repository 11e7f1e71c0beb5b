"""Restatement of agp_predict_sample_batch's random draws (include/autogp_hip.h) on numpy.random.Philox, an independent Philox4x64-10:
uniforms, the component inverse CDF and the normals z = ndtri(u) through scipy.special.ndtri."""
import numpy as np
from scipy.special import ndtri

MASK64 = (1 << 64) - 1


def philox_block(seed, c0, c1, c2, c3):
    """The 4 words of counter (c0, c1, c2, c3) under the key (seed, 0).  numpy advances its counter before the first block it
    returns, so block c is Philox(counter=c - 1).random_raw(4)."""
    v = (c0 + (c1 << 64) + (c2 << 128) + (c3 << 192) - 1) % (1 << 256)
    ctr = np.array([(v >> (64 * i)) & MASK64 for i in range(4)], dtype=np.uint64)
    g = np.random.Philox(key=np.array([seed & MASK64, 0], dtype=np.uint64), counter=ctr)
    return [int(w) for w in g.random_raw(4)]


def uniform(w):
    u = (float(int(w) >> 11) + 0.5) * 2.0 ** -53
    return u if u < 1.0 else 1.0 - 2.0 ** -53


def components(seed, weights, S):
    """Inverse CDF over the fp64 cumulative weights in particle order: the first p with u < cum[p], else the last positive weight."""
    w = np.asarray(weights, dtype=np.float64)
    cum = np.empty_like(w)
    acc = 0.0
    for p in range(w.shape[0]):
        acc += w[p]
        cum[p] = acc
    last = int(np.nonzero(w > 0)[0][-1])
    out = np.empty(S, dtype=np.int32)
    for s in range(S):
        u = uniform(philox_block(seed, s, 0, 0, 0)[0])
        k = int(np.searchsorted(cum, u, side="right"))
        out[s] = last if k >= w.shape[0] else k
    return out


def normals(seed, m, samples):
    """z[:, j] for the sample indices `samples`: word i % 4 of block (i / 4, s, 1, 0), through scipy's ndtri; shape (m, len)."""
    z = np.empty((m, len(samples)))
    for j, s in enumerate(samples):
        for i4 in range((m + 3) // 4):
            b = philox_block(seed, i4, int(s), 1, 0)
            for r in range(4):
                if 4 * i4 + r < m:
                    z[4 * i4 + r, j] = ndtri(uniform(b[r]))
    return z
