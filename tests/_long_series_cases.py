"""Cases shared by the tests of the long-series kernel's block Cholesky (tests/test_gpu_long_series_probe.py and its CPU twin
tests/test_long_series_probe_cpu.py): sizes, the matrices of each size with their right-hand sides and reference caps, matrices with
a known first bad pivot, and particles whose covariance is exact in float64.  Plain NumPy.

The kernel (csrc/agp_long_series_kernel.hpp) factors left-looking by 16-wide block columns; wave w owns the block rows ib >= j with
ib % 4 == w, C of them, and stage (b) has one loop body per C = 1 .. 8 (C = c first runs at n = 64 (c - 1) + 17):
   1         one ragged block, three waves idle
  16, 17     a full block; the first long_update, whose one-step chain prefetches its own operands again
  65         a fifth block row (a wave with two rows, no update of the second yet)
  81         the first C = 2
 177         the first size the short kernel cannot take
 337         C = 6, the last prefetching body
 401         C = 7, the first body without the prefetch
 465         C = 8
 497         32 block rows, one real row in the last block
 512         the cap"""
import numpy as np

import _factor_ref as R

SIZES = (1, 16, 17, 65, 81, 177, 337, 401, 465, 497, 512)
N_CAP = 512
NINE_UP_TO = 177      # the batch of nine up to here, its first five members (one per family) above
# both sides of the boundaries of block 0's 4-wide sub-steps, of blocks, of the four waves' round (64) and of the short kernel's
# cap; the first and last pivot of the last block row
INFO_PIVOTS = (0, 3, 4, 15, 16, 63, 64, 176, 177, 255, 256, 383, 384, 447, 448, 495, 496, 511)

_CACHE = {}


def batch(n):
    """(labels, K, y, kappa_blk) of size n: the batch of nine of tests/_factor_ref.py up to n = 177, its first five members above;
    computed once per size (the longdouble reference factors behind kappa_blk are what costs), never modified."""
    if n not in _CACHE:
        nine = R.batch_of_nine(n)
        if n > NINE_UP_TO:
            nine = nine[:len(R.FAMILIES)]
        K = np.stack([k for _, k in nine]); K.setflags(write=False)
        y = np.ascontiguousarray(R.batch_rhs(n)[:len(nine)]); y.setflags(write=False)
        kap = np.array([R.kappa_blk(R.ref_chol(k)) for k in K])
        _CACHE[n] = ([l for l, _ in nine], K, y, kap)
    return _CACHE[n]


# (kind, n, argument): matrices that are not positive definite from a known pivot on
INFO_SPECS = tuple(("indefinite", N_CAP, (j,)) for j in INFO_PIVOTS)
# the later pivot sits in a block row of a lower-numbered wave (block rows 17 and 2: waves 1 and 2): the first of the four waves'
# first bad pivots is the smallest, not wave 0's
INFO_SPECS += (("indefinite", N_CAP, (272, 40)), ("indefinite", N_CAP, (16, 17)))
INFO_SPECS += tuple(("zero_pivot", N_CAP, j) for j in (0, 64, 496))
# the only real row of a ragged block (padding rows are never reported), and the smallest matrix
INFO_SPECS += (("indefinite", 497, (496,)), ("zero_pivot", 497, 496), ("indefinite", 1, (0,)))


def info_name(spec):
    kind, n, arg = spec
    return f"{kind}({n}, {list(arg) if kind == 'indefinite' else arg})"


def info_probe(spec):
    """(K, expected LAPACK info) of one entry of INFO_SPECS"""
    kind, n, arg = spec
    if kind == "indefinite":
        return R.indefinite(n, list(arg)), min(arg) + 1
    return R.zero_pivot(n, arg), arg + 1


def exact_particles(G, n):
    """(ts, [(node, noise)]) for n <= 512: the particles of tests/_series_cases.py on times that are multiples of 2^-9 below 1 —
    every entry of K + noise I is a sum and product of dyadic numbers that fits 53 bits, whatever the order of evaluation"""
    assert 1 <= n <= N_CAP
    ts = np.arange(n) / 512.0
    return ts, [(G.Constant(0.5) + G.WhiteNoise(0.25), 0.25), (G.Linear(0.25, 0.5, 2.0), 0.25)]
