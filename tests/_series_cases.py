"""Cases shared by the tests of the short-series kernel's factorisation (tests/test_gpu_series_probe.py, tests/test_gpu_series.py
and their CPU twins in tests/test_factor_ref_cpu.py, tests/test_series_cpu.py): sizes, matrices with a known first bad pivot,
particles that fail at a chosen point of a 176-point series, and particles whose covariance is exact in float64.  Plain NumPy."""
import numpy as np

import _factor_ref as R

# every block count nb = ceil(n / 16) = 1 .. 11 both full and ragged; n >= 81 reaches the second pass of the panel loop (two blocks
# per wave and pass: rows jb + 1 + w + 8 ..), nb = 11 every trailing-triangle size of the three-pairs-per-pass loop
SIZES = (1, 5, 16, 17, 33, 48, 49, 80, 81, 97, 112, 127, 129, 144, 145, 161, 176)
N_CAP = 176
# every 4-wide sub-step of block 0, both sides of the block boundaries 16, 32, 80 and 160, the last pivot
INFO_PIVOTS = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 79, 80, 159, 160, 175)
# first failing leading minor k + 1 of changepoint_particle(k)
CP_POINTS = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 159, 160, 175)


def info_probes():
    """[(K, expected LAPACK info, name)]: matrices that are not positive definite from a known pivot on"""
    out = [(R.indefinite(N_CAP, [j]), j + 1, f"indefinite({N_CAP}, [{j}])") for j in INFO_PIVOTS]
    out += [(R.indefinite(N_CAP, [128, 40]), 41, f"indefinite({N_CAP}, [128, 40])"),
            (R.indefinite(N_CAP, [16, 17]), 17, f"indefinite({N_CAP}, [16, 17])")]
    out += [(R.zero_pivot(N_CAP, j), j + 1, f"zero_pivot({N_CAP}, {j})") for j in (0, 16, 160)]
    # the only real row of a ragged block; padding rows are never reported
    out += [(R.indefinite(161, [160]), 161, "indefinite(161, [160])"), (R.zero_pivot(161, 160), 161, "zero_pivot(161, 160)")]
    out += [(R.indefinite(1, [0]), 1, "indefinite(1, [0])")]
    return out


def first_bad_minor(K):
    """1-based order of the first leading minor LAPACK cannot factor, None when K is positive definite"""
    for k in range(1, K.shape[0] + 1):
        try:
            np.linalg.cholesky(K[:k, :k])
        except np.linalg.LinAlgError:
            return k
    return None


CP_TS = np.linspace(0.0, 1.0, N_CAP)
CP_NOISE = -0.5


def changepoint_particle(G, k):
    """With noise CP_NOISE on CP_TS: diagonal 0.5 before point k and -0.499 from k on (the ChangePoint switches half a grid step
    before ts[k], 28 scales away from either neighbour: sigma is 0 or 1 to rounding) -> the first failing leading minor is k + 1"""
    return G.ChangePoint(G.WhiteNoise(1.0), G.Constant(1e-3), CP_TS[k] - 0.5 / (N_CAP - 1), 1e-4)


def exact_particles(G, n):
    """(ts, [(node, noise)]): every entry of K + noise I is a sum and product of dyadic numbers that fits 53 bits, whatever the order
    of evaluation (times are multiples of 2^-8 below 1, parameters multiples of 2^-2)"""
    ts = np.arange(n) / 256.0
    return ts, [(G.Constant(0.5) + G.WhiteNoise(0.25), 0.25), (G.Linear(0.25, 0.5, 2.0), 0.25)]
