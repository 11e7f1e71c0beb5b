"""The predictive checker (oracle/predcheck.py) checked on a machine without a GPU: an independent correct double-precision route —
the blocked 16 x 16 algorithm of tests/_series_predict_ref.py — passes it at mult = 8 on the whole family; three seeded faults that
the suite's old criterion |d| <= 1e-8 max(1, max|ref|) lets through are rejected; and the caps on R_mean and R_var hold for every
case of tests/test_gpu_predict_components.py (tests/_predict_cases.py).  Run with -s to see the ratios."""
import numpy as np
import pytest

import _predict_cases as PCS
import _series_predict_ref as R
from oracle import predcheck as PC

BLOCK_N = (17, 144, 176)


def block_case(n):
    """the series of the GPU suite's short-series cases with their references (shared, computed once): 17 irregular times with a
    duplicate, and prefixes of shuffled 256-point series as the short-series suite uses them.  (mult = 8 is no law for a correct
    route: on 176 irregular times — irregular_series(176, seed=476) — this route is 9.03 R_mean from the 80-bit mean of the
    ChangePoint at noise 1e-5 at one training-time query, with LAPACK's triangular inversion of the blocks 9.51; the dense pass of the
    device is 7.9 .. 13.3 R_mean from it on that particle.  R is the worst of three samples.)"""
    return PCS.case({17: "joint_17", 144: "series_144", 176: "series_176"}[n])


def blocked(c, i):
    return R.series_predict_blocks(c.nodes[i].to_tuple(), float(c.noises[i]), c.ts[:c.n], c.xs[:c.n], c.tq, noise_pred=float(c.noise_pred[i]))


@pytest.mark.parametrize("n", BLOCK_N)
def test_independent_correct_route_passes(n):
    c = block_case(n)
    refs = c.refs()
    worst = np.zeros(2)
    for i, r in enumerate(refs):
        mean, var = blocked(c, i)
        rm, rv, _ = PC.assert_predictive(mean, var, r, mult=8, ctx=("blocked", n, i, r.tree, r.noise))
        worst = np.maximum(worst, [rm, rv])
    print(f"[pred-components] blocked 16 x 16 route n={n}: worst distance / R: mean {worst[0]:.3f}, variance {worst[1]:.3f}"
          f" over {len(refs)} particles")


def gap_particles(c):
    """where small outputs live: the small-amplitude kernel at every noise, every kernel at noise 1e-5"""
    k = len(PCS.NOISES)
    return [i for i in range(len(c.nodes)) if i // k == PCS.SMALL_AMPLITUDE or c.noises[i] == 1e-5]


def rejected(mean, var, ref):
    try:
        PC.assert_predictive(mean, var, ref, mult=8)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("n", BLOCK_N)
def test_seeded_faults_are_rejected(n, monkeypatch):
    """Seed 1: one variance at a training-time query moved by 64 times its bound.  Seed 2: one mean moved by 64 times its bound.
    Seed 3: the K21 entry of the last real column (next to the padding wherever n is no multiple of 16) of one query perturbed by
    1e-9 before the solve.  Every seed is planted in every particle of gap_particles and must be rejected there.  The documented
    gap — the old criterion lets the fault through — is asserted where it exists: seeds 1 and 2 on the small-amplitude kernel at
    every noise, seed 1 on every noise 1e-5 particle, seed 2 on at least 8 of the 11 particles (a particle whose R is large, the
    lone Linear at noise 1e-5 with R_mean 1e-6, is checked by the old criterion almost as tightly as by the new one, and 64 times
    its mean's bound is seen by both), seed 3 on the small-amplitude kernel at noise 0.1 (see below: at noise 1e-5 the old criterion
    sees seed 3 as well)."""
    c = block_case(n)
    refs = c.refs()
    gap = PCS.SMALL_AMPLITUDE * len(PCS.NOISES)     # Constant(1e-4) * SE(0.2, 1.0) at noise 1e-5
    assert c.noises[gap] == 1e-5 and gap in gap_particles(c)
    j_train = 1                                     # a query on a training time (tq starts with every 7th training time)
    assert c.tq[j_train] in c.ts[:c.n]
    small = [i for i in gap_particles(c) if i // len(PCS.NOISES) == PCS.SMALL_AMPLITUDE]
    assert len(small) == len(PCS.NOISES) and gap in small
    n_old = 0
    for i in gap_particles(c):
        r = refs[i]
        mean, var = blocked(c, i)
        assert PC.passes_old_criterion(mean, var, r) and not rejected(mean, var, r)
        bm, bv, _ = r.bounds(8)
        v1 = var.copy(); v1[j_train] += 64 * bv[j_train]
        m2 = mean.copy(); m2[j_train] -= 64 * bm[j_train]
        assert rejected(mean, v1, r), (n, i, "seed 1")
        assert rejected(m2, var, r), (n, i, "seed 2")
        old = PC.passes_old_criterion(mean, v1, r), PC.passes_old_criterion(m2, var, r)
        n_old += all(old)
        if i in small:                              # the small-amplitude kernel at every noise
            assert all(old), (n, i, "seeds 1 and 2 against the old criterion", old)
        if c.noises[i] == 1e-5:                     # a moved variance of 1e-7 is never seen by a bound on the scale of max|cov|
            assert old[0], (n, i, "seed 1 against the old criterion")
    # (seed 2 on a noise 1e-5 particle passes the old criterion unless 64 x 8 R_mean sigma exceeds 1e-8: the lone Linear, R_mean 1e-6,
    # and at n >= 144 one more ill-conditioned particle; 8 of the 11 at least)
    assert n_old >= 8, (n, n_old)
    print(f"[pred-components] seeded faults n={n}: seeds 1 and 2 rejected in {len(gap_particles(c))} particles, {n_old} of them pass the"
          " old criterion with both")

    # seed 3 moves the last mean by 1e-9 alpha_(n-1), alpha = K11^-1 x: at noise 1e-5 alpha is 1e3 .. 1e4 on data of width 1 and the
    # old criterion sees 1e-6 .. 1e-5 too; the gap is where |alpha| <= |x| / noise stays below 10, the small-amplitude kernel at noise 0.1
    gap3 = gap + len(PCS.NOISES) - 1
    assert c.noises[gap3] == 0.1
    eval_cov = R.O.eval_cov
    j = c.tq.size - 1                               # the last query, past the series

    def faulty(tree, ts):
        K = eval_cov(tree, ts).copy()
        K[c.n + j, c.n - 1] += 1e-9                 # (series_predict_blocks reads K21 from the lower-left block)
        return K
    monkeypatch.setattr(R.O, "eval_cov", faulty)
    out3 = {i: blocked(c, i) for i in gap_particles(c)}
    monkeypatch.undo()
    for i, (mean3, var3) in out3.items():
        assert rejected(mean3, var3, refs[i]), (n, i, "seed 3")
    assert PC.passes_old_criterion(*out3[gap3], refs[gap3]), (n, "seed 3 against the old criterion")


@pytest.mark.parametrize("name", PCS.CASE_NAMES)
def test_caps_hold_for_every_gpu_case(name):
    assert set(PCS.CASE_NAMES) == set(PCS.cases())
    c = PCS.case(name)
    refs = c.refs()
    for i, r in enumerate(refs):
        PC.assert_caps(r, ctx=(name, i, r.tree, r.noise))
    Rm = max(r.R_mean for r in refs); Rv = max(r.R_var for r in refs)
    Rc = max((r.R_cov for r in refs if r.R_cov is not None), default=float("nan"))
    print(f"[pred-components] {name}: n={c.n} m={c.tq.size} particles={len(refs)} worst R_mean {Rm:.2e} (cap {PC.CAP_R_MEAN:.0e}),"
          f" R_var {Rv:.2e} (cap {PC.CAP_R_VAR:.0e}), R_cov {Rc:.2e}, smallest variance {min(r.v80.min() for r in refs):.2e}")
