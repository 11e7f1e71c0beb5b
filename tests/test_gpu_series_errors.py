"""The many-series entries refuse the same defect the same way (csrc/agp_series.hip: series_y_transform, mix_plan,
series_check_joint): a bad (slope, intercept), weights that do not sum to 1, and training plus query points above the joint cap, on
every entry that takes the argument — the band, the held-out scores, the samples, the decompositions (tests/_series_raw.py).

Family: three series of 5, 7 and 9 points, two query points each, two particles per series, single-leaf kernels.  Every call is the
C function itself with sentinel-filled outputs one element longer than the entry may write: a refused call launches nothing and
writes nothing.

Two defects at once: the band checks a series' transform and weights in one pass over the series, so the lower series is the one
reported, whatever the kind of its defect.  The held-out and the sampling entry check every series' transform (with its sizes and
values) in their own pass BEFORE the mixtures: a bad slope is reported ahead of bad weights even in a lower series.  Both orders
are pinned here as they are."""
import numpy as np
import pytest

import _series_raw as RAW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fam(pkg):
    return RAW.family(pkg)


def refused(pkg, engine, entry, a):
    rc, msg, o = RAW.call(pkg, engine, entry, a)
    assert rc != 0, (entry, msg)
    assert RAW.touched(o) == [], (entry, msg)                              # nothing is written
    return msg


def test_family_is_valid(pkg, engine, fam):
    """the family itself is accepted by all four entries, and every entry writes: a refusal below is the defect's"""
    for entry in RAW.ENTRIES:
        rc, msg, o = RAW.call(pkg, engine, entry, fam)
        assert rc == 0, (entry, msg)
        assert (o["info"][:-1] == 0).all() and o["info"][-1] == RAW.FILL, entry


def test_zero_slope(pkg, engine, fam):
    msgs = {e: refused(pkg, engine, e, RAW.with_yts(fam, 1, 0, 0.0)) for e in RAW.ENTRIES}
    print(msgs)
    assert all(m.startswith("series 1:") and "non-zero slope" in m for m in msgs.values()), msgs
    assert len(set(msgs.values())) == 1, msgs


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_intercept(pkg, engine, fam, bad):
    msgs = {e: refused(pkg, engine, e, RAW.with_yts(fam, 2, 1, bad)) for e in RAW.TAKES_INTERCEPT}
    print(msgs)
    assert all(m.startswith("series 2:") and "finite intercept" in m for m in msgs.values()), msgs
    assert len(set(msgs.values())) == 1, msgs


def test_weights_not_summing_to_one(pkg, engine, fam):
    msgs = {e: refused(pkg, engine, e, RAW.with_bad_weights(fam, 1)) for e in RAW.TAKES_WEIGHTS}
    print(msgs)
    assert all(m.startswith("series 1:") and "sum to 1" in m for m in msgs.values()), msgs
    assert len(set(msgs.values())) == 1, msgs


def test_joint_cap(pkg, engine, fam):
    """170 training + 10 query points = 180 > AGP_SERIES_MAX_N = 176 (each alone is allowed)"""
    assert pkg.SERIES_MAX_N == 176
    a = RAW.over_joint_cap(pkg, fam)
    for entry, word in (("held_out", "held-out"), ("sample", "query")):
        msg = refused(pkg, engine, entry, a)
        print(entry, msg)
        assert msg == f"series 1 has 170 training and 10 {word} points, together more than AGP_SERIES_MAX_N (176)"


def test_two_defects(pkg, engine, fam):
    weights0_slope1 = RAW.with_yts(RAW.with_bad_weights(fam, 0), 1, 0, 0.0)
    slope0_weights1 = RAW.with_yts(RAW.with_bad_weights(fam, 1), 0, 0, 0.0)
    for entry in RAW.TAKES_WEIGHTS:
        msg = refused(pkg, engine, entry, slope0_weights1)
        print(entry, msg)
        assert msg.startswith("series 0:") and "non-zero slope" in msg, (entry, msg)
    msg = refused(pkg, engine, "band", weights0_slope1)
    print("band", msg)
    assert msg.startswith("series 0:") and "sum to 1" in msg, msg
    for entry in RAW.JOINT:                                                # (the transforms' own pass comes first: see the docstring)
        msg = refused(pkg, engine, entry, weights0_slope1)
        print(entry, msg)
        assert msg.startswith("series 1:") and "non-zero slope" in msg, (entry, msg)
