"""Device build of csrc/agp_math.hpp (agp_debug_math) on the inputs of tests/test_fastmath.py and against the same bounds; exp_f,
exp_t (read from an LDS copy of the table, as the covariance kernels read it), sin2_f and sincos_pi_f consist of explicit fma,
products feeding an fma operand, rint and ldexp only — nothing the device compiler may contract differently — so their device
results must also equal the host build's bit for bit.  log_f and pow_f may contract: accuracy bounds only."""
import ctypes

import mpmath as mp
import numpy as np
import pytest

import _fastmath_cases as CASES

pytestmark = pytest.mark.gpu

EXP_F, SIN2_F, LOG_F, POW_F, EXP_T, SINCOS_S, SINCOS_C = 0, 1, 2, 3, 6, 7, 8


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return CASES.build_host_lib(tmp_path_factory.mktemp("fm_gpu"))


def call1(fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64); y = np.empty_like(x)
    fn(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(x.size))
    return y


def ulps(got, ref):
    """error in units of the last place of the reference"""
    ref_f = np.array([float(r) for r in ref])
    err = np.array([abs(mp.mpf(float(g)) - r) for g, r in zip(got, ref)], dtype=object)
    return np.array([float(e / mp.mpf(np.spacing(abs(rf)) if rf != 0 else 5e-324)) for e, rf in zip(err, ref_f)])


def assert_same_bits(name, x, dev, hst):
    d = dev.view(np.uint64) != hst.view(np.uint64)
    assert not d.any(), (f"{name}: {int(d.sum())} of {x.size} device results differ from the host build, first at x = "
                         f"{x[d][0]!r}: device {dev[d][0]!r} host {hst[d][0]!r}")


@pytest.mark.parametrize("which, fn, inputs", [(EXP_F, "v_exp", CASES.exp_inputs), (EXP_T, "v_exp_t", CASES.exp_table_inputs)])
def test_exp_device(engine, host, which, fn, inputs):
    mp.mp.dps = 40
    x = inputs()
    got = engine.debug_math(which, x)
    u = ulps(got, [mp.exp(mp.mpf(float(v))) for v in x])
    print(f"device exp (which={which}): max {u.max():.3f} ulp")
    assert u.max() < 1.6, u.max()
    assert engine.debug_math(which, CASES.EXP_UNDERFLOW).tolist() == [0.0, 0.0, 0.0]
    sub = engine.debug_math(which, CASES.EXP_SUBNORMAL)[0]          # subnormal result
    assert abs(sub - float(mp.exp(-720))) <= 5e-324 * 2
    assert engine.debug_math(which, np.array([0.0]))[0] == 1.0
    xs = np.concatenate([x, CASES.EXP_UNDERFLOW, CASES.EXP_SUBNORMAL])
    assert_same_bits(fn, xs, engine.debug_math(which, xs), call1(getattr(host, fn), xs))


def test_exp_f_and_exp_t_agree_on_device(engine):
    """agreement of the two implementations where the kernels use them (arg <= 0)"""
    x = CASES.exp_table_inputs(); x = x[x <= 0]
    a = engine.debug_math(EXP_F, x); b = engine.debug_math(EXP_T, x)
    assert np.max(np.abs(a - b) / np.maximum(a, 1e-300)) < 5e-16


def test_sin2_device(engine, host):
    mp.mp.dps = 60
    x = CASES.sin2_inputs()
    got = engine.debug_math(SIN2_F, x)
    ref = [mp.sin(mp.mpf(float(v))) ** 2 for v in x]
    # near multiples of pi the value is ~0 and only absolute accuracy (relative to 1) is meaningful
    abs_err = np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(got, ref)])
    rel = abs_err / np.maximum(np.array([float(r) for r in ref]), 1e-300)
    good = np.array([float(r) for r in ref]) > 1e-6
    assert rel[good].max() < 1e-15 * 3 and abs_err.max() < 1e-15, (rel[good].max(), abs_err.max())
    assert_same_bits("sin2_f", x, got, call1(host.v_sin2, x))


def test_sincos_pi_device(engine, host):
    mp.mp.dps = 60
    x = CASES.sincos_inputs()
    s = engine.debug_math(SINCOS_S, x); c = engine.debug_math(SINCOS_C, x)
    e2 = max(float(abs(mp.mpf(float(a)) ** 2 - mp.sin(mp.mpf(float(v))) ** 2)) for a, v in zip(s, x))
    esc = max(float(abs(mp.mpf(float(a)) * mp.mpf(float(b)) - mp.sin(mp.mpf(float(v))) * mp.cos(mp.mpf(float(v)))))
              for a, b, v in zip(s, c, x))
    assert e2 < 1e-15 and esc < 1e-15, (e2, esc)
    y = np.empty(2 * x.size)
    host.v_sincos(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(x.size))
    assert_same_bits("sincos_pi_f (sine)", x, s, np.ascontiguousarray(y[0::2]))
    assert_same_bits("sincos_pi_f (cosine)", x, c, np.ascontiguousarray(y[1::2]))


def test_log_pow_device(engine):
    mp.mp.dps = 40
    x, uu, gg = CASES.log_pow_inputs()
    u = ulps(engine.debug_math(LOG_F, x), [mp.log(mp.mpf(float(v))) for v in x])
    print(f"device log_f: max {u[np.abs(x - 1.0) > 1e-3].max():.3f} ulp")
    assert u[np.abs(x - 1.0) > 1e-3].max() < 1.1
    got = engine.debug_math(POW_F, uu, gg)
    ref = [mp.mpf(float(a)) ** mp.mpf(float(b)) for a, b in zip(uu, gg)]
    rel = np.array([float(abs(mp.mpf(float(g)) - r) / r) for g, r in zip(got, ref)])
    y = np.abs(gg * np.log(uu))
    assert (rel <= (3 + 1.2 * y) * 1.12e-16).all(), (rel / ((3 + 1.2 * y) * 1.12e-16)).max()
    assert engine.debug_math(POW_F, np.zeros(3), CASES.POW_ZERO_G).tolist() == [0.0, 0.0, 0.0]
