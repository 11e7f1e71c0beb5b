"""Input sets of the elementary-function tests, shared by the host build (tests/test_fastmath.py) and the device build
(tests/test_gpu_fastmath.py) of csrc/agp_math.hpp so the two cannot drift; plus the host build itself."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SRC = r'''
#include "agp_math.hpp"
extern "C" {
void v_exp(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = agp::fm::exp_f(x[i]); }
void v_exp_t(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = agp::fm::exp_t(x[i], agp::fm::EXP_TAB); }
void v_sin2(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = agp::fm::sin2_f(x[i]); }
void v_sincos(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) agp::fm::sincos_pi_f(x[i], y + 2 * i, y + 2 * i + 1); }
void v_log(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = agp::fm::log_f(x[i]); }
void v_pow(const double* x, const double* g, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = agp::fm::pow_f(x[i], g[i]); }
}
'''


def build_host_lib(d):
    """The header compiled for the host into d/libfm.so: g++ -O2 -ffp-contract=off (ROCm's clang++ with the same flags when there
    is no g++)."""
    (d / "fm.cpp").write_text(SRC)
    so = d / "libfm.so"
    cxx = "g++" if shutil.which("g++") else "/opt/rocm/llvm/bin/clang++"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(ROOT / "autogp.jl_amd" / "csrc"),
                    "-o", str(so), str(d / "fm.cpp")], check=True)
    return ctypes.CDLL(str(so))


EXP_UNDERFLOW = np.array([-746.0, -1000.0, -1e9])
EXP_SUBNORMAL = np.array([-720.0])
POW_ZERO_G = np.array([0.3, 1.0, 2.0])


def exp_inputs():
    rng = np.random.default_rng(0)
    return np.concatenate([-rng.random(1500) * 50, -np.exp(rng.uniform(-40, 6.5, 1500)), rng.random(500) * 12,
                           [0.0, -1e-300, -700.0, -1e-17, 11.5]])


def exp_table_inputs():
    rng = np.random.default_rng(1)
    return np.concatenate([-rng.random(3000) * 50, -np.exp(rng.uniform(-40, 6.5, 3000)), rng.random(800) * 12,
                           np.arange(-1280, 1281) * (np.log(2) / 256),          # ties of the table index
                           [0.0, -1e-300, -700.0, -1e-17, 11.5, 700.0]])


def sin2_inputs():
    rng = np.random.default_rng(1)
    return np.concatenate([rng.random(2000) * 4, rng.random(2000) * 700, rng.random(500) * 1e5, [0.0, 1e-9, np.pi, np.pi / 2]])


def sincos_inputs():
    rng = np.random.default_rng(5)
    return np.concatenate([rng.random(2000) * 4, rng.random(2000) * 700, rng.random(500) * 1e5, [0.0, 1e-9, np.pi, np.pi / 2]])


def log_pow_inputs():
    """x of the log test, then (u, gamma) of the pow test: u = |dx|/l in (0, ~200], gamma in (0, 2] (one generator, in this order)"""
    rng = np.random.default_rng(2)
    x = np.concatenate([np.exp(rng.uniform(-30, 8, 3000)), [1.0, 0.5, 2.0, 1e-310, 5e-324, 1.4142135623730951, 0.7071067811865476]])
    uu = np.exp(rng.uniform(-25, 5.3, 4000)); gg = 2.0 / (1.0 + np.exp(-rng.standard_normal(4000)))
    return x, uu, gg
