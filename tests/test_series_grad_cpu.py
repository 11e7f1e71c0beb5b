"""CPU tests of the many-short-series value-and-gradient entry (agp_logpdf_grad_series_batch): its declaration, export, documentation
and bindings; the kernel's block algorithm restated in NumPy (tests/_series_grad_ref.py) against the oracle, component by component;
the Python-side validation, which runs before any library call; and the LDS map's ChangePoint-table count quoted in the header."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _series_grad_ref as R
from oracle import gradcheck as GC

ROOT = Path(__file__).resolve().parent.parent
SYM = "agp_logpdf_grad_series_batch"


def test_entry_is_wired_everywhere(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert SYM in pkg.EXPORTED_SYMBOLS
    assert re.search(r"\bint %s\s*\(" % SYM, hdr)
    assert SYM in (ROOT / "INTEGRATION.md").read_text()
    sys.path.insert(0, str(ROOT / "tools"))
    import check_ccall_signatures as CK
    problems, _, seen, _ = CK.check()
    assert problems == [] and SYM in seen
    assert hasattr(pkg.GPEngine, "logpdf_grad_series_batch")
    shim = (ROOT / "autogp.jl_amd" / "julia" / "src" / "AutoGPHIP.jl").read_text()
    # the docstring sits directly above its own definition
    assert re.search(r'"\nfunction logpdf_grad_series_batch\(', shim)


def trees(G):
    return [G.SquaredExponential(0.3, 0.8),
            G.ChangePoint(G.SquaredExponential(0.2, 1.0), G.Periodic(0.5, 0.1, 0.8), 0.45, 0.05),
            G.Linear(0.3, 0.2, 0.7) * G.SquaredExponential(0.25, 0.8) + G.Constant(0.1)]


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 176])
def test_block_algorithm_against_the_oracle(pkg, n):
    """index algebra and weights of the packed-block inverse and contraction: every component within TAU_ORACLE of its own scale"""
    ts, xs = pkg.prior.synthetic_series(256, seed=40 + n, shuffle=True)
    ts, xs = ts[:n].copy(), xs[:n].copy()
    for node, noise in zip(trees(pkg), (0.1, 0.05, 0.2)):
        ref = GC.reference(node.to_tuple(), noise, ts, xs)
        lp, g, gn = R.series_grad_blocks(node.to_tuple(), noise, ts, xs)
        assert abs(lp - ref.lp) <= 1e-8 * max(1.0, abs(ref.lp))
        assert np.isfinite(g).all()                    # (no padding entry of dK was read with a weight)
        GC.assert_grad_components(g, gn, ref, ctx=(n, node.to_tuple()))


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were validated")


def test_python_side_validation_runs_before_any_library_call(pkg):
    good = pkg.SquaredExponential(0.3, 0.8)
    ok = (np.linspace(0, 1, 5), np.zeros(5))
    eng = object.__new__(pkg.GPEngine)
    eng._lib = _NoLibrary(); eng._ctx = None
    for entry in (eng.logpdf_grad_series_batch, eng.logpdf_series_batch):
        with pytest.raises(ValueError, match="one noise per particle"):
            entry([ok], [good, good], [0.1], [0, 0])
        with pytest.raises(ValueError, match="one noise per particle"):
            entry([ok], [good], [[0.1]], [0])
        with pytest.raises(ValueError, match="one series index per particle"):
            entry([ok], [good], [0.1], [0, 0])
        with pytest.raises(ValueError, match="one series index per particle"):
            entry([ok], [good, good], [0.1, 0.1], [[0, 0]])
        n = pkg.SERIES_MAX_N + 1
        with pytest.raises(ValueError, match="series 1 has %d points" % n):
            entry([ok, (np.zeros(n), np.zeros(n))], [good], [0.1], [0])
    # the shared helper itself
    pt_off, ts, xs, progs, P, noises, sidx = pkg.series_call_args([ok, ok], [good, good, good], [0.1, 0.2, 0.3], [1, 0, 1])
    assert P == 3 and pt_off.tolist() == [0, 5, 10] and sidx.dtype == np.int32 and noises.dtype == np.float64
    assert progs[0].shape == (4,)


def test_changepoint_tables_at_the_cap_match_the_header(pkg):
    """the number the header and the kernel's comment quote is the one the map gives"""
    N = pkg.SERIES_MAX_N
    fit_grad = max(k for k in range(1, 40) if R.cp_chain_fits(k, N, grad=True))
    fit_val = max(k for k in range(1, 40) if R.cp_chain_fits(k, N, grad=False))
    assert fit_grad < fit_val
    assert R.cp_chain_fits(fit_grad + 8, 100, grad=True)      # the same chains fit a 100-point series
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    m = re.search(r"a chain of (\d+) ChangePoint nodes \((\d+) nodes, (\d+) parameters,\s*\*?\s*(\d+) per-point tables\) fits and one of (\d+) does not", hdr)
    assert m, "the header states the count"
    assert [int(x) for x in m.groups()] == [fit_grad, 2 * fit_grad + 1, 3 * fit_grad + 1, fit_grad, fit_grad + 1]
    # the Python twin of the map is the C++ one: same expressions in csrc/agp_args.hpp
    src = (ROOT / "autogp.jl_amd" / "csrc" / "agp_args.hpp").read_text()
    for expr in ("m.o_alpha = m.o_blk + n_cp * 256;", "m.o_gprm = m.o_alpha + m.np;", "m.o_gtab = m.o_gprm + ((g_n_prm + 4) & ~1);", "m.o_red = m.o_gtab + ((g_n_ops + 1) & ~1);",
                 "m.o_blk = m.o_red + ((4 * (g_n_prm + 1) + 1) & ~1);"):
        assert expr in src, expr
