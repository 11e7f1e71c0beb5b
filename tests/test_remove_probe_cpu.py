"""Host side of the removal-update probe (tests/_remove_probe_ref.py; the device side is tests/test_gpu_remove_probe.py): the
conditions the probe's bound puts on its INPUTS, checked without a GPU.

  * On every case the GPU test runs, the two reference routes (reflector by reflector; columns one at a time as well) keep
    R <= 2 gamma_{n'+1} and R_s <= 4 gamma_{n'}: the bound 4 max(R, 2 gamma) is then at most 8 gamma (16 gamma for the solve) and no
    case buys the device room through a badly conditioned reference.  A case that breaks this is replaced (ALPHA_IS_Z of the
    reference module), the cap stays.
  * A correct route with another summation order — panels of 16 columns, passes of 8 — passes the device's bound on every case.
    The compact-WY route on 128-wide panels and LAPACK on the rounded target are printed beside them, never part of a bound.
  * Faults planted in a copy of the reflector route (faulty_rows: the same bits as the route without a fault) are rejected by that
    bound on the cases that exercise them."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _chol_remove_ref as C      # noqa: E402
import _factor_ref as F           # noqa: E402
import _remove_probe_ref as P     # noqa: E402


@pytest.mark.parametrize("n, name", P.CASES)
def test_reference_routes_stay_within_their_caps_and_a_blocked_route_passes(n, name):
    idx = P.PATTERNS[n][name]
    fails = []
    for fam in P.FAMILIES:
        ref = P.reference(fam, n, name)
        L0, a0 = P.inputs(fam, n, name)
        g1, g0 = F.gamma(ref["n_new"] + 1), F.gamma(ref["n_new"])
        Lb, ab = P.route_blocked(L0, a0, idx)
        Lw, aw = P.route_wy128(L0, a0, idx)
        Ll, al = P.route_lapack(ref["M"], ref["y"])
        eb, esb = P.eta(ref["M"], Lb), P.eta_s(Lb, ab, ref["y"])
        print(f"n {n} {name:13s} {fam:9s}: R {ref['R'] / g1:.3f} R_s {ref['R_s'] / g0:.3f} gamma | blocked 16/8 {eb / g1:.3f} {esb / g0:.3f} | "
              f"compact-WY 128 {P.eta(ref['M'], Lw) / g1:.3f} {P.eta_s(Lw, aw, ref['y']) / g0:.3f} | "
              f"LAPACK {P.eta(ref['M'], Ll) / g1:.3f} {P.eta_s(Ll, al, ref['y']) / g0:.3f}")
        if not ref["R"] <= 2 * g1:
            fails.append(f"{fam}: R = {ref['R'] / g1:.4g} gamma_(n'+1) > 2")
        if not ref["R_s"] <= 4 * g0:
            fails.append(f"{fam}: R_s = {ref['R_s'] / g0:.4g} gamma_n' > 4")
        if not eb <= ref["bound"]:
            fails.append(f"{fam}: blocked route eta = {eb / g1:.4g} gamma above the bound {ref['bound'] / g1:.4g} gamma")
        if not esb <= ref["bound_s"]:
            fails.append(f"{fam}: blocked route eta_s = {esb / g0:.4g} gamma above the bound {ref['bound_s'] / g0:.4g} gamma")
    assert not fails, "\n".join(fails)


def test_families_sizes_and_patterns():
    assert P.FAMILIES == F.FAMILIES + ("se_short",) and len(P.CASES) == 27
    assert sorted({n for n, _ in P.CASES}) == [2, 17, 129, 257, 300, 384]
    for n, name in P.CASES:
        idx = P.PATTERNS[n][name]
        assert idx == sorted(set(idx)) and 0 <= idx[0] and idx[-1] < n and len(idx) < n
    early = [(n, name) for n, name in P.CASES if P.returns_early(n, P.PATTERNS[n][name])]
    assert early == [(129, "last"), (257, "last"), (384, "tile_row")]
    # the passes and lane-pair widths the patterns are there for: (run length) -> columns of each pass
    widths = {name: [min(32, r - c0) for _, r in C.runs_of(idx) for c0 in range(0, r, 32)] for name, idx in P.PATTERNS[300].items()}
    assert widths["front3"] == [3] and widths["front8"] == [8] and widths["front9"] == [9] and widths["front32"] == [32]
    assert widths["r33"] == [32, 1] and widths["r40"] == [32, 8] and widths["r128"] == [32] * 4 and widths["comb64"] == [1] * 64
    assert C.runs_of(P.PATTERNS[300]["tile_start"]) == [(128, 1)] and len(C.runs_of(P.PATTERNS[300]["three_runs"])) == 3
    # se_short is what reaches the negligible-row branch: exact zeros and denormals below the diagonal of its factor
    L0 = P.factor("se_short", 300)[0]
    low = L0[np.tril_indices(300, -1)]
    assert (low == 0).sum() > 10000 and (np.abs(low[low != 0]) < np.finfo(np.float64).tiny).any()
    W = L0[1:, 0]
    assert ((W * W > 0) & (W * W <= np.diag(L0)[1:] ** 2 * C.NEGLIGIBLE)).any() or (W == 0).any()


def test_metrics_on_known_perturbations():
    L0, a0 = P.inputs("wishart", 300, "first")
    ref = P.reference("wishart", 300, "first")
    L, al = P.route_reflector(L0, a0, [0])
    assert P.eta(ref["M"], L) <= ref["bound"] and P.eta_s(L, al, ref["y"]) <= ref["bound_s"]
    Lp = L.copy(); Lp[200, 50] *= 1 + 1e-11      # one element off by 1e-11 relative
    assert P.eta(ref["M"], Lp) > ref["bound"]
    # (the solve is measured against ||L'_i|| ||alpha'||, ~17 |alpha'_i| here: its resolution on one entry is some 1e-11 relative)
    ap = al.copy(); ap[np.argmax(np.abs(al))] *= 1 + 1e-10
    assert P.eta_s(L, ap, ref["y"]) > ref["bound_s"]
    bad = L.copy(); bad[5, 5] = np.nan
    assert P.eta(ref["M"], bad) == np.inf


def _first_a(idx):
    return C.runs_of(idx)[0][0]


def _fault_skip_row(idx, taus, n_new):
    a = _first_a(idx)
    return ("skip_row", 0, 0, a, a + 1)


def _fault_tau(idx, taus, n_new):
    _, ri, pi, j = max((t for t in taus if t[3] < n_new - 1), key=lambda t: t[0])
    return ("tau", ri, pi, j, 1 + 1e-9)


FAULTS = {
    # one reflector (the first of the run) not applied to the row right below it
    "skip_row": (_fault_skip_row, [(17, "first"), (129, "first"), (300, "front8"), (300, "r33"), (300, "tile_start")]),
    # tau of the largest-tau reflector (with rows below it) scaled by 1 + 1e-9
    "tau": (_fault_tau, [(17, "scattered"), (129, "first"), (300, "first"), (300, "front9"), (300, "r40"), (300, "comb64")]),
    # the source row at a taken from old row a + r - 1
    "src_row": (lambda idx, taus, n_new: ("src_row",), [(17, "scattered"), (300, "front3"), (300, "r33"), (300, "across_tile"), (300, "tile_start")]),
    # the carried alpha entries of the run dropped between two passes (runs wider than one pass)
    "drop_carried": (lambda idx, taus, n_new: ("drop_carried",), [(300, "r33"), (300, "r40"), (300, "r128")]),
    # one column of W skipped in the second tile row
    "skip_w": (lambda idx, taus, n_new: ("skip_w", 0), [(257, "first"), (300, "front9"), (300, "r40"), (300, "across_tile")]),
}
# Where a fault is NOT exercised, by construction of the input (asserted: the faulted route gives the clean route's bits): the
# factor of se_short is diagonal to working precision at n = 17 (every reflector is the identity) and has exact zeros in column 0
# from row 128 on.
NOT_EXERCISED = {("skip_row", 17, "first", "se_short"), ("tau", 17, "scattered", "se_short"),
                 ("skip_w", 257, "first", "se_short"), ("skip_w", 300, "front9", "se_short"), ("skip_w", 300, "r40", "se_short")}
# ... and where it is exercised below the metric's resolution: spec's largest tau sits at a row whose diagonal entry is ~1e-5 of the
# row's norm, and a relative 1e-9 of that column's entries is 1e-14 of the rows' norms spread over the trailing rows — under the
# row-wise bound (eta measures against sqrt(M_ii M_jj), not against the entry).
BELOW_RESOLUTION = {("tau", 300, "first", "spec")}


@pytest.mark.parametrize("kind", sorted(FAULTS))
def test_planted_faults_are_rejected(kind):
    make, cases = FAULTS[kind]
    fails = []
    for n, name in cases:
        idx = P.PATTERNS[n][name]
        for fam in P.FAMILIES:
            ref = P.reference(fam, n, name)
            L0, a0 = P.inputs(fam, n, name)
            taus = []
            Lc, ac = P.faulty_rows(np.array(L0), np.array(a0), idx, None, taus=taus)
            Lr, ar = P.route_reflector(L0, a0, idx)
            assert np.array_equal(Lc, Lr) and np.array_equal(ac, ar), "the copy without a fault is not the reference route"
            fault = make(idx, taus, ref["n_new"])
            Lf, af = P.faulty_rows(np.array(L0), np.array(a0), idx, fault)
            changed = not (np.array_equal(Lf, Lc) and np.array_equal(af, ac))
            e, es = P.eta(ref["M"], Lf), P.eta_s(Lf, af, ref["y"])
            rejected = e > ref["bound"] or es > ref["bound_s"]
            print(f"{kind} {fault[1:]} n {n} {name} {fam}: changed {changed}, eta / bound {e / ref['bound']:.3g}, eta_s / bound {es / ref['bound_s']:.3g}")
            key = (kind, n, name, fam)
            if key in NOT_EXERCISED:
                if changed:
                    fails.append(f"{key}: listed as not exercised, but the fault changed the result")
            elif key in BELOW_RESOLUTION:
                if not changed:
                    fails.append(f"{key}: listed as below the resolution, but the fault changed nothing")
            elif not rejected:
                fails.append(f"{key}: fault {fault} passes the bound (eta / bound {e / ref['bound']:.3g}, eta_s / bound {es / ref['bound_s']:.3g})")
    assert not fails, "\n".join(fails)


def test_entry_declared_and_exported(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert "int agp_debug_remove_factor(agp_ctx* ctx, const double* L0" in hdr
    assert "agp_debug_remove_factor" in pkg.EXPORTED_SYMBOLS and hasattr(pkg.GPEngine, "debug_remove_factor")
