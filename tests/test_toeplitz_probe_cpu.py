"""Host side of the Schur (Toeplitz) kernel probe (tests/_toeplitz_probe_ref.py; the device side is
tests/test_gpu_toeplitz_probe.py), checked without a GPU:

  * the longdouble recursion that is the target above 513 points, against the dense longdouble target at n <= 300 and against the
    closed forms of the AR(1) and MA(1) columns;
  * every family admitted at every size the GPU test uses: all four float64 routes complete with |rho| < 1, and stay inside the
    bounds the device is held to (a bound is the smaller of a multiple of the routes' own error and a conditioning cap, so this is
    a condition on the cap);
  * the constructor of first columns with chosen reflection coefficients: the recursion reproduces them, and the dense longdouble
    Cholesky and the four routes fail or succeed at the planted column as intended;
  * faults planted in the direct / recurrence route are rejected by at least one metric at its bound on the cases listed."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _factor_ref as F              # noqa: E402
import _toeplitz_probe_ref as T      # noqa: E402

LD = T.LD


@pytest.mark.parametrize("n, m", [(17, 0), (17, 40), (300, 0), (120, 90)])
def test_longdouble_recursion_matches_the_dense_target(n, m):
    """both are longdouble algorithms: their distance is 2^-11 of a float64 route's; 2^-8 of the float64 bounds leaves three bits"""
    N = n + m
    fails = []
    for fam in T.FAMILIES:
        ref = T.reference(fam, 2 if m else 1, n, m)
        tg = ref["tg"]
        assert tg["dense"]
        s = T.schur(np.asarray(ref["r_eff"], dtype=LD), ref["x"], n, N, 0, dtype=LD, recur=False, store=True)
        assert s["ok"]
        res = dict(L=s["L"], fwd=s["fwd"], sol=T.back_plain(s["L"], s["fwd"]), logdet=s["logdet"], qxx=s["fwd"][0] @ s["fwd"][0],
                   pacc=s["pacc"], lps={vi: T.logpdf_from(n, s["logdet"], s["fwd"], lv, dtype=LD)[0] for vi, lv in enumerate(T.VARIANTS)})
        e = T.quantities(tg, res, T.VARIANTS, True)
        e["eta"] = T.eta_full(ref["r_eff"], s["L"])
        for k, v in e.items():
            if not v <= ref["bound"][k] / 256:
                fails.append(f"{fam} {k}: {v:.3g} above 2^-8 of the float64 bound {ref['bound'][k]:.3g}")
    assert not fails, "\n".join(fails)


def test_longdouble_recursion_matches_the_closed_forms():
    for n in (300, 2049):
        # (the column itself is rounded to longdouble: an entry's 2^-64 moves rho_k by up to ~k 2^-64 / (1 - rho^2) and log|T| by the sum)
        tol = 5 * n * n * 2.0 ** -63
        g = np.arange(n)
        rho = LD("0.9")
        r = rho ** g.astype(LD)
        s = T.schur(r, np.zeros(n), n, n, 0, dtype=LD, recur=False, store=n == 300)
        assert s["ok"]
        assert abs(s["rho"][1] - rho) < 1e-18 and np.abs(s["rho"][2:]).max() < 1e-17
        assert abs(s["logdet"] - (n - 1) * np.log(1 - rho * rho)) < tol
        if n == 300:
            Lc = np.zeros((n, n), dtype=LD)
            d = g[:, None] - g[None, :]
            Lc[d >= 0] = (rho ** np.abs(d).astype(LD))[d >= 0]
            Lc[:, 1:] *= np.sqrt(1 - rho * rho)
            assert np.abs(s["L"] - np.tril(Lc)).max() < 1e-15
        # MA(1), theta = -0.9: |T_n| = (1 - theta^(2 n + 2)) / (1 - theta^2)
        r = np.zeros(n, dtype=LD); r[0] = LD("1.81"); r[1] = LD("-0.9")
        s = T.schur(r, np.zeros(n), n, n, 0, dtype=LD, recur=False)
        th2 = LD("0.81")
        assert s["ok"] and abs(s["logdet"] - np.log((1 - th2 ** (n + 1)) / (1 - th2))) < tol
        # its pivots: L(k,k)^2 = (1 - theta^(2 k + 4)) / (1 - theta^(2 k + 2))
        k = np.arange(n).astype(LD)
        assert np.abs(s["diag"] ** 2 - (1 - th2 ** (k + 2)) / (1 - th2 ** (k + 1))).max() < 1e-15


def test_update_form_of_the_targets_matches_a_dense_factorisation_of_k():
    """the targets take log N(x; 0, T + U C U') from T's factor (determinant lemma and Woodbury, in longdouble); here against a dense
    longdouble Cholesky of the full matrix, on the benign families (the comparison itself is conditioned like T)"""
    for n, rank0 in ((17, 0), (120, 5)):
        for fam in ("ar1", "ma1", "ge1", "se_per", "const_wn", "refl"):
            ref = T.reference(fam, 0, n, 0, rank0)
            for lv in T.VARIANTS:
                lp, terms = T.target_logpdf(ref["tg"], lv)
                dense = T.dense_logpdf(ref["r_eff"], ref["x"], n, rank0, lv)
                # (two longdouble evaluations: unit roundoff 5.4e-20, n <= 120 terms, condition numbers up to ~1e7 on these families)
                assert abs(lp - dense) <= 1e-10 * float(terms), (fam, n, lv, float(lp), float(dense))


def test_decimal_target_of_the_near_singular_cases():
    """target_hp (80 digits) against the dense longdouble target on a benign case, and what it is there for: with 1 - 1e-12 planted at
    column 1 the longdouble recursion is 4e-11 relative off in the Schur complement's diagonal, forty times the bound of that quantity"""
    n, m = 17, 40
    ref = T.reference("ge1", 2, n, m)
    hp = T.target_hp(ref["r_eff"], ref["x"], n, n + m)
    for k in ("L", "fwd", "sol", "pacc", "pacc_terms"):
        assert np.abs(hp[k] - ref["tg"][k]).max() < 1e-16, k
    assert abs(hp["logdet"] - ref["tg"]["logdet"]) < 1e-16 and abs(hp["qxx"] - ref["tg"]["qxx"]) < 1e-15
    n, m = 520, 80
    r = np.asarray(T.inverse_schur(T.planted_rho(n + m, 1, 1 - LD("1e-12"), True)), dtype=np.float64)
    x = T.rhs_x(n)
    hp = T.target_hp(r, x, n, n + m)
    ld = T.target(r, x, n, n + m)
    off = float(np.abs(ld["pacc"][3] - hp["pacc"][3]).max())
    again = T.target_hp(r, x, n, n + m, digits=120)
    assert float(np.abs(again["pacc"][3] - hp["pacc"][3]).max()) < 1e-30
    assert 1e-21 < off < 1e-19 and off > 16 * F.gamma(n + 2) * float(hp["pacc"][3].max())


def _cases():
    out = [(0, n, 0, T.RANK0_MODE0) for n in T.SIZES_01 + T.SIZES_0_BIG]
    out += [(1, n, 0, 0) for n in T.SIZES_01]
    out += [(2, n, m, 0) for n, m in T.SIZES_2]
    return out


def _check_admitted(fam, mode, n, m, rank0):
    ref = T.reference(fam, mode, n, m, rank0)
    fails = []
    if not ref["admitted"] or not ref["max_rho"] < 1:
        return [f"{fam}: not admitted (max |rho| = {ref['max_rho']})"]
    for k, v in ref["R"].items():
        if not v <= ref["bound"][k]:
            fails.append(f"{fam} {k}: the routes' {v:.3g} is above the bound {ref['bound'][k]:.3g}")
    g1, g0 = F.gamma(n + 1), F.gamma(n)
    R = ref["R"]
    print(f"mode {mode} n {n} m {m} {fam:9s}: max|rho| {ref['max_rho']:.6f}  R eta {R.get('eta', 0) / g1:.3g} gamma  solve_f {R.get('solve_f', 0) / g0:.3g} gamma  "
          f"solve_b {R.get('solve_b', 0) / g0:.3g} gamma  logdet {R.get('logdet', 0):.3g} / {ref['bound'].get('logdet', 0):.3g}")
    return fails


@pytest.mark.parametrize("mode, n, m, rank0", _cases())
def test_families_are_admitted_and_the_routes_meet_the_bounds(mode, n, m, rank0):
    fails = []
    for fam in T.FAMILIES:
        fails += _check_admitted(fam, mode, n, m, rank0)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode, n, m", [(1, 2048, 0), (2, 2048, 2048)])
def test_large_store_cases_are_admitted(mode, n, m):
    fails = []
    for fam in T.BIG_FAMILIES:
        fails += _check_admitted(fam, mode, n, m, 0)
    assert not fails, "\n".join(fails)


PLANT_COLS = (1, 2, 255, 256, 257, 511, 512)


@pytest.mark.parametrize("k", PLANT_COLS + (-1,))
def test_inverse_schur_plants_the_coefficient_it_is_given(k):
    N = 600
    k = N - 1 if k < 0 else k
    # the recursion reproduces a whole sequence of coefficients
    rho = T.planted_rho(N, k, LD("0.5"), quiet=False)
    r = T.inverse_schur(rho)
    s = T.schur(r, np.zeros(N), N, N, 0, dtype=LD, recur=False)
    assert s["ok"] and np.abs(s["rho"][1:] - rho[1:]).max() < 1e-14
    for value, quiet, fails in ((1 + LD("1e-9"), False, True), (-(1 + LD("1e-9")), False, True), (LD(1), True, True), (LD(-1), True, True),
                                (1 - LD("1e-12"), True, False)):
        r = np.asarray(T.inverse_schur(T.planted_rho(N, k, value, quiet)), dtype=np.float64)
        try:
            F.ref_chol(T.toeplitz(r.astype(LD)[:k + 2 if k + 2 <= N else N]))
            failed = False
        except ArithmeticError as e:
            failed = True
            assert f"pivot {k} " in str(e), (k, value, str(e))
        assert failed == fails, (k, float(value), quiet)
        for mixed, recur in T.ROUTES:
            s = T.schur(r, np.zeros(N), N, N, 0, mixed=mixed, recur=recur)
            if fails:
                assert not s["ok"] and s["bad_col"] == k, (k, float(value), mixed, recur, s["bad_col"])
            else:
                assert s["ok"] and abs(abs(s["rho"][k]) - 1) < 2e-12


# fault -> the cases (mode, n, m, rank0) on which at least one family must break at least one metric at its bound
FAULT_CASES = {
    "u_unshifted": [(1, 17, 0, 0), (1, 257, 0, 0)],
    "rho_sign": [(1, 17, 0, 0), (1, 257, 0, 0)],
    "pivot_late": [(1, 17, 0, 0), (1, 257, 0, 0)],
    # (at n = 257 the only element of register 1 is j = k itself, read again only by the future rows: mode 2 at (256, 1))
    "skip_rlo": [(2, 256, 1, 0), (1, 300, 0, 0)],
    # (with the recurrence's pivot stored as L(k,k), what element j = k computes is read again only by the future rows' diagonal sums)
    "ge_gt": [(2, 5, 3, 0), (2, 17, 40, 0)],
    "e_zero": [(1, 5, 0, 0), (1, 17, 0, 0)],
    "c01_sign": [(0, 17, 0, T.RANK0_MODE0), (0, 257, 0, T.RANK0_MODE0)],
    "tau_no_rank0": [(0, 17, 0, T.RANK0_MODE0), (0, 257, 0, T.RANK0_MODE0)],
    "be_from_nm1": [(2, 5, 3, 0), (2, 17, 40, 0)],
    "tri_transposed": [(1, 5, 0, 0), (1, 17, 0, 0)],
    "missing_zero_pivot": [(1, 5, 0, 0), (1, 17, 0, 0)],
}


def test_fault_list_is_complete():
    assert sorted(FAULT_CASES) == sorted(T.FAULTS_FORWARD + T.FAULTS_LIN + T.FAULTS_BACK)
    gpu_cases = set(_cases())
    for cases in FAULT_CASES.values():
        assert set(cases) <= gpu_cases


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_planted_faults_are_rejected(fault):
    caught = []
    for mode, n, m, rank0 in FAULT_CASES[fault]:
        n_caught = 0
        for fam in T.FAMILIES:
            ref = T.reference(fam, mode, n, m, rank0)
            store = mode >= 1
            res = T.run_route(ref["r_eff"], ref["x"], n, n + m, rank0, False, True, T.VARIANTS, store=store, fault=fault)
            if res is None:                      # the faulty route refuses an admitted input: the device would report info = 1
                n_caught += 1
                continue
            e = T.quantities(ref["tg"], res if store else {k: v for k, v in res.items() if k != "L"}, T.VARIANTS, True)
            if store:
                e["eta"] = T.eta_of(ref["r_eff"], res["L"])
            broken = [k for k, v in e.items() if not v <= ref["bound"][k]]
            print(f"{fault} mode {mode} n {n} m {m} {fam}: breaks {broken}")
            n_caught += bool(broken)
        caught.append(n_caught)
    assert all(c >= 1 for c in caught), f"{fault}: families that reject it per case {caught}"


def test_entry_declared_and_exported(pkg):
    hdr = (ROOT / "include" / "autogp_hip.h").read_text()
    assert "int agp_debug_toeplitz(agp_ctx* ctx, int32_t mode" in hdr
    assert "agp_debug_toeplitz" in pkg.EXPORTED_SYMBOLS and hasattr(pkg.GPEngine, "debug_toeplitz")
