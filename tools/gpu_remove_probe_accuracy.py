"""Row-wise backward errors of the removal update (agp_debug_remove_factor: agp_remove_data's kernels on caller factors) on the
cases of tests/test_gpu_remove_probe.py, next to the reference routes that set the test's bound and to two routes that are shown
for information only.

    python tools/gpu_remove_probe_accuracy.py [out.txt]      # default profiles/remove_probe_accuracy.txt

Per n x pattern x family: the device's eta / gamma_{n'+1} and eta_s / gamma_{n'}, the reference routes' R and R_s (the larger of
reflector by reflector and column by column), the bound 4 max(R, 2 gamma) in gamma, and the two figures of the compact-WY route on
128-wide panels and of LAPACK on the rounded target.  Then the worst ratio of every check of the test."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g
import _factor_ref as F
import _remove_probe_ref as P

pkg = g.load_package()
eng = pkg.GPEngine(0)
out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "remove_probe_accuracy.txt"
lines = ["# eta / gamma_{n'+1} (factor) and eta_s / gamma_{n'} (forward-solve vector) of agp_debug_remove_factor (the update of",
         "# agp_remove_data on caller factors), MI355X, per n x removal pattern x family of tests/_remove_probe_ref.py, one call per",
         "# n x pattern (P = 6).  R, R_s: the larger of the two reference routes (reflector by reflector; columns one at a time as well);",
         "# bound = 4 max(R, 2 gamma), what tests/test_gpu_remove_probe.py holds the device to; wy128_*: the compact-WY route on 128-wide",
         "# panels, lapack_*: numpy's Cholesky / solve on the rounded 80-bit target — both for information, never part of a bound.",
         "# 'early': whole trailing tile rows went and the update leaves the slot as it is.  tools/gpu_remove_probe_accuracy.py",
         f"# {'n':>3s} {'pattern':13s} {'family':9s} {'n_new':>5s} {'eta':>8s} {'R':>8s} {'bound':>7s} {'eta_s':>8s} {'R_s':>8s} {'bound_s':>7s} "
         f"{'wy128':>8s} {'wy128_s':>8s} {'lapack':>8s} {'lapack_s':>8s}"]
worst = dict(eta=(0.0, ""), eta_s=(0.0, ""), eta_b=(0.0, ""), eta_s_b=(0.0, ""), ld=(0.0, ""), ss=(0.0, ""), winv=(0.0, ""))


def note(key, value, where):
    if value > worst[key][0]:
        worst[key] = (float(value), where)


for n, name in P.CASES:
    idx = P.PATTERNS[n][name]
    L0, a0 = P.batch_inputs(n, name)
    L, alpha, part, winv, info = eng.debug_remove_factor(L0, a0, idx)
    assert (info == 0).all(), (n, name, info)
    early = P.returns_early(n, idx)
    for p, fam in enumerate(P.FAMILIES):
        ref = P.reference(fam, n, name)
        m = ref["n_new"]
        g1, g0 = F.gamma(m + 1), F.gamma(m)
        e, es = P.eta(ref["M"], L[p, :m, :m]), P.eta_s(L[p, :m, :m], alpha[p, :m], ref["y"])
        Lw, aw = P.route_wy128(L0[p], a0[p], idx)
        Ll, al = P.route_lapack(ref["M"], ref["y"])
        where = f"n {n} {name} {fam}"
        note("eta", e / g1, where); note("eta_s", es / g0, where)
        note("eta_b", e / ref["bound"], where); note("eta_s_b", es / ref["bound_s"], where)
        lines.append(f"  {n:3d} {name:13s} {fam:9s} {m:5d} {e / g1:8.4f} {ref['R'] / g1:8.4f} {ref['bound'] / g1:7.3f} {es / g0:8.4f} "
                     f"{ref['R_s'] / g0:8.4f} {ref['bound_s'] / g0:7.3f} {P.eta(ref['M'], Lw) / g1:8.4f} {P.eta_s(Lw, aw, ref['y']) / g0:8.4f} "
                     f"{P.eta(ref['M'], Ll) / g1:8.4f} {P.eta_s(Ll, al, ref['y']) / g0:8.4f}" + ("  early" if early else ""))
        if early:
            continue
        for J in range(idx[0] // P.NB, part.shape[1]):
            sl = slice(J * P.NB, (J + 1) * P.NB)
            lg = 2 * np.log(np.diag(L[p])[sl].astype(F.LD)); sq = alpha[p, sl].astype(F.LD) ** 2
            if np.abs(lg).sum() > 0:
                note("ld", abs(F.LD(part[p, J, 0]) - lg.sum()) / (16 * F.U * np.abs(lg).sum()), where)
            if sq.sum() > 0:
                note("ss", abs(F.LD(part[p, J, 1]) - sq.sum()) / (16 * F.U * sq.sum()), where)
            for b in range(8):
                b0 = J * P.NB + 16 * b
                T, X = L[p, b0:b0 + 16, b0:b0 + 16].astype(F.LD), winv[p, J, b].astype(F.LD)
                note("winv", F._ratio_max(np.abs(T @ X - np.eye(16)), np.abs(T) @ np.abs(X)) / F.gamma(16), where)
    print(f"n = {n} {name} done", flush=True)
lines += ["# worst over all cases:",
          f"#   eta   {worst['eta'][0]:.4f} gamma_(n'+1) ({worst['eta'][1]}); closest to its bound: {worst['eta_b'][0]:.4f} of it ({worst['eta_b'][1]})",
          f"#   eta_s {worst['eta_s'][0]:.4f} gamma_n' ({worst['eta_s'][1]}); closest to its bound: {worst['eta_s_b'][0]:.4f} of it ({worst['eta_s_b'][1]})",
          f"#   log-det partial vs 2 sum log L'_ii: {worst['ld'][0]:.4f} of 16 u sum|.| ({worst['ld'][1]})",
          f"#   quadratic-form partial vs sum alpha'_i^2: {worst['ss'][0]:.4f} of 16 u sum ({worst['ss'][1]})",
          f"#   inverse blocks |L_bb X - I| / (|L_bb| |X|): {worst['winv'][0]:.4f} gamma_16 ({worst['winv'][1]})"]
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
eng.close()
