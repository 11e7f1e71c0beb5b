"""Backward errors of the short-series kernel's factorisation (agp_debug_series_factor) on the matrix families of
tests/_factor_ref.py at the sizes of tests/test_gpu_series_probe.py, next to LAPACK's on the same matrices and to the bound the
test applies.  A record only: the test's margins are those of the tile schedules (tests/test_gpu_factor_probe.py), not this table.

    python tools/gpu_series_probe_accuracy.py [out.txt]      # default profiles/series_probe_accuracy.txt

Per family x n (the worst matrix of the family in the batch of nine, P = 9): omega / gamma_{n+1} of the factor, omega_solve /
gamma_n of the carried forward solve, LAPACK's two ratios, kappa_blk of the reference factor (the smallest in the family) and the
two bounds min(M, kappa_blk, BENIGN_CAP) the test holds the ratios against."""
import sys
from pathlib import Path

import numpy as np
import scipy.linalg as sla

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g
import _factor_ref as R
import _series_cases as S
from test_gpu_factor_probe import M, M_SOLVE, BENIGN_CAP

pkg = g.load_package()
eng = pkg.GPEngine(0)
out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "series_probe_accuracy.txt"
lines = ["# omega / gamma_{n+1} (factor) and omega_solve / gamma_n (forward solve) of agp_debug_series_factor (the factorisation of",
         "# k_series_logpdf on caller matrices), MI355X, per family x n, worst matrix of the family in the batch of nine of",
         "# tests/_factor_ref.py (P = 9); lapack_* = scipy.linalg.cholesky / solve_triangular on the same matrices; kappa_blk = smallest",
         "# over the family's matrices (reference factor); bound_* = min(M, kappa_blk, BENIGN_CAP) of tests/test_gpu_series_probe.py.",
         "# tools/gpu_series_probe_accuracy.py",
         f"# {'family':9s} {'n':>4s} {'omega':>9s} {'solve':>9s} {'lapack_om':>9s} {'lapack_sv':>9s} {'kappa_blk':>10s} {'bound_om':>9s} {'bound_sv':>9s}"]
worst = {}
for n in S.SIZES:
    batch = R.batch_of_nine(n)
    K = np.stack([k for _, k in batch]); labels = [l for l, _ in batch]
    y = R.batch_rhs(n)
    kap = [R.kappa_blk(R.ref_chol(k)) for k in K]
    lap = []
    for k, yy in zip(K, y):
        Lr = sla.cholesky(k, lower=True)
        lap.append((R.omega(k, Lr) / R.gamma(n + 1), R.omega_solve(Lr, sla.solve_triangular(Lr, yy, lower=True), yy) / R.gamma(n)))
    L, alpha, part, lp, info = eng.debug_series_factor(K, y)
    assert (info == 0).all(), (n, info)
    om = [R.omega(K[i], L[i]) / R.gamma(n + 1) for i in range(9)]
    sv = [R.omega_solve(L[i], alpha[i], y[i]) / R.gamma(n) for i in range(9)]
    for fam in R.FAMILIES:
        members = [i for i in range(9) if labels[i] == fam]
        kb = min(kap[i] for i in members)
        cap = min(kb, BENIGN_CAP.get(fam, np.inf))
        row = (max(om[i] for i in members), max(sv[i] for i in members), max(lap[i][0] for i in members), max(lap[i][1] for i in members))
        lines.append(f"  {fam:9s} {n:4d} {row[0]:9.4f} {row[1]:9.4f} {row[2]:9.4f} {row[3]:9.4f} {kb:10.4g} {min(M[fam], cap):9.4g} "
                     f"{min(M_SOLVE[fam], cap):9.4g}")
        w = worst.setdefault(fam, [0.0, 0.0])
        w[0] = max(w[0], row[0]); w[1] = max(w[1], row[1])
    print(f"n = {n} done", flush=True)
lines.append("# largest ratio per family (factor, solve) over these sizes, and the tile schedules' margins M, M_solve it is held against:")
for fam in R.FAMILIES:
    lines.append(f"#   {fam:9s} {worst[fam][0]:9.4f} {worst[fam][1]:9.4f}    M = {M[fam]:.3f}, M_solve = {M_SOLVE[fam]:.3f}")
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
eng.close()
