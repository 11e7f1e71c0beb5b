"""Backward errors of the long-series kernel's block Cholesky (agp_debug_long_series_factor) on the matrix families of
tests/_factor_ref.py at the sizes of tests/test_gpu_long_series_probe.py, next to LAPACK's on the same matrices and to the bound the
test applies.  A record only: the test's margins are those of the tile schedules (tests/test_gpu_factor_probe.py and the large sizes
appended to profiles/factor_probe_accuracy.txt), not this table.

    python tools/gpu_long_series_probe_accuracy.py [out.txt]      # default profiles/long_series_probe_accuracy.txt

Per family x n (the worst matrix of the family in the size's batch, tests/_long_series_cases.py): omega / gamma_{n+1} of the factor,
omega_solve / gamma_n of the carried forward solve, LAPACK's two ratios, kappa_blk of the reference factor (the smallest in the
family) and the two bounds min(M, kappa_blk, BENIGN_CAP) the test holds the ratios against.  Per size n <= 176 also the number of
entries of L and alpha whose bits differ from agp_debug_series_factor's on the same batch, and per n <= 128 from each tile schedule's
(agp_debug_factor_batch, members 2, 3, 4)."""
import sys
from pathlib import Path

import numpy as np
import scipy.linalg as sla

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g
import _factor_ref as R
import _long_series_cases as LS
import _series_cases as S
from test_gpu_factor_probe import BENIGN_CAP, MEMBERS
from test_gpu_long_series_probe import bits, margins

pkg = g.load_package()
eng = pkg.GPEngine(0)
out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "long_series_probe_accuracy.txt"
lines = ["# omega / gamma_{n+1} (factor) and omega_solve / gamma_n (forward solve) of agp_debug_long_series_factor (the block Cholesky of",
         "# k_long_series_logpdf on caller matrices), MI355X, per family x n, worst matrix of the family in the size's batch of",
         "# tests/_long_series_cases.py (the batch of nine up to n = 177, its first five members above); lapack_* = scipy.linalg.cholesky /",
         "# solve_triangular on the same matrices; kappa_blk = smallest over the family's matrices (reference factor); bound_* =",
         "# min(M, kappa_blk, BENIGN_CAP) of tests/test_gpu_long_series_probe.py.  tools/gpu_long_series_probe_accuracy.py",
         f"# {'family':9s} {'n':>4s} {'omega':>9s} {'solve':>9s} {'lapack_om':>9s} {'lapack_sv':>9s} {'kappa_blk':>10s} {'bound_om':>9s} {'bound_sv':>9s}"]
worst = {}
alike = []
for n in LS.SIZES:
    labels, K, y, kap = LS.batch(n)
    Mf, Ms = margins(n)
    P = len(labels)
    lap = []
    for k, yy in zip(K, y):
        Lr = sla.cholesky(k, lower=True)
        lap.append((R.omega(k, Lr) / R.gamma(n + 1), R.omega_solve(Lr, sla.solve_triangular(Lr, yy, lower=True), yy) / R.gamma(n)))
    L, alpha, part, lp, info = eng.debug_long_series_factor(K, y)
    assert (info == 0).all(), (n, info)
    om = [R.omega(K[i], L[i]) / R.gamma(n + 1) for i in range(P)]
    sv = [R.omega_solve(L[i], alpha[i], y[i]) / R.gamma(n) for i in range(P)]
    for fam in R.FAMILIES:
        members = [i for i in range(P) if labels[i] == fam]
        kb = min(kap[i] for i in members)
        cap = min(kb, BENIGN_CAP.get(fam, np.inf))
        row = (max(om[i] for i in members), max(sv[i] for i in members), max(lap[i][0] for i in members), max(lap[i][1] for i in members))
        lines.append(f"  {fam:9s} {n:4d} {row[0]:9.4f} {row[1]:9.4f} {row[2]:9.4f} {row[3]:9.4f} {kb:10.4g} {min(Mf[fam], cap):9.4g} "
                     f"{min(Ms[fam], cap):9.4g}")
        w = worst.setdefault(fam, [0.0, 0.0, 0.0, 0.0])
        w[0] = max(w[0], row[0]); w[1] = max(w[1], row[1])
        w[2] = max(w[2], row[0] / min(Mf[fam], cap)); w[3] = max(w[3], row[1] / min(Ms[fam], cap))
    if n <= S.N_CAP:
        Ls, als, _, _, infos = eng.debug_series_factor(K, y)
        alike.append(f"#   n {n:3d} short-series kernel: {int((bits(L) != bits(Ls)).sum())} entries of L, "
                     f"{int((bits(alpha) != bits(als)).sum())} of alpha differ, info {'equal' if np.array_equal(info, infos) else 'differs'}")
    if n <= 128:
        idx = list(MEMBERS[3])
        for s in (0, 1, 2, 4, -1):
            Lt, alt, _, infot = eng.debug_factor_batch(K[idx], y[idx], schedule=s)
            alike.append(f"#   n {n:3d} tile schedule {s:2d}: {int((bits(L[idx]) != bits(Lt)).sum())} entries of L, "
                         f"{int((bits(alpha[idx]) != bits(alt)).sum())} of alpha differ, info {'equal' if np.array_equal(info[idx], infot) else 'differs'}")
    print(f"n = {n} done", flush=True)
lines.append("# largest ratio per family (factor, solve) over these sizes, and the largest share of its bound a ratio reached:")
for fam in R.FAMILIES:
    lines.append(f"#   {fam:9s} {worst[fam][0]:9.4f} {worst[fam][1]:9.4f}    share of bound {worst[fam][2]:.4f}, {worst[fam][3]:.4f}")
lines.append("# entries whose bits differ from the other factorisations' on the same matrices (n <= 176: agp_debug_series_factor on the")
lines.append("# whole batch; n <= 128: agp_debug_factor_batch on members 2, 3, 4):")
lines += alike
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
eng.close()
