"""Backward errors of every factorisation schedule (agp_debug_factor_batch) on the matrix families of tests/_factor_ref.py, next to
LAPACK's on the same matrices: the table behind the margins M of tests/test_gpu_factor_probe.py.

    python tools/gpu_factor_probe_accuracy.py [out.txt]      # default profiles/factor_probe_accuracy.txt

Per family x n x schedule (the worst matrix of the family in the batch of nine): omega / gamma_{n+1} of the factor, omega_solve /
gamma_n of the fused forward solve, LAPACK's two ratios and kappa_blk of the reference factor (the smallest in the family: the cap of
M).  Schedule 3 (hybrid) exists at n = 300 only; -1 is agp_logpdf_batch's choice, at n = 300 with P = 9 and P = 1.  The inputs are the
tests' own (matrices and right-hand sides); at n = 300 the tests' P = 1 and P = 3 sub-batches are recorded too."""
import sys
from pathlib import Path

import numpy as np
import scipy.linalg as sla

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g
import _factor_ref as R

SIZES = (1, 5, 16, 17, 127, 128, 129, 300)
pkg = g.load_package()
eng = pkg.GPEngine(0)
out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "factor_probe_accuracy.txt"
lines = ["# omega / gamma_{n+1} (factor) and omega_solve / gamma_n (forward solve) of agp_debug_factor_batch, MI355X, per family x n x",
         "# schedule (0 mixed, 1 split, 2 right-looking, 3 hybrid, 4 dataflow, -1 logpdf_batch's choice; P = 9 unless noted), worst",
         "# matrix of the family in the batch of nine of tests/_factor_ref.py; lapack_* = scipy.linalg.cholesky / solve_triangular on",
         "# the same matrices; kappa_blk = smallest over the family's matrices (reference factor).  tools/gpu_factor_probe_accuracy.py",
         f"# {'family':9s} {'n':>4s} {'sched':>5s} {'P':>2s} {'omega':>9s} {'solve':>9s} {'lapack_om':>9s} {'lapack_sv':>9s} {'kappa_blk':>10s}"]
worst = {}
for n in SIZES:
    batch = R.batch_of_nine(n)
    K = np.stack([k for _, k in batch]); labels = [l for l, _ in batch]
    y = R.batch_rhs(n)
    kap = [R.kappa_blk(R.ref_chol(k)) for k in K]
    lap = []
    for k, yy in zip(K, y):
        Lr = sla.cholesky(k, lower=True)
        lap.append((R.omega(k, Lr) / R.gamma(n + 1), R.omega_solve(Lr, sla.solve_triangular(Lr, yy, lower=True), yy) / R.gamma(n)))
    runs = [(s, np.arange(9)) for s in (0, 1, 2, 4)]
    if n == 300:
        runs += [(3, np.arange(9)), (-1, np.arange(9))] + [(s, np.array([3])) for s in (0, 1, 2, 3, 4, -1)] + [(s, np.array([2, 3, 4])) for s in (0, 1, 2, 3, 4)]
    for sched, idx in runs:
        L, beta, part, info = eng.debug_factor_batch(K[idx], y[idx], schedule=sched)
        assert (info == 0).all(), (n, sched, info)
        om = [R.omega(K[i], L[j]) / R.gamma(n + 1) for j, i in enumerate(idx)]
        sv = [R.omega_solve(L[j], beta[j], y[i]) / R.gamma(n) for j, i in enumerate(idx)]
        for fam in R.FAMILIES:
            sel = [j for j, i in enumerate(idx) if labels[i] == fam]
            if not sel:
                continue
            members = [idx[j] for j in sel]
            row = (max(om[j] for j in sel), max(sv[j] for j in sel), max(lap[i][0] for i in members), max(lap[i][1] for i in members),
                   min(kap[i] for i in members))
            lines.append(f"  {fam:9s} {n:4d} {sched:5d} {len(idx):2d} {row[0]:9.4f} {row[1]:9.4f} {row[2]:9.4f} {row[3]:9.4f} {row[4]:10.4g}")
            w = worst.setdefault(fam, [0.0, 0.0])
            w[0] = max(w[0], row[0]); w[1] = max(w[1], row[1])
    print(f"n = {n} done", flush=True)
lines.append("# largest engine ratio per family (factor, solve) -> M = max(1, 8 x ratio):")
for fam in R.FAMILIES:
    lines.append(f"#   {fam:9s} {worst[fam][0]:9.4f} {worst[fam][1]:9.4f} -> M = {max(1.0, 8 * worst[fam][0]):.3f}, M_solve = {max(1.0, 8 * worst[fam][1]):.3f}")
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
print("\n".join(lines))
eng.close()
