"""Backward errors of every factorisation schedule (agp_debug_factor_batch) on the matrix families of tests/_factor_ref.py, next to
LAPACK's on the same matrices: the table behind the margins M of tests/test_gpu_factor_probe.py.

    python tools/gpu_factor_probe_accuracy.py [out.txt]      # default profiles/factor_probe_accuracy.txt

Per family x n x schedule (the worst matrix of the family in the batch of nine): omega / gamma_{n+1} of the factor, omega_solve /
gamma_n of the fused forward solve, LAPACK's two ratios and kappa_blk of the reference factor (the smallest in the family: the cap of
M).  Schedule 3 (hybrid) exists at n = 300 only; -1 is agp_logpdf_batch's choice, at n = 300 with P = 9 and P = 1.  The inputs are the
tests' own (matrices and right-hand sides); at n = 300 the tests' P = 1 and P = 3 sub-batches are recorded too.

    python tools/gpu_factor_probe_accuracy.py out.txt --append --sizes 641 --members 2,3,4 --schedules 0,1,3,4

records further sizes for one sub-batch (members of the batch of nine) and the given schedules, and appends the rows and their
per-family maxima to the file instead of rewriting it (tests/test_gpu_kloop.py: n = 641, six tile rows)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import scipy.linalg as sla

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g
import _factor_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=str(ROOT / "profiles" / "factor_probe_accuracy.txt"))
ap.add_argument("--sizes", default=None, help="comma-separated sizes instead of the tests' list")
ap.add_argument("--members", default=None, help="one sub-batch of the batch of nine (comma-separated indices) instead of the tests' batches")
ap.add_argument("--schedules", default=None, help="comma-separated schedules for --members")
ap.add_argument("--append", action="store_true", help="append rows and maxima to the file (no header)")
args = ap.parse_args()
SIZES = tuple(int(s) for s in args.sizes.split(",")) if args.sizes else (1, 5, 16, 17, 127, 128, 129, 300)
pkg = g.load_package()
eng = pkg.GPEngine(0)
out = Path(args.out)
lines = [] if args.append else ["# omega / gamma_{n+1} (factor) and omega_solve / gamma_n (forward solve) of agp_debug_factor_batch, MI355X, per family x n x",
         "# schedule (0 mixed, 1 split, 2 right-looking, 3 hybrid, 4 dataflow, -1 logpdf_batch's choice; P = 9 unless noted), worst",
         "# matrix of the family in the batch of nine of tests/_factor_ref.py; lapack_* = scipy.linalg.cholesky / solve_triangular on",
         "# the same matrices; kappa_blk = smallest over the family's matrices (reference factor).  tools/gpu_factor_probe_accuracy.py",
         f"# {'family':9s} {'n':>4s} {'sched':>5s} {'P':>2s} {'omega':>9s} {'solve':>9s} {'lapack_om':>9s} {'lapack_sv':>9s} {'kappa_blk':>10s}"]
worst = {}
for n in SIZES:
    batch = R.batch_of_nine(n)
    K = np.stack([k for _, k in batch]); labels = [l for l, _ in batch]
    y = R.batch_rhs(n)
    used = [int(i) for i in args.members.split(",")] if args.members else list(range(9))
    kap = [R.kappa_blk(R.ref_chol(k)) if i in used else np.inf for i, k in enumerate(K)]
    lap = []
    for i, (k, yy) in enumerate(zip(K, y)):
        if i not in used:
            lap.append((0.0, 0.0)); continue
        Lr = sla.cholesky(k, lower=True)
        lap.append((R.omega(k, Lr) / R.gamma(n + 1), R.omega_solve(Lr, sla.solve_triangular(Lr, yy, lower=True), yy) / R.gamma(n)))
    runs = [(s, np.arange(9)) for s in (0, 1, 2, 4)]
    if args.members:
        runs = [(int(s), np.array(used)) for s in (args.schedules or "0,1,2,4").split(",")]
    elif n == 300:
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
lines.append("# largest engine ratio per family (factor, solve) -> M = max(1, 8 x ratio):" if not args.append else
             f"# n = {', '.join(map(str, SIZES))}, members {args.members or 'all'}: largest engine ratio per family (factor, solve) -> M = max(1, 8 x ratio):")
for fam in R.FAMILIES:
    if fam not in worst:
        continue
    lines.append(f"#   {fam:9s} {worst[fam][0]:9.4f} {worst[fam][1]:9.4f} -> M = {max(1.0, 8 * worst[fam][0]):.3f}, M_solve = {max(1.0, 8 * worst[fam][1]):.3f}")
out.parent.mkdir(parents=True, exist_ok=True)
with open(out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
eng.close()
