"""Errors of the Schur (Toeplitz) kernels on caller-supplied first columns (agp_debug_toeplitz: launch_toep_logpdf on caller data) on
the cases of tests/test_gpu_toeplitz_probe.py, next to the four float64 routes that set the test's bounds.

    python tools/gpu_toeplitz_probe_accuracy.py [out.txt]      # default profiles/toeplitz_probe_accuracy.txt

Per mode x n (x m) x family and quantity: the device's figure, the four routes' (direct / mixed rotation x pivot by division / by
recurrence) and the bound.  eta in gamma_{n+1}, the two omega_solve figures in gamma_n, the end quantities as absolute errors
against the longdouble target (sol: largest error / largest entry; lp, sol, pacc: the worst of the variants / right-hand sides / rows).
Nothing reads the file: the tests' bounds come from the host routes."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as g
import numpy as np
import _factor_ref as F
import _toeplitz_probe_ref as T
import test_gpu_toeplitz_probe as G

pkg = g.load_package()
eng = pkg.GPEngine(0)
out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "toeplitz_probe_accuracy.txt"
lines = ["# agp_debug_toeplitz (k_toep_logpdf / k_toep_back through launch_toep_logpdf on caller first columns), MI355X, per mode x n x m x",
         "# family of tests/_toeplitz_probe_ref.py; one call per mode x n x m, four particles per family (0, 1, 2 Linear leaves, zero amplitude",
         "# + split table).  Per quantity: device | direct/div direct/rec mixed/div mixed/rec (float64 routes) | bound.  eta in gamma_{n+1},",
         "# solve_f = omega_solve(L_dev, fwd, rhs) and solve_b = omega_solve(L_dev', sol, fwd) in gamma_n; logdet, qxx = b_x'b_x, lp, pacc:",
         "# absolute error against the longdouble target; sol: largest error / largest entry.  lp, sol, pacc: the worst of the variants /",
         "# right-hand sides / rows (relative to its bound).  Above 513 points eta is taken over the test's fixed sample of entries.",
         "# tools/gpu_toeplitz_probe_accuracy.py"]
worst = {}


def cell(name, e, ref, unit=1.0):
    r = " ".join(f"{(x[name] / unit if x and name in x else float('nan')):.3g}" for x in ref["routes"])
    return f"{name} {e[name] / unit:.3g} | {r} | {ref['bound'][name] / unit:.3g}"


def worst_of(prefix, e, ref):
    ks = [k for k in e if k[:-1] == prefix and k[-1].isdigit()]
    return max(ks, key=lambda k: e[k] / ref["bound"][k] if ref["bound"][k] > 0 else 0.0) if ks else None


cases = [(0, n, 0, T.FAMILIES) for n in T.SIZES_01 + T.SIZES_0_BIG] + [(1, n, 0, T.FAMILIES) for n in T.SIZES_01]
cases += [(1, 2048, 0, T.BIG_FAMILIES)] + [(2, n, m, T.FAMILIES) for n, m in T.SIZES_2] + [(2, 2048, 2048, T.BIG_FAMILIES)]
for mode, n, m, fams in cases:
    res_all, rank0 = G.run(eng, mode, n, m, fams)
    assert (res_all["info"] == 0).all(), (mode, n, m, res_all["info"])
    g1, g0 = F.gamma(n + 1), F.gamma(n)
    for f, fam in enumerate(fams):
        ref = T.reference(fam, mode, n, m, rank0)
        p0 = f * G.NV
        res = dict(lps={vi: res_all["lp"][p0 + vi] for vi in range(G.NV)})
        if mode >= 1:
            L, _ = T.unpack_columns(res_all["Lcols"][p0 + 1], n)
            fwd, sol = res_all["fwd"][p0 + 1, :, :n], res_all["sol"][p0 + 1, :, :n]
            res.update(L=L, fwd=fwd, sol=sol, logdet=2 * np.log(np.diag(L).astype(T.LD)).sum(), qxx=fwd[0].astype(T.LD) @ fwd[0].astype(T.LD))
        if mode == 2:
            res["pacc"] = res_all["pacc"][p0 + 1, :, :m]
        e = T.quantities(ref["tg"], res, T.VARIANTS, True)
        cells = []
        if mode >= 1:
            e["eta"] = T.eta_of(ref["r_eff"], res["L"])
            cells += [cell("eta", e, ref, g1), cell("solve_f", e, ref, g0), cell("solve_b", e, ref, g0), cell("logdet", e, ref), cell("qxx", e, ref)]
        for prefix in ("lp", "sol", "pacc"):
            k = worst_of(prefix, e, ref)
            if k:
                cells.append(cell(k, e, ref))
        for k, v in e.items():
            ratio = v / ref["bound"][k] if ref["bound"][k] > 0 else 0.0
            key = k.rstrip("0123")
            if ratio > worst.get(key, (0.0, ""))[0]:
                worst[key] = (ratio, f"mode {mode} n {n} m {m} {fam} {k}")
        lines.append(f"  mode {mode} n {n:4d} m {m:4d} {fam:9s} max|rho| {ref['max_rho']:.6f}  " + "   ".join(cells))
    print(f"mode {mode} n {n} m {m} done", flush=True)
lines.append("# closest to its bound, per quantity (error / bound):")
lines += [f"#   {k:8s} {v[0]:.4f} ({v[1]})" for k, v in sorted(worst.items())]
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
print("\n".join(lines[-12:]))
eng.close()
