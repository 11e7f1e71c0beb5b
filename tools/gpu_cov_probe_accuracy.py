"""Figures of the covariance probe (GPEngine.debug_cov_sweep; tests/test_gpu_cov_probe.py, tests/_cov_probe_ref.py) on one MI355X:

    python tools/gpu_cov_probe_accuracy.py [out.txt]          (default: profiles/cov_probe_accuracy.txt)

Per sweep (path) and program (family): R of the float64 routes in units of 2^-53; the device's worst |dev - target| / (R S) and
where it occurred (tile, row and column inside it, table entry); the device's worst error in units of 2^-53 S; and, on table
paths, the largest |mean signed error| over the lag diagonals of at least 16 pairs, relative to the diagonal's mean S, next to the
same figure of the float64 table route (recorded, not asserted: a representative that is coherently off shows there while every
entry stays inside its bound)."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def diagonal_bias(err, S, entry, lower):
    """largest |mean(err)| / mean(S) over the table entries that at least 16 stored elements read"""
    e = entry[lower]
    cnt = np.bincount(e)
    se = np.bincount(e, weights=err[lower])
    ss = np.bincount(e, weights=S[lower])
    ok = cnt >= 16
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(se[ok]) / ss[ok]))


def main(out_path):
    import __graft_entry__ as g
    import _cov_probe_ref as R
    pkg = g.load_package()
    U = R.U
    cases = R.sweep_cases(pkg.prior)
    old = os.environ.get("AGP_GE_TABLE")
    os.environ["AGP_GE_TABLE"] = "0"
    engines = {"no_ge_table": pkg.GPEngine(0)}
    if old is None:
        os.environ.pop("AGP_GE_TABLE")
    else:
        os.environ["AGP_GE_TABLE"] = old
    engines["default"] = pkg.GPEngine(0)
    lines = [f"Covariance probe, {engines['default'].version}: per sweep and program — R (units of 2^-53), the device's worst",
             "|dev - target| / (R S) with its place (tile, row, column, table entry), its worst error in units of 2^-53 S, and on table",
             "paths the largest |mean signed error| / mean S over the lag diagonals of >= 16 pairs: device, then the float64 table route.",
             "Bound of tests/test_gpu_cov_probe.py: 8 R S on every entry (R here without the sampled scalar route: never above the tests').", ""]
    overall = (0.0, "")
    for name, (mk, n, mode, kw) in cases.items():
        ts, xs = mk()
        n = len(ts) if n is None else n
        lay = R.sweep_layout(ts, n, mode, pkg.probe_lattice(ts) if mode != "general" else None)
        allp = R.sweep_programs(pkg, ts, large=name in R.LARGE_CASES, for_gradient=bool(kw.get("for_gradient")))
        tile = np.arange(n) // R.NB
        lower = tile[:, None] >= tile[None, :]
        for ename in (("default", "no_ge_table") if mode == "general" else ("default",)):
            eng = engines[ename]
            eng.set_data(ts, xs)
            lines.append(f"==== {name} (n = {n} of {len(ts)}, {mode}{', gradient plan' if kw.get('for_gradient') else ''}"
                         f"{', log|dt| table' if mode == 'general' and ename == 'default' else ''}) ====")
            for group in R.GROUPS:
                progs = R.program_group(allp, group)
                out = eng.debug_cov_sweep([nd for _, nd, _ in progs], np.array([z for _, _, z in progs]), n=n, want_tables=False, **kw)
                assert out["mode"] == mode
                for p, (nm, nd, nz) in enumerate(progs):
                    ref = R.Ref(nd.to_tuple(), nz, ts[:n] if mode == "general" else ts, lay, scalar_twin=False)
                    err = (out["K"][p][:n, :n].astype(R.LD) - ref.target).astype(np.float64)
                    rel = np.where(lower, np.abs(err) / ref.S, 0.0)
                    i, j = np.unravel_index(int(np.argmax(rel)), rel.shape)
                    w = float(rel[i, j])
                    place = f"tile ({i // R.NB},{j // R.NB}) row {i % R.NB} col {j % R.NB}" + (f" entry {int(lay.entry[i, j])}" if lay.tables else "")
                    bias = ""
                    if lay.tables:
                        route = (R.table_route(nd.to_tuple(), nz, ts, lay).astype(R.LD) - ref.target).astype(np.float64)
                        bias = f"  diagonal bias dev {diagonal_bias(err, ref.S, lay.entry, lower) / U:7.3f} route {diagonal_bias(route, ref.S, lay.entry, lower) / U:7.3f}"
                    ratio = w / ref.R if ref.R > 0 else 0.0
                    overall = max(overall, (ratio, f"{name}/{ename}/{group}/{nm}"))
                    lines.append(f"  {group:4s} {nm:9s} {out['decode'][p]:8s} R {ref.R / U:5.2f}  worst/(R S) {ratio:5.2f}  worst {w / U:6.2f} u S  at {place}{bias}")
    lines.insert(5, f"Largest |dev - target| / (R S) of all: {overall[0]:.2f} ({overall[1]}).")
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text("\n".join(lines) + "\n")
    print(lines[5])
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "cov_probe_accuracy.txt"))
