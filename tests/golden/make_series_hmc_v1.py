"""Generator of tests/golden/series_hmc_v1.json: the cases of tests/test_gpu_series_hmc.py, their expected chains by the fp64 reference
(tests/_series_hmc_ref.py) and, per case, a MEASURED tolerance:

  the reference is rerun with every value perturbed by 1e-11 S (S = max(1, |logpdf|)) and every gradient component by 1e-11 S_k (S_k of
  oracle/gradcheck.py: oracle.gp_logpdf_grad_scales), random signs — one order above the 9.3e-13 S_k that profiles/series_grad_perf.txt
  records for the gradient entry; tol = 8 x the largest deviation of the final z, z_noise, any alpha and the final logpdf over FOUR sign
  draws (four draws sample the worst direction, they do not bound it).

A case is admitted only if every move of its reference chain has |alpha - log u| >= 1e-3 (no accept decision near its threshold), the
decisions survive all four perturbed reruns, and tol < 1e-6; otherwise the next seed is tried.  Tiny cases (n <= 24, n_hmc = 2, L = 3) are
replayed at 60 digits (oracle_mp) on the same draws and the deviation of the fp64 reference is recorded.

    python tests/golden/make_series_hmc_v1.py        (a few minutes on a CPU)"""
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as ge      # noqa: E402

G = ge.load_package()
import _series_hmc_ref as H       # noqa: E402
from oracle import oracle as O    # noqa: E402

TF = G.prior.hmc_transform_table()
PERT = 1e-11


def cp_chain(k):
    nd = G.Constant(0.5)
    for i in range(k):
        nd = G.ChangePoint(nd, G.Constant(0.3 + 0.01 * i), 0.1 + 0.8 * i / max(1, k - 1), 0.05)
    return nd


SHAPES = [      # name, n, structure, schedule
    ("se_n1", 1, G.SquaredExponential(1, 1), {}),
    ("per_n15", 15, G.Periodic(1, 1, 1), {}),
    ("ge_n16", 16, G.GammaExponential(1, 1, 1), {}),
    ("lin_x_per_n17", 17, G.Linear(1, 1, 1) * G.Periodic(1, 1, 1), {}),
    ("sum3_n33", 33, G.SquaredExponential(1, 1) + G.Periodic(1, 1, 1) + G.Linear(1, 1, 1), {}),
    ("se_n49", 49, G.SquaredExponential(1, 1), {}),
    ("defaults_n144", 144, G.SquaredExponential(1, 1) + G.Periodic(1, 1, 1), dict(n_hmc=10, L_param=10, L_noise=10)),
    ("cp_chain_n176", 176, cp_chain(4), {}),
    ("tiny_se_n12", 12, G.SquaredExponential(1, 1), dict(n_hmc=2)),
    ("tiny_ge_plus_lin_n24", 24, G.GammaExponential(1, 1, 1) + G.Linear(1, 1, 1), dict(n_hmc=2)),
]


def perturbed(ts, xs, rng):
    def f(tree, noise):
        try:
            lp, g, gn, S, Sn = O.gp_logpdf_grad_scales(tree, noise, ts, xs)
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError, OverflowError, FloatingPointError):
            return math.nan, None, math.nan, 1
        s = rng.choice([-1.0, 1.0], size=g.size + 2)
        return (lp + s[0] * PERT * max(1.0, abs(lp)), [float(a + b * PERT * c) for a, b, c in zip(g, s[1:], S)],
                gn + s[-1] * PERT * Sn, 0)
    return f


def decisions(r):
    return [[bool(m[1] < m[0]) if not math.isnan(m[1]) else None for m in row] for row in r["trace"]]


def deviation(r, ref):
    d = [abs(a - b) for a, b in zip(r["z"], ref["z"])] + [abs(r["z_noise"] - ref["z_noise"]), abs(r["logpdf"] - ref["logpdf"])]
    for ra, rb in zip(r["trace"], ref["trace"]):
        for ma, mb in zip(ra, rb):
            if not math.isnan(mb[0]) and math.isfinite(mb[0]):
                d.append(abs(ma[0] - mb[0]))
    return max(d)


def run(tree, z, zn, cls, ts, xs, seed, kw, evalfn=None, **extra):
    return H.hmc_chain(tree, z, zn, cls, TF, seed, kw["n_hmc"], evalfn or H.eval_oracle(ts, xs), L_param=kw["L_param"],
                       eps_param=kw["eps_param"], L_noise=kw["L_noise"], eps_noise=kw["eps_noise"], n_exit=kw.get("n_exit"), **extra)


def make_case(name, n, node, sched, idx):
    kw = dict(n_hmc=3, L_param=3, eps_param=0.02, L_noise=3, eps_noise=0.02)
    kw.update(sched)
    cls = G.prior.hmc_classes(node)
    tree = node.to_tuple()
    for attempt in range(50):
        seed = 1000 * (idx + 1) + attempt
        rng = np.random.default_rng(seed)
        ts, xs = (a[:n].copy() for a in G.prior.synthetic_series(max(n, 32), seed=seed, shuffle=True))
        z = [float(v) if c >= 0 else float(p) for v, c, p in zip(0.5 * rng.standard_normal(len(cls)), cls, G.encode(node)[1])]
        zn = float(0.5 * rng.standard_normal())
        try:
            ref = run(tree, z, zn, cls, ts, xs, seed, kw)
        except Exception as e:      # (a state the oracle cannot evaluate: next seed)
            print(name, "seed", seed, "failed:", e); continue
        if ref["info"] != 0:
            continue
        margin = min((abs(m[0] - m[1]) for row in ref["trace"] for m in row if not math.isnan(m[1])), default=math.inf)
        if margin < 1e-3:
            continue
        dev, same = 0.0, True
        for k in range(4):
            r = run(tree, z, zn, cls, ts, xs, seed, kw, evalfn=perturbed(ts, xs, np.random.default_rng(77 + k)))
            same = same and decisions(r) == decisions(ref)
            dev = max(dev, deviation(r, ref)) if same else dev
        tol = 8.0 * dev
        if not same or not tol < 1e-6:
            print(name, "seed", seed, "rejected: decisions", same, "tol", tol); continue
        half = dict(kw, eps_param=kw["eps_param"] / 2, L_param=2 * kw["L_param"], n_hmc=1)      # (the same trajectory length: second order)
        a1 = ref["trace"][0][0][0]
        a2 = run(tree, z, zn, cls, ts, xs, seed, half)["trace"][0][0][0]
        ratio = a1 / a2 if a2 != 0 else math.nan
        case = dict(name=name, n=n, tree=tree, cls=[int(c) for c in cls], ts=list(map(float, ts)), xs=list(map(float, xs)), z=z, z_noise=zn,
                    seed=seed, sched=kw, tol=tol, margin=margin, energy=bool(3.5 <= ratio <= 4.5), alpha_ratio_ref=ratio,
                    expect=dict(z=[float(v) for v in ref["z"]], z_noise=float(ref["z_noise"]), prm=[float(v) for v in ref["prm"]],
                                noise=float(ref["noise"]), logpdf=float(ref["logpdf"]), counts=ref["counts"], trace=ref["trace"]))
        if n <= 24 and kw["n_hmc"] == 2:
            MP, eval_mp = H.mp_backend()
            r = run(tree, z, zn, cls, ts, xs, seed, kw, evalfn=eval_mp(ts, xs), ops=MP)
            r = dict(r, z=[float(v) for v in r["z"]], z_noise=float(r["z_noise"]), logpdf=float(r["logpdf"]))
            assert decisions(r) == decisions(ref), name
            case["mp_deviation"] = deviation(r, ref)
        print(f"{name}: seed {seed}, tol {tol:.3e}, margin {margin:.3e}, alpha ratio {ratio:.4f}, counts {ref['counts']}"
              + (f", 60-digit replay deviates by {case['mp_deviation']:.3e}" if "mp_deviation" in case else ""))
        return case
    raise RuntimeError(f"no admissible seed for {name}")


def exit_case():
    """eps = 5 forces rejections: the chain stops after n_exit = 2 consecutive rejected parameter moves"""
    node = G.SquaredExponential(1, 1)
    cls = G.prior.hmc_classes(node)
    kw = dict(n_hmc=5, L_param=3, eps_param=5.0, L_noise=3, eps_noise=0.02, n_exit=2)
    for seed in range(9000, 9050):
        rng = np.random.default_rng(seed)
        ts, xs = G.prior.synthetic_series(17, seed=seed, shuffle=True)
        z = [float(v) for v in 0.5 * rng.standard_normal(len(cls))]; zn = float(0.5 * rng.standard_normal())
        ref = run(node.to_tuple(), z, zn, cls, ts, xs, seed, kw)
        rows = [m for row in ref["trace"] for m in row if not math.isnan(m[1])]
        if ref["counts"][0] == 0 and ref["counts"][1] == 2 and all(abs(m[0] - m[1]) >= 1e-3 for m in rows):
            print("n_exit case: seed", seed, "counts", ref["counts"], "trace", ref["trace"])
            return dict(name="n_exit", n=17, tree=node.to_tuple(), cls=[int(c) for c in cls], ts=list(map(float, ts)), xs=list(map(float, xs)),
                        z=z, z_noise=zn, seed=seed, sched=kw,
                        expect=dict(counts=ref["counts"], trace=ref["trace"], z=[float(v) for v in ref["z"]]))
    raise RuntimeError("no n_exit case")


def notpd_case():
    """a Constant kernel (rank one) with noise_jitter = 0: a noise move at eps = 30 that drives the noise below 1e-17 leaves the positive
    definite region decisively (the second pivot is exactly 0); every noise on the way is either above 1e-12 or below 1e-17"""
    node = G.Constant(1)
    cls = G.prior.hmc_classes(node)
    kw = dict(n_hmc=3, L_param=1, eps_param=0.01, L_noise=2, eps_noise=30.0, n_exit=0)
    for seed in range(9500, 9700):
        rng = np.random.default_rng(seed)
        ts, xs = G.prior.synthetic_series(12, seed=seed, shuffle=True)
        z = [float(0.3 * rng.standard_normal())]; zn = float(0.5 * rng.standard_normal())
        seen = []

        def ev(tree, noise, base=H.eval_oracle(ts, xs)):
            seen.append(noise)
            return base(tree, noise)
        ref = H.hmc_chain(node.to_tuple(), z, zn, cls, TF, seed, kw["n_hmc"], ev, L_param=1, eps_param=0.01, L_noise=2, eps_noise=30.0,
                          n_exit=0, jitter=0.0)
        rows = [m for row in ref["trace"] for m in row if not math.isnan(m[1])]
        decisive = all(v > 1e-12 or v < 1e-17 for v in seen) and all(math.isfinite(v) for v in seen)
        if ref["counts"][3] >= 1 and decisive and all(abs(m[0] - m[1]) >= 1e-3 for m in rows):
            print("not-PD case: seed", seed, "counts", ref["counts"])
            return dict(name="notpd", n=12, tree=node.to_tuple(), cls=[int(c) for c in cls], ts=list(map(float, ts)), xs=list(map(float, xs)),
                        z=z, z_noise=zn, seed=seed, sched=kw, jitter=0.0,
                        expect=dict(counts=ref["counts"], trace=ref["trace"], z=[float(v) for v in ref["z"]], z_noise=float(ref["z_noise"])))
    raise RuntimeError("no not-PD case")


def main():
    cases = [make_case(*s, idx=i) for i, s in enumerate(SHAPES)]
    assert sum(c["energy"] for c in cases) >= 3, "too few cases for the energy check"
    out = dict(version=1, perturbation=PERT, tf=TF.tolist(), cases=cases, exit_case=exit_case(), notpd_case=notpd_case())
    path = Path(__file__).with_name("series_hmc_v1.json")
    path.write_text(json.dumps(out, indent=0, allow_nan=True) + "\n")
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
