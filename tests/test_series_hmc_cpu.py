"""CPU tests of the HMC entry's reference (tests/_series_hmc_ref.py) and of what the Python layer adds for it: the Philox counter layout
against numpy.random.Philox; the transforms and their derivatives against prior.py and finite differences; the reference chain against
a 60-digit replay of the same draws on a tiny case (the larger tiny cases' replays are recorded in the golden file by its generator);
the golden file's admission rules; n_exit bookkeeping; the LDS-fit arithmetic."""
import json
import math
import re
from pathlib import Path

import numpy as np

import _pred_sample_ref as PR
import _series_grad_ref as GR
import _series_hmc_ref as H

ROOT = Path(__file__).resolve().parents[1]
GOLD = json.loads((Path(__file__).parent / "golden" / "series_hmc_v1.json").read_text())


def test_counter_layout_against_numpy_philox():
    seed, it = 0x1234567890ABCDEF, 3
    for mv in (0, 1):
        for k in (0, 1, 3, 4, 9):
            ctr = np.array([k // 4, it, mv, H.TAG], dtype=np.uint64)
            v = sum(int(c) << (64 * i) for i, c in enumerate(ctr)) - 1      # (numpy advances the counter before its first block)
            g = np.random.Philox(key=np.array([seed, 0], dtype=np.uint64), counter=np.array([(v >> (64 * i)) & PR.MASK64 for i in range(4)], dtype=np.uint64))
            w = int(g.random_raw(4)[k % 4])
            from scipy.special import ndtri
            assert H.momentum(seed, it, mv, k) == float(ndtri(PR.uniform(w)))
        assert H.log_u(seed, it, mv) == math.log(PR.uniform(PR.philox_block(seed, 1 << 32, it, mv, 0x484D43)[0]))
    assert H.momentum(seed, it, 0, 0) != H.momentum(seed, it, 1, 0) != H.momentum(seed + 1, it, 1, 0)


def test_transforms_and_derivatives(pkg):
    pr = pkg.prior
    tf = pr.hmc_transform_table()
    assert tf.tolist() == [[-1.5, 1.0, 0.0], [-1.5, 1.0, 0.0], [0.0, 1.0, 2.0]]
    custom = pr.hmc_transform_table({"wildcard": {"mu": -1.0, "sigma": 0.5}, "period": {"mu": 0.2, "sigma": 2.0}, "gamma": {"mu": 0.1, "sigma": 0.7, "scale": 1.5}})
    for z in (-2.3, -0.4, 0.0, 0.9, 3.1):
        assert H.transform(z, 0, tf) == pr.transform_param("lengthscale", z) and H.transform(z, 1, tf) == pr.transform_param("period", z)
        assert H.transform(z, 2, tf) == pr.transform_param("gamma", z) and H.transform(z, -1, tf) == z
        for t in (tf, custom):
            for c in (0, 1, 2):
                th = H.transform(z, c, t)
                assert th == pr.hmc_transform(z, c, t) and abs(pr.hmc_untransform(th, c, t) - z) <= 1e-12 * max(1.0, abs(z))
                h = 1e-6
                fd = (H.transform(z + h, c, t) - H.transform(z - h, c, t)) / (2 * h)
                assert abs(H.dtheta(th, c, t) - fd) <= 1e-8 * max(1.0, abs(fd)), (z, c)
    nd = pkg.ChangePoint(pkg.Linear(0.2, 0.3, 0.4), pkg.GammaExponential(0.4, 1.2, 0.7) * pkg.Periodic(0.5, 0.6, 0.7), 0.5, 0.001)
    assert pr.hmc_classes(nd).tolist() == [0, 0, 0, 0, 2, 0, 0, 1, 0, 0, -1]
    assert pkg.with_params(nd, pkg.encode(nd)[1]) == nd
    moved = pkg.with_params(nd, 0.1 * np.arange(1.0, 12.0))
    assert pkg.encode(moved)[1].tolist() == list(0.1 * np.arange(1.0, 12.0)) and np.array_equal(pkg.encode(moved)[0], pkg.encode(nd)[0])


def test_reference_chain_against_60_digit_replay(pkg):
    """the same draws, the whole chain in 60-digit arithmetic (value by oracle_mp, gradient by central differences there): the fp64
    reference's decisions are the replay's and its state deviates by rounding only; the golden file records the same for its tiny cases"""
    G = pkg
    node = G.SquaredExponential(1, 1) + G.Linear(1, 1, 1)
    cls = G.prior.hmc_classes(node)
    tf = G.prior.hmc_transform_table()
    ts, xs = (a[:8].copy() for a in G.prior.synthetic_series(32, seed=5, shuffle=True))
    z, zn, seed = [0.3, -0.2, 0.1, 0.4, -0.5], 0.2, 77
    kw = dict(L_param=3, eps_param=0.02, L_noise=3, eps_noise=0.02)
    ref = H.hmc_chain(node.to_tuple(), z, zn, cls, tf, seed, 2, H.eval_oracle(ts, xs), **kw)
    MP, eval_mp = H.mp_backend()
    rep = H.hmc_chain(node.to_tuple(), z, zn, cls, tf, seed, 2, eval_mp(ts, xs), ops=MP, **kw)
    assert ref["counts"] == rep["counts"] and ref["counts"][1] == 2 and ref["evals"][0] == 2 + 4 * 4
    dev = max([abs(a - float(b)) for a, b in zip(ref["z"], rep["z"])] + [abs(ref["z_noise"] - float(rep["z_noise"])), abs(ref["logpdf"] - float(rep["logpdf"]))]
              + [abs(a[0] - b[0]) for ra, rb in zip(ref["trace"], rep["trace"]) for a, b in zip(ra, rb)])
    print(f"[series-hmc] fp64 reference against the 60-digit replay: {dev:.3e}")
    assert dev <= 1e-12
    tiny = [c for c in GOLD["cases"] if "mp_deviation" in c]
    assert len(tiny) == 2 and all(c["n"] <= 24 and c["sched"]["n_hmc"] == 2 and c["sched"]["L_param"] == 3 and c["mp_deviation"] <= 1e-12 for c in tiny)


def test_golden_admission_rules():
    assert GOLD["perturbation"] == 1e-11
    assert sorted(c["n"] for c in GOLD["cases"]) == [1, 12, 15, 16, 17, 24, 33, 49, 144, 176]
    for c in GOLD["cases"]:
        rows = [m for row in c["expect"]["trace"] for m in row if not math.isnan(m[1])]
        assert rows and all(abs(m[0] - m[1]) >= 1e-3 for m in rows) and 0.0 < c["tol"] < 1e-6, c["name"]
        assert c["energy"] == (3.5 <= c["alpha_ratio_ref"] <= 4.5)
    assert sum(c["energy"] and c["sched"]["n_hmc"] == 3 for c in GOLD["cases"]) >= 3


def test_n_exit_bookkeeping():
    """a stub evaluation whose trajectories always fail: every parameter move is rejected; the chain stops after n_exit of them in a
    row, the noise move of the stopping iteration still runs, n_exit <= 0 never stops, a particle without a moving parameter never stops"""
    tf = [[-1.5, 1.0, 0.0]]
    calls = []

    def ev(tree, noise):
        calls.append(tree)
        first = len(calls) == 1 or tree[1] == math.exp(-1.5)      # the start state evaluates, whatever moved does not
        return (-1.0, [0.0], 0.0, 0) if first else (math.nan, None, math.nan, 3)
    kw = dict(L_param=1, eps_param=0.5, L_noise=0, eps_noise=0.1)
    r = H.hmc_chain(("C", 1.0), [0.0], 0.0, [0], tf, 1, 6, ev, n_exit=2, **kw)
    assert r["counts"] == [0, 2, 0, 2] and [math.isnan(row[0][1]) for row in r["trace"]] == [False, False, True, True, True, True]
    assert r["z"] == [0.0] and all(math.isnan(row[1][1]) for row in r["trace"])
    calls.clear()
    assert H.hmc_chain(("C", 1.0), [0.0], 0.0, [0], tf, 1, 6, ev, n_exit=0, **kw)["counts"] == [0, 6, 0, 6]
    calls.clear()
    assert H.hmc_chain(("C", 1.0), [0.0], 0.0, [0], tf, 1, 6, ev, **kw)["counts"] == [0, 6, 0, 6]      # default: n_exit = n_hmc
    calls.clear()
    # no moving parameter: no parameter move, the counter never advances, the noise moves all run
    ok = lambda tree, noise: (-1.0, [0.0], 0.0, 0)
    r = H.hmc_chain(("C", 1.0), [1.0], 0.0, [-1], tf, 1, 4, ok, n_exit=1, L_param=1, eps_param=0.5, L_noise=1, eps_noise=0.1)
    assert r["counts"][:2] == [0, 0] and not any(math.isnan(row[1][1]) for row in r["trace"]) and all(math.isnan(row[0][1]) for row in r["trace"])
    assert r["z"] == [1.0] and r["prm"] == [1.0]
    e = GOLD["exit_case"]
    assert e["expect"]["counts"][:2] == [0, 2] and e["sched"]["n_exit"] == 2 and e["sched"]["eps_param"] == 5.0


def test_lds_fit_arithmetic_against_the_header():
    """series_hmc_lds of csrc/agp_args.hpp restated in _series_hmc_ref.py: the constants are read out of the header, and the boundary the
    C header states — a chain of 4 ChangePoint nodes at 176 points fits, 5 do not — follows from them"""
    src = (ROOT / "autogp.jl_amd" / "csrc" / "agp_args.hpp").read_text()
    assert int(re.search(r"constexpr int HMC_ST_N = (\d+);", src).group(1)) == H.HMC_ST_N
    body = src[src.index("inline SeriesHmcLds series_hmc_lds("):]
    body = body[:body.index("return m;")]
    for frag in ("const int npc = (g_n_prm + 1) & ~1;", "m.o_z = m.o_th + npc", "m.o_zs = m.o_z + npc", "m.o_mom = m.o_zs + npc", "m.o_grd = m.o_mom + npc",
                 "m.o_cls = m.o_grd + npc", "m.o_tf = m.o_cls + npc", "m.o_st = m.o_tf + ((3 * C + 1) & ~1)", "m.o_blk = m.o_st + HMC_ST_N"):
        assert frag in body, frag
    assert H.series_hmc_lds_total(176, 9, 13, 4, 9, 13, 3) == GR.series_grad_lds_total(176, 9, 13, 4, 9, 13) + 6 * 14 + 10 + 32
    assert H.cp_chain_fits_hmc(4, 176) and not H.cp_chain_fits_hmc(5, 176) and H.cp_chain_fits_hmc(5, 100)
    assert max(k for k in range(1, 40) if H.cp_chain_fits_hmc(k, 176)) == max(k for k in range(1, 40) if GR.cp_chain_fits(k, 176, grad=True))
    assert "a chain of 4\n *     ChangePoint nodes still fits and one of 5 does not" in (ROOT / "include" / "autogp_hip.h").read_text()
