"""The Schur (Toeplitz) kernels on caller-supplied first columns (GPEngine.debug_toeplitz: launch_toep_logpdf itself — the value,
gradient and predictive instantiations of k_toep_logpdf and k_toep_back — on programs and rank-layout tables built from the
arguments, every output seeded with the sentinel -7).  Families, targets, routes, metrics and bounds: tests/_toeplitz_probe_ref.py;
the conditions on the inputs and the planted faults: tests/test_toeplitz_probe_cpu.py.

A case is ONE call with every family stacked, four particles per family (VARIANTS of the reference module: 0, 1 and 2 Linear
leaves, centres at, left of and far right of t_ref, one leaf with zero amplitude; the last variant has its table split in two):

  1. L (packed columns, identical bits for a family's four particles): eta <= 4 max(R, 2 gamma_{n+1});
  2. fwd and sol: omega_solve of both substitutions against L as the device stored it, <= 4 max(R_s or R_b, 2 gamma_n);
  3. log|T| (from the stored diagonal), b_x'b_x (from fwd), out_lp of every variant, every row of pacc and sol against the
     longdouble target: <= 8 max(R, floor) and never above the conditioning cap;
  4. the sentinel wherever the layout stores nothing;
  5. mode 0 runs with rank0 = 5, modes 1 and 2 with rank0 = 0.

Then: refusal at a planted column, isolation and determinism, argument errors, and the probe against logpdf_batch on real kernels.
Figures of one MI355X run: profiles/toeplitz_probe_accuracy.txt (tools/gpu_toeplitz_probe_accuracy.py)."""
import numpy as np
import pytest

import _factor_ref as F
import _toeplitz_probe_ref as T

pytestmark = pytest.mark.gpu

S = T.SENTINEL
NV = len(T.VARIANTS)
_RUNS = {}


def stacked_inputs(fams, n, N):
    """arguments of debug_toeplitz for the families' four variants each"""
    P = len(fams) * NV
    r = np.zeros((P, N)); r2 = np.zeros((P, N)); mask = np.zeros(P, dtype=bool)
    noise = np.zeros(P); const = np.full(P, np.nan); wn = np.full(P, np.nan); lin = []
    for f, fam in enumerate(fams):
        d = T.family(fam, n, N)
        for vi, leaves in enumerate(T.VARIANTS):
            p = f * NV + vi
            if vi == T.SPLIT_VARIANT:
                r[p], r2[p] = T.split_tables(d["tab"]); mask[p] = True
            else:
                r[p] = d["tab"]
            noise[p], const[p], wn[p] = d["noise"], d["const"], d["wn"]
            lin.append(list(leaves))
    return dict(r=r, r2=(mask, r2[mask]), noise=noise, const=const, wn=wn, lin=lin)


def run(engine, mode, n, m, fams=T.FAMILIES):
    key = (mode, n, m, fams)
    if key not in _RUNS:
        N = n + m
        a = stacked_inputs(fams, n, N)
        h, mid = T.grid_of(n)
        rank0 = T.RANK0_MODE0 if mode == 0 else 0
        out = engine.debug_toeplitz(mode, a["r"], T.rhs_x(n), a["noise"], m_future=m, r2=a["r2"], const=a["const"], wn=a["wn"], lin=a["lin"],
                                    rank0=rank0, grid_h=h, grid_mid=mid, t_ref=T.T_REF)
        for v in out.values():
            v.setflags(write=False)
        _RUNS[key] = (out, rank0)
    return _RUNS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_case(out, rank0, mode, n, m, fams, tag="toeplitz-probe"):
    """failures of checks 1 to 4 of a case; prints every figure"""
    fails = []
    N = n + m
    tri = n * (n + 1) // 2
    g1, g0 = F.gamma(n + 1), F.gamma(n)
    if not (out["info"] == 0).all():
        return [f"info = {out['info']}"]
    for f, fam in enumerate(fams):
        ref = T.reference(fam, mode, n, m, rank0)
        tg, bound = ref["tg"], ref["bound"]
        p0 = f * NV
        res = dict(lps={vi: out["lp"][p0 + vi] for vi in range(NV)})
        if mode >= 1:
            L, guard_ok = T.unpack_columns(out["Lcols"][p0 + 1], n)
            packed = out["Lcols"][p0 + 1][:tri]
            if not guard_ok:
                fails.append(f"{fam}: the doubles after the packed triangle were written")
            if not np.isfinite(packed).all() or (packed == S).any():
                fails.append(f"{fam}: an entry of the packed triangle is not finite, or was never written")
            for vi in range(NV):
                if not same_bits(out["Lcols"][p0 + vi], out["Lcols"][p0 + 1]):
                    fails.append(f"{fam}: variant {vi} has other bits in L than variant 1")
                lin_v = vi > 0
                rows = slice(0, 4) if lin_v else slice(0, 2)
                if vi != 1 and not (same_bits(out["fwd"][p0 + vi, rows, :n], out["fwd"][p0 + 1, rows, :n]) and same_bits(out["sol"][p0 + vi, rows, :n], out["sol"][p0 + 1, rows, :n])):
                    fails.append(f"{fam}: variant {vi} has other bits in fwd or sol than variant 1")
                if not ((out["fwd"][p0 + vi, :, n:] == S).all() and (out["sol"][p0 + vi, :, n:] == S).all()):
                    fails.append(f"{fam}: variant {vi}: fwd or sol written beyond n")
                if (out["fwd"][p0 + vi, rows, :n] == S).any() or (out["sol"][p0 + vi, rows, :n] == S).any():
                    fails.append(f"{fam}: variant {vi}: an entry of fwd or sol below n still holds the sentinel")
            fwd, sol = out["fwd"][p0 + 1, :, :n], out["sol"][p0 + 1, :, :n]
            res.update(L=L, fwd=fwd, sol=sol, logdet=2 * np.log(np.diag(L).astype(T.LD)).sum(), qxx=fwd[0].astype(T.LD) @ fwd[0].astype(T.LD))
        if mode == 2:
            for vi in range(NV):
                pr = [0, 1, 2, 3] if vi > 0 else [0, 3]
                if vi != 1 and not same_bits(out["pacc"][p0 + vi, pr, :m], out["pacc"][p0 + 1, pr, :m]):
                    fails.append(f"{fam}: variant {vi} has other bits in pacc than variant 1")
                if not (out["pacc"][p0 + vi, :, m:] == S).all():
                    fails.append(f"{fam}: variant {vi}: pacc written beyond m")
            res["pacc"] = out["pacc"][p0 + 1, :, :m]
        e = T.quantities(tg, res, T.VARIANTS, True)
        if mode >= 1:
            e["eta"] = T.eta_of(ref["r_eff"], res["L"])
        line = []
        for k, v in e.items():
            unit = g1 if k == "eta" else g0 if k.startswith("solve") else 1.0
            line.append(f"{k} {v / unit:.3g} (R {ref['R'][k] / unit:.3g}, bound {bound[k] / unit:.3g})")
            if not v <= bound[k]:
                fails.append(f"{fam}: {k} = {v / unit:.4g} above the bound {bound[k] / unit:.4g} (R = {ref['R'][k] / unit:.4g})")
        print(f"[{tag}] mode {mode} n {n} m {m} {fam:9s}: " + "  ".join(line))
    return fails


@pytest.mark.parametrize("n", T.SIZES_01 + T.SIZES_0_BIG)
def test_value_sweep(engine, n):
    out, rank0 = run(engine, 0, n, 0)
    fails = check_case(out, rank0, 0, n, 0, T.FAMILIES)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", T.SIZES_01)
def test_gradient_sweep(engine, n):
    out, rank0 = run(engine, 1, n, 0)
    fails = check_case(out, rank0, 1, n, 0, T.FAMILIES)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n, m", T.SIZES_2)
def test_predictive_sweep(engine, n, m):
    out, rank0 = run(engine, 2, n, m)
    fails = check_case(out, rank0, 2, n, m, T.FAMILIES)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode, n, m", [(1, 2048, 0), (2, 2048, 2048)])
def test_all_registers_full(engine, mode, n, m):
    """eta over the fixed sample of entries (sample_entries), the solves in full"""
    out, rank0 = run(engine, mode, n, m, T.BIG_FAMILIES)
    fails = check_case(out, rank0, mode, n, m, T.BIG_FAMILIES)
    assert not fails, "\n".join(fails)


# ---- refusal at a chosen column ----------------------------------------------------------------------------------------------------
PLANT_N = 600
PLANT_COLS = (1, 2, 255, 256, 257, 511, 512, PLANT_N - 1)
PLANT_VALUES = ((1 + T.LD("1e-9"), False), (-(1 + T.LD("1e-9")), False), (T.LD(1), True), (T.LD(-1), True))
_PLANTED = {}


def planted(N, k, value, quiet):
    key = (N, k, float(value), float(value - 1), quiet)
    if key not in _PLANTED:
        _PLANTED[key] = np.asarray(T.inverse_schur(T.planted_rho(N, k, value, quiet)), dtype=np.float64)
    return _PLANTED[key]


def planted_batch(mode):
    """(n, m, rows, kind) of the planted-column call of a mode"""
    n, m = (520, 80) if mode == 2 else (PLANT_N, 0)
    N = n + m
    cols = PLANT_COLS if mode < 2 else tuple(k for k in PLANT_COLS if k < n - 1) + (n - 1, n, 560, N - 1)
    rows, kind = [], []
    for k in cols:
        for value, quiet in PLANT_VALUES:
            rows.append(planted(N, k, value, quiet)); kind.append(("refused", k))
        rows.append(planted(N, k, 1 - T.LD("1e-12"), True)); kind.append(("accepted", k))
    rows.append(np.ones(N)); kind.append(("refused", 1))                       # all-ones column, zero noise: rho_1 = 1
    nan_row = planted(N, 300, T.LD("0.5"), False).copy(); nan_row[400] = np.nan
    rows.append(nan_row); kind.append(("refused", 400))
    return n, m, np.stack(rows), kind


def planted_run(engine, mode):
    key = ("planted", mode)
    if key not in _RUNS:
        n, m, r, kind = planted_batch(mode)
        _RUNS[key] = (n, m, r, kind, engine.debug_toeplitz(mode, r, T.rhs_x(n), 0.0, m_future=m))
    return _RUNS[key]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_refusal_at_a_planted_column(engine, mode):
    """|rho_k| = 1 + 1e-9 (behind seeded coefficients in +-0.05) and exactly 1 (behind zeros: only then is the planted value what the
    arithmetic sees) at the columns where the owner of the pivot changes thread, register or buffer, and in mode 2 at future columns;
    an all-ones column with zero noise; a NaN entry.  The same call holds the accepted columns of the next test."""
    n, m, r, kind, out = planted_run(engine, mode)
    fails = []
    for p, (what, k) in enumerate(kind):
        if what != "refused":
            continue
        if not (out["info"][p] == 1 and np.isnan(out["lp"][p])):
            fails.append(f"particle {p} (column {k}): info {out['info'][p]}, lp {out['lp'][p]} instead of a refusal")
        if mode >= 1 and not (out["sol"][p] == S).all():
            fails.append(f"particle {p} (column {k}): refused, but sol was written")
        if mode == 2 and not (out["pacc"][p] == S).all():
            fails.append(f"particle {p} (column {k}): refused, but pacc was written")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_near_singular_planted_column_is_accepted(engine, mode):
    """|rho_k| = 1 - 1e-12 behind zeros at the same columns (in mode 2 the future columns n, 560 and N - 1 too, where the training
    block is the identity and the plant shows in the rows of pacc alone): accepted, and every quantity within the bounds of its own
    routes.  The
    condition number is 1e12, beyond the longdouble recursion (it leaves the Schur complement's diagonal 6.5e-21 off where the bound
    is 1.5e-22 and the device, whose fused multiply-adds keep the residues r_j - rho r_(j-1) of the rounded column, is within 1.3e-23):
    the target of these cases is the recursion in 80-digit decimal arithmetic (target_hp)."""
    n, m, r, kind, out = planted_run(engine, mode)
    x = T.rhs_x(n)
    fails = []
    for p, (what, k) in enumerate(kind):
        if what != "accepted":
            continue
        if out["info"][p] != 0:
            fails.append(f"particle {p} (column {k}, 1 - 1e-12): refused")
            continue
        if mode >= 1 and not ((out["fwd"][p, :, n:] == S).all() and (out["sol"][p, :, n:] == S).all() and (out["Lcols"][p, n * (n + 1) // 2:] == S).all()):
            fails.append(f"column {k} (1 - 1e-12): fwd, sol or L written where the layout stores nothing")
        if mode == 2 and not ((out["pacc"][p, :, m:] == S).all() and (out["pacc"][p, [0, 3], :m] != S).all()):
            fails.append(f"column {k} (1 - 1e-12): pacc written beyond m, or not written below it")
        ref = T.build_reference(r[p], x, n, m, 0, mode >= 1, leaves_list=T.VARIANTS[:1], hp=True)
        assert ref["admitted"]
        res = dict(lps={0: out["lp"][p]})
        if mode >= 1:
            L, guard_ok = T.unpack_columns(out["Lcols"][p], n)
            fwd, sol = out["fwd"][p, :, :n], out["sol"][p, :, :n]
            res.update(L=L, fwd=fwd, sol=sol, logdet=2 * np.log(np.diag(L).astype(T.LD)).sum(), qxx=fwd[0].astype(T.LD) @ fwd[0].astype(T.LD))
        if mode == 2:
            res["pacc"] = out["pacc"][p, :, :m]
        e = T.quantities(ref["tg"], res, T.VARIANTS[:1], False)
        if mode >= 1:
            e["eta"] = T.eta_of(r[p], res["L"])
        for name, v in e.items():
            print(f"[toeplitz-probe] planted 1 - 1e-12 at column {k}, mode {mode}: {name} {v:.3g} (R {ref['R'][name]:.3g}, bound {ref['bound'][name]:.3g})")
            if not v <= ref["bound"][name]:
                fails.append(f"column {k} (1 - 1e-12): {name} = {v:.4g} above the bound {ref['bound'][name]:.4g}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("opcode", [3, 7, 8, 11, 200])        # SE kept in its direct form, Times, ChangePoint, the tabled GE leaf, no opcode at all
def test_foreign_opcode_is_refused(engine, mode, opcode):
    n, m = 17, (3 if mode == 2 else 0)
    d = T.family("ge1", n, n + m)
    r = np.stack([d["tab"]] * 3)
    x = T.rhs_x(n)
    good = engine.debug_toeplitz(mode, r, x, d["noise"], m_future=m)
    out = engine.debug_toeplitz(mode, r, x, d["noise"], m_future=m, raw=(1, opcode))
    assert list(out["info"]) == [0, 1, 0] and np.isnan(out["lp"][1])
    for k, v in out.items():
        if k in ("lp", "info"):
            assert same_bits(v[[0, 2]].astype(np.float64), good[k][[0, 2]].astype(np.float64))
        else:
            assert (v[1] == S).all(), f"{k} of the refused particle was written"
            assert same_bits(v[[0, 2]], good[k][[0, 2]]), f"{k} of a neighbour changed"


# ---- isolation and determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, n, m", [(0, 300, 0), (1, 300, 0), (2, 255, 45), (0, 2049, 0)])
def test_isolation_and_determinism(engine, mode, n, m):
    """two particles of the batch (one per family) refused: the others are bit for bit what the all-good batch gives, what P = 1 calls give and what
    a second call gives"""
    N = n + m
    fams = T.FAMILIES
    cols = [T.family(f, n, N) for f in fams]
    kw = dict(m_future=m, const=np.array([c["const"] for c in cols]), wn=np.array([c["wn"] for c in cols]),
              lin=[list(T.VARIANTS[i % NV]) for i in range(len(fams))], grid_h=T.grid_of(n)[0], grid_mid=T.grid_of(n)[1], t_ref=T.T_REF)
    r = np.stack([c["tab"] for c in cols]); noise = np.array([c["noise"] for c in cols])
    x = T.rhs_x(n)
    good = engine.debug_toeplitz(mode, r, x, noise, **kw)
    assert (good["info"] == 0).all()
    bad = r.copy()
    bad[2] = planted(N, min(257, n - 1), 1 + T.LD("1e-9"), False)      # (ma1's slot: noise 0 and no leaves, so r0 stays 1)
    bad[6] = np.nan
    mixed = engine.debug_toeplitz(mode, bad, x, noise, **kw)
    again = engine.debug_toeplitz(mode, bad, x, noise, **kw)
    keep = [p for p in range(len(fams)) if p not in (2, 6)]
    assert list(mixed["info"]) == [0 if p in keep else 1 for p in range(len(fams))]
    for k in good:
        assert np.array_equal(np.ascontiguousarray(mixed[k]).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8)), f"{k}: two identical calls differ"
        assert np.array_equal(np.ascontiguousarray(mixed[k][keep]).view(np.uint8), np.ascontiguousarray(good[k][keep]).view(np.uint8)), f"{k}: a refused neighbour changed a particle's bits"
    for p in keep:
        one = engine.debug_toeplitz(mode, r[p:p + 1], x, noise[p:p + 1], m_future=m, const=kw["const"][p:p + 1], wn=kw["wn"][p:p + 1],
                                    lin=kw["lin"][p:p + 1], grid_h=kw["grid_h"], grid_mid=kw["grid_mid"], t_ref=T.T_REF)
        for k in good:
            assert np.array_equal(np.ascontiguousarray(one[k]).view(np.uint8), np.ascontiguousarray(good[k][p:p + 1]).view(np.uint8)), f"{k} of {fams[p]}: the batch and the particle alone differ"


# ---- argument errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg, engine):
    import ctypes as C
    lib, ctx = engine._lib, engine._ctx
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    big = np.zeros(4096 * 2 + 64); lp = np.zeros(4); info = np.zeros(4, dtype=np.int32)
    leaves = np.zeros(1, dtype=np.int32)

    def call(mode=0, n=17, nj=0, P=1, r=big, leaves=None, noise=big, x=big, raw_p=-1, raw_op=0, lp=lp, info=info, Lc=None, fw=None, so=None, pa=None):
        arg = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
        return lib.agp_debug_toeplitz(ctx, mode, n, nj, P, arg(r, dp), None, arg(leaves, ip), None, None, None, arg(noise, dp), arg(x, dp), 0, 1.0, 0.0,
                                      0.0, raw_p, raw_op, arg(lp, dp), arg(info, ip), arg(Lc, dp), arg(fw, dp), arg(so, dp), arg(pa, dp))

    out = np.zeros(1 << 16)
    bad = [dict(mode=3), dict(mode=-1), dict(n=0), dict(n=4097), dict(P=0), dict(P=4097), dict(nj=18), dict(r=None), dict(noise=None), dict(x=None),
           dict(lp=None), dict(info=None),
           dict(mode=1, n=2049, Lc=out, fw=out, so=out),                      # STORE above 2048 points
           dict(mode=2, n=2049, nj=2050, Lc=out, fw=out, so=out, pa=out),
           dict(mode=2, n=17, nj=4097, Lc=out, fw=out, so=out, pa=out),        # joint grid above 4096 points
           dict(mode=2, n=17, nj=16, Lc=out, fw=out, so=out, pa=out),          # inconsistent: nj < n
           dict(mode=2, n=17, nj=0, Lc=out, fw=out, so=out, pa=out),
           dict(mode=1, n=17, nj=20, Lc=out, fw=out, so=out),                  # nj belongs to mode 2
           dict(mode=1), dict(mode=2, nj=20, Lc=out, fw=out, so=out),          # missing output arrays
           dict(leaves=leaves + 1), dict(leaves=leaves + 2), dict(leaves=leaves + 8), dict(leaves=leaves + 24), dict(leaves=leaves + 32),
           dict(raw_p=1), dict(raw_p=0, raw_op=256), dict(raw_p=0, raw_op=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw                                   # AGP_ERR_ARG
    big[:17] = T.family("ge1", 17)["tab"]
    noise = np.full(4, 1e-6)
    assert call(noise=noise) == 0 and info[0] == 0 and np.isfinite(lp[0])
    out, rank0 = run(engine, 1, 17, 0)
    assert not check_case(out, rank0, 1, 17, 0, T.FAMILIES)


# ---- the probe is the production code ------------------------------------------------------------------------------------------------------
def test_probe_matches_the_structured_value_sweep(pkg):
    """real kernels on a regular grid: the first column from agp_cov_matrix of the kernel without its Linear leaf (column 0 in
    sorted order), the Linear leaf passed through — out_lp must equal logpdf_batch's under set_lag_tables(3), bit for bit"""
    G = pkg
    n = 300
    ts = np.linspace(0.0, 1.0, n)
    xs = np.random.default_rng(77).standard_normal(n)
    se, per = G.SquaredExponential(0.13, 0.8), G.Periodic(0.7, 0.21, 1.1)
    lin = G.Linear(0.31, 0.2, 0.9)
    stat = [se, se + per, se + G.Constant(0.4), se + per + G.Constant(0.4)]
    nodes = stat + [s + lin for s in stat]
    lins = [[]] * len(stat) + [[(0.31, 0.2, 0.9)]] * len(stat)
    noises = np.linspace(0.02, 0.2, len(nodes))
    lat = G.probe_lattice(ts)
    assert lat["kind"] == 1 and lat["n_lattice"] == n
    eng = G.GPEngine(0)
    try:
        eng.set_lag_tables(3)
        eng.set_data(ts, xs)
        lp, info = eng.logpdf_batch(nodes, noises, check=False)
        assert eng.toeplitz_particles() == len(nodes) and (info == 0).all()
        r = np.stack([eng.cov_matrix(s, 0.0, ts)[:, 0] for s in stat] * 2)
        out = eng.debug_toeplitz(0, r, xs, noises, lin=lins, rank0=0, grid_h=lat["spacing"], grid_mid=0.5 * (n - 1), t_ref=0.5 * (ts[0] + ts[-1]))
    finally:
        eng.close()
    assert (out["info"] == 0).all()
    print("[toeplitz-probe] probe - logpdf_batch:", out["lp"] - lp)
    assert same_bits(out["lp"], lp), (out["lp"] - lp)
