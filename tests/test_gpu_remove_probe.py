"""The removal update of resident factors on caller-supplied factors (GPEngine.debug_remove_factor: agp_remove_data's own host
function and kernels on arrays of the store's layout).  Inputs, targets, metrics and bounds: tests/_remove_probe_ref.py; the
conditions on the inputs and the planted faults: tests/test_remove_probe_cpu.py.  Every case is one call with the six families'
factors of one size and one removal pattern, made once and shared by the checks:

  1. row-wise backward error of L' and of alpha' against the 80-bit target, eta <= 4 max(R, 2 gamma_{n'+1}),
     eta_s <= 4 max(R_s, 2 gamma_{n'}), R from the two reference routes on the same input;
  2. what must not change, bit for bit: rows and columns before the first removed position a, alpha before a, the sentinel in
     the partials and inverse blocks of the tile columns before a // 128 — and everything where the update returns early;
  3. the shape of the slot: exactly lower triangular, exactly the identity from n' on, alpha zero there, positive diagonal, info 0;
  4. the log-det and quadratic-form partials of the rewritten tile columns against the L' and alpha' they came from (16 u: one
     1-ulp log, seven butterfly levels and the first pair sum, doubled);
  5. the inverses of the 16 x 16 pivot blocks against their blocks: |L_bb X - I| <= gamma_16 |L_bb| |X| (substitution, Higham
     Theorem 8.5), X lower triangular, the identity on the padding;
  6. isolation and repeatability: the batch, its reverse and each factor alone give the same bits, and so do two calls; a probe
     call between remove_data / logpdf_batch_extend sequences changes neither their results nor the engine's counters;
  7. the argument errors, each followed by a call that still passes check 1.

Figures of one MI355X run: profiles/remove_probe_accuracy.txt (tools/gpu_remove_probe_accuracy.py)."""
import ctypes as C

import numpy as np
import pytest

import _factor_ref as F
import _remove_probe_ref as P

pytestmark = pytest.mark.gpu

U = F.U
_RUNS = {}


def run(engine, n, name):
    """(L0, alpha0, (L, alpha, partial, winv, info)) of a case: one call, cached, read-only"""
    if (n, name) not in _RUNS:
        L0, a0 = P.batch_inputs(n, name)
        out = engine.debug_remove_factor(L0, a0, P.PATTERNS[n][name])
        for x in (L0, a0) + tuple(out):
            x.setflags(write=False)
        _RUNS[(n, name)] = (L0, a0, out)
    return _RUNS[(n, name)]


def backward_errors(n, name, L, alpha, members=range(len(P.FAMILIES))):
    """failures of check 1 for the members of a case's batch; prints every figure"""
    fails = []
    for j, i in enumerate(members):
        fam = P.FAMILIES[i]
        ref = P.reference(fam, n, name)
        m = ref["n_new"]
        g1, g0 = F.gamma(m + 1), F.gamma(m)
        e, es = P.eta(ref["M"], L[j, :m, :m]), P.eta_s(L[j, :m, :m], alpha[j, :m], ref["y"])
        print(f"[remove-probe] n {n} {name:13s} {fam:9s}: eta {e / g1:.4f} gamma (R {ref['R'] / g1:.4f}, bound {ref['bound'] / g1:.3f})  "
              f"eta_s {es / g0:.4f} gamma (R_s {ref['R_s'] / g0:.4f}, bound {ref['bound_s'] / g0:.3f})")
        if not e <= ref["bound"]:
            fails.append(f"{fam}: eta = {e / g1:.4g} gamma_(n'+1) above the bound {ref['bound'] / g1:.4g} (R = {ref['R'] / g1:.4g})")
        if not es <= ref["bound_s"]:
            fails.append(f"{fam}: eta_s = {es / g0:.4g} gamma_n' above the bound {ref['bound_s'] / g0:.4g} (R_s = {ref['R_s'] / g0:.4g})")
    return fails


@pytest.mark.parametrize("n, name", P.CASES)
def test_backward_error(engine, n, name):
    _, _, (L, alpha, _, _, info) = run(engine, n, name)
    assert (info == 0).all(), info
    fails = backward_errors(n, name, L, alpha)
    assert not fails, "\n".join(fails)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n, name", P.CASES)
def test_untouched_parts_are_bit_identical(engine, n, name):
    L0, a0, (L, alpha, part, winv, info) = run(engine, n, name)
    idx = P.PATTERNS[n][name]
    keep = P.keep_of(n, idx)
    a, m = idx[0], n - len(idx)
    fails = []
    for p, fam in enumerate(P.FAMILIES):
        low0 = np.tril(L0[p])
        if not same_bits(L[p, :a, :a], low0[:a, :a]):
            fails.append(f"{fam}: rows and columns before a = {a} changed")
        if not same_bits(L[p, a:m, :a], low0[keep[a:], :a]):
            fails.append(f"{fam}: the columns before a = {a} of the rows that moved up are not the old rows'")
        if not same_bits(alpha[p, :a], a0[p, :a]):
            fails.append(f"{fam}: alpha before a = {a} changed")
        if P.returns_early(n, idx):
            if not (same_bits(L[p, :m, :m], low0[:m, :m]) and same_bits(alpha[p, :m], a0[p, :m])):
                fails.append(f"{fam}: whole trailing tile rows went, but L' or alpha' differ from the inputs")
            if not ((part[p] == P.SENTINEL).all() and (winv[p] == P.SENTINEL).all()):
                fails.append(f"{fam}: whole trailing tile rows went, but a partial or an inverse block was written")
        else:
            J0 = a // P.NB
            if not ((part[p, :J0] == P.SENTINEL).all() and (winv[p, :J0] == P.SENTINEL).all()):
                fails.append(f"{fam}: a partial or an inverse block of a tile column before {J0} was written")
            if (part[p, J0:] == P.SENTINEL).any() or (winv[p, J0:] == P.SENTINEL).any():
                fails.append(f"{fam}: a partial or an inverse block of a tile column from {J0} on still holds the sentinel")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n, name", P.CASES)
def test_shape_of_the_slot(engine, n, name):
    _, _, (L, alpha, _, _, info) = run(engine, n, name)
    m = n - len(P.PATTERNS[n][name])
    npad = P.NB * -(-m // P.NB)
    assert L.shape == (len(P.FAMILIES), npad, npad) and alpha.shape == (len(P.FAMILIES), npad)
    assert (info == 0).all(), info
    fails = []
    eye = np.eye(npad)
    for p, fam in enumerate(P.FAMILIES):
        if not np.array_equal(L[p], np.tril(L[p])):
            fails.append(f"{fam}: not exactly lower triangular")
        if not (np.array_equal(L[p, m:, :], eye[m:, :]) and np.array_equal(L[p, :, m:], eye[:, m:])):
            fails.append(f"{fam}: rows or columns from n' = {m} on are not exactly the identity")
        if not (alpha[p, m:] == 0).all():
            fails.append(f"{fam}: alpha is not zero from n' = {m} on")
        if not (np.diag(L[p]) > 0).all() or not np.isfinite(L[p]).all() or not np.isfinite(alpha[p]).all():
            fails.append(f"{fam}: a diagonal entry is not positive, or an entry is not finite")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n, name", P.CASES)
def test_partials_match_the_factor_they_came_from(engine, n, name):
    _, _, (L, alpha, part, _, _) = run(engine, n, name)
    idx = P.PATTERNS[n][name]
    if P.returns_early(n, idx):
        assert (part == P.SENTINEL).all()
        return
    fails, worst = [], [0.0, 0.0]
    for p, fam in enumerate(P.FAMILIES):
        for J in range(idx[0] // P.NB, part.shape[1]):
            sl = slice(J * P.NB, (J + 1) * P.NB)
            lg = 2 * np.log(np.diag(L[p])[sl].astype(F.LD))
            sq = alpha[p, sl].astype(F.LD) ** 2
            d_ld, b_ld = abs(F.LD(part[p, J, 0]) - lg.sum()), 16 * U * np.abs(lg).sum()
            d_ss, b_ss = abs(F.LD(part[p, J, 1]) - sq.sum()), 16 * U * sq.sum()
            worst[0] = max(worst[0], float(d_ld / b_ld) if b_ld > 0 else 0.0)
            worst[1] = max(worst[1], float(d_ss / b_ss) if b_ss > 0 else 0.0)
            if not d_ld <= b_ld:
                fails.append(f"{fam} tile column {J}: log-det partial {part[p, J, 0]!r} vs {float(lg.sum())!r} (bound {float(b_ld):.3g})")
            if not d_ss <= b_ss:
                fails.append(f"{fam} tile column {J}: quadratic-form partial {part[p, J, 1]!r} vs {float(sq.sum())!r} (bound {float(b_ss):.3g})")
    print(f"[remove-probe] n {n} {name}: partials, worst distance / (16 u sum|.|): log-det {worst[0]:.4f}, quadratic form {worst[1]:.4f}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n, name", P.CASES)
def test_inverse_blocks_invert_their_pivot_blocks(engine, n, name):
    _, _, (L, _, _, winv, _) = run(engine, n, name)
    idx = P.PATTERNS[n][name]
    if P.returns_early(n, idx):
        assert (winv == P.SENTINEL).all()
        return
    m = n - len(idx)
    g16 = F.gamma(16)
    fails, worst = [], 0.0
    for p, fam in enumerate(P.FAMILIES):
        for J in range(idx[0] // P.NB, winv.shape[1]):
            for b in range(8):
                b0 = J * P.NB + 16 * b
                X = winv[p, J, b]
                T = L[p, b0:b0 + 16, b0:b0 + 16]
                if not np.array_equal(X, np.tril(X)):
                    fails.append(f"{fam} block ({J}, {b}): the inverse is not lower triangular")
                if b0 >= m and not np.array_equal(X, np.eye(16)):
                    fails.append(f"{fam} block ({J}, {b}): the inverse of a padding block is not the identity")
                Tl, Xl = T.astype(F.LD), X.astype(F.LD)
                w = F._ratio_max(np.abs(Tl @ Xl - np.eye(16)), np.abs(Tl) @ np.abs(Xl))
                worst = max(worst, w / g16)
                if not w <= g16:
                    fails.append(f"{fam} block ({J}, {b}): |L_bb X - I| = {w / g16:.4g} gamma_16 |L_bb| |X|")
    print(f"[remove-probe] n {n} {name}: inverse blocks, worst residual {worst:.4f} gamma_16")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n, name", [(17, "scattered"), (129, "first"), (300, "r40"), (300, "three_runs"), (384, "tile_row")])
def test_isolation_and_repeatability(engine, n, name):
    L0, a0, out = run(engine, n, name)
    idx = P.PATTERNS[n][name]
    names = ("L", "alpha", "partial", "winv", "info")
    again = engine.debug_remove_factor(L0, a0, idx)
    rev = engine.debug_remove_factor(L0[::-1], a0[::-1], idx)
    for x, y, z, what in zip(out, again, rev, names):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: two identical calls differ"
        assert np.array_equal(x.view(np.uint8), np.ascontiguousarray(z[::-1]).view(np.uint8)), f"{what}: the batch in reverse order differs"
    for p, fam in enumerate(P.FAMILIES):
        one = engine.debug_remove_factor(L0[p:p + 1], a0[p:p + 1], idx)
        for x, y, what in zip(out, one, names):
            assert np.array_equal(np.ascontiguousarray(x[p:p + 1]).view(np.uint8), y.view(np.uint8)), f"{what} of {fam}: the batch of six and the factor alone differ"


def test_no_forward_solve_vector_means_zeros(engine):
    L0, a0, out = run(engine, 300, "front9")
    got = engine.debug_remove_factor(L0, None, P.PATTERNS[300]["front9"])
    assert same_bits(got[0], out[0]) and same_bits(got[3], out[3]) and np.array_equal(got[4], out[4])
    assert (got[1] == 0).all() and same_bits(got[2][:, :, 0], out[2][:, :, 0]) and (got[2][:, :, 1] == 0).all()


@pytest.mark.parametrize("n, name", [(300, "r40"), (300, "three_runs"), (257, "first")])
def test_poison_mode_gives_the_same_bits(pkg, engine, monkeypatch, n, name):
    """every buffer NaN-poisoned before use (AGP_POISON=1): the update reads nothing it or the packer has not written"""
    L0, a0, out = run(engine, n, name)
    monkeypatch.setenv("AGP_POISON", "1")
    e = pkg.GPEngine(0)
    try:
        got = e.debug_remove_factor(L0, a0, P.PATTERNS[n][name])
    finally:
        e.close()
    for x, y, what in zip(out, got, ("L", "alpha", "partial", "winv", "info")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: poison mode changes the result"


def test_a_probe_call_leaves_the_engine_as_it_was(pkg):
    """the same remove_data / logpdf_batch_extend sequences with and without probe calls between them: results and counters equal"""
    G = pkg
    ts, xs = G.prior.synthetic_series(300, seed=5)
    nodes = [G.SquaredExponential(0.47, 0.13), G.Periodic(0.96, 0.21, 1.1), G.Linear(0.1, 1.3, 0.7) + G.SquaredExponential(0.2, 0.5)]
    noises = np.array([0.05, 0.1, 0.2])
    L0, a0 = P.batch_inputs(300, "r40")
    res = []
    for probe in (False, True):
        e = G.GPEngine(0)
        try:
            e.set_remove_update(2)
            e.set_data(ts, xs)
            seq = [e.logpdf_batch_extend(nodes, noises, check=False)]
            if probe:
                e.debug_remove_factor(L0, a0, P.PATTERNS[300]["r40"])
            e.remove_data([0, 130, 131])
            if probe:
                e.debug_remove_factor(L0[:2], None, [128])
            seq.append(e.logpdf_batch_extend(nodes, noises, check=False))
            e.remove_data(list(range(10, 50)))
            seq.append(e.logpdf_batch_extend(nodes, noises, check=False))
            res.append((seq, e.remove_stats(), e.extend_stats()))
        finally:
            e.close()
    (s0, r0, x0), (s1, r1, x1) = res
    assert r0 == r1 and x0 == x1 and r0["updated"] == 2 * len(nodes)
    for (lp0, i0), (lp1, i1) in zip(s0, s1):
        assert same_bits(lp0, lp1) and np.array_equal(i0, i1) and (i0 == 0).all()


def test_argument_errors(engine):
    lib, ctx = engine._lib, engine._ctx
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    n, P_ = 17, 2
    L0 = np.ascontiguousarray(np.stack([P.factor(f, n)[0] for f in ("wishart", "spec")]))
    a0 = np.ascontiguousarray(np.stack([P.factor(f, n)[1] for f in ("wishart", "spec")]))
    big = 128 * 128
    oL, oa, op, ow, oi = np.zeros(P_ * big), np.zeros(P_ * 128), np.zeros(P_ * 2), np.zeros(P_ * 2048), np.zeros(P_, dtype=np.int32)

    def call(n=n, P=P_, idx=(2, 9, 15), k=None, L0=L0, oL=oL, oa=oa, op=op, oi=oi, idx_null=False):
        v = np.asarray(idx, dtype=np.int64)
        arg = lambda x, t: None if x is None else x.ctypes.data_as(t)      # noqa: E731
        return lib.agp_debug_remove_factor(ctx, arg(L0, dp), arg(a0, dp), n, P, None if idx_null else v.ctypes.data_as(lp),
                                           len(v) if k is None else k, arg(oL, dp), arg(oa, dp), arg(op, dp), arg(ow, dp), arg(oi, ip))

    def valid_call_passes():
        L, alpha, _, _, info = engine.debug_remove_factor(L0, a0, [2, 9, 15])
        assert (info == 0).all()
        fails = backward_errors(17, "scattered", L, alpha, members=(P.FAMILIES.index("wishart"), P.FAMILIES.index("spec")))
        assert not fails, "\n".join(fails)

    assert P.PATTERNS[17]["scattered"] == [2, 9, 15]
    bad = [dict(n=1, idx=(0,)), dict(n=1025), dict(k=0), dict(idx=tuple(range(17))), dict(idx=tuple(range(16)) + (16, 17), k=18), dict(P=0), dict(P=-1),
           dict(n=1024, P=17),                                        # P n^2 > 2^24
           dict(idx=(9, 2, 15)), dict(idx=(2, 2, 15)), dict(idx=(-1, 2)), dict(idx=(2, 17)),
           dict(L0=None), dict(oL=None), dict(oa=None), dict(op=None), dict(oi=None), dict(idx_null=True)]
    for kw in bad:
        assert call(**kw) == -1, kw                                   # AGP_ERR_ARG
        valid_call_passes()
    assert call() == 0
