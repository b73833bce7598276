"""Single kernel values of every fp64 product entry point against the np.longdouble closed form (tests/kernel_value_cases.py has the point
sets, the derivation of the per-element tolerance and the case table).  Values are read out with unit vectors: every other term of the
fixed-order sums is kappa * 0, so the entry returns one product.  Outputs are pre-filled with NaN, every element is compared, a second
extraction must be bitwise equal, and each configuration shows from cglb_get_stat that it ran the instance its row names.
K_ff products: test_matvec_values, test_matmat_values.  Cross products: test_cross_values (every padded width up to 32),
test_cross_matvec_values_wide (rectangular Gram tiles).  Input-gradient products, value and gradient [n_new, N, D] of every pair:
test_cross_grad_values, test_cross_grad_values_mid_width, test_cross_grad_weighted_values(_inducing).  K_ff gradient passes by probe pairs:
test_grad_kff_multi_values, test_grad_kff_multi_values_mid_width (which kernel runs for which S: its docstring).  Not covered: the feature
products' cos_turns / sincos_turns, the gradient pass through the Gram tiles, fp32."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_value_cases as kv

pytestmark = pytest.mark.gpu

VAR, NOISE = 1.7, 0.3
CASES = kv.case_table()


def _cases(names):
    return [c for c in CASES if c.name in names]


def _ids(cases):
    return [kv.case_id(c) for c in cases]


DEFAULTS = {"kff_variant": 2, "kff_rows": 4, "precision": 1, "sym_order": 1, "wide_reg": 1}   # cglb_internal.h


def _configure(ctx, case, options):
    """the options of one configuration (every other one at its default), then the hyper-parameters; returns the regime it ran in"""
    X, ls = kv.build_set(case)
    for k, v in {**DEFAULTS, **options}.items():
        ctx.set_option(k, v)
    ctx.set_hypers(ls, VAR, NOISE, 0.0, X[:1], 1e-6)
    clamp, bias = kv.regime(case.kind, X, ls)
    assert int(ctx.get_stat("exp_clamp")) == clamp == case.clamp          # the instance the row names
    assert ctx.get_stat("m32_bias") == pytest.approx(bias, rel=1e-12, abs=0.0)
    return clamp, bias


def _context(case, options):
    from cglb_amd.hip_context import HipContext
    X, ls = kv.build_set(case)
    ctx = HipContext(X, np.zeros(X.shape[0]), 1, case.kind)
    clamp, bias = _configure(ctx, case, options)
    return ctx, clamp, bias


def _check(lib, ctx, rc):
    from cglb_amd import _lib
    _lib.check(rc, ctx._ctx)


def _matvec_matrix(ctx):
    """K + noise I by N mat-vecs with unit vectors; row j of the buffer is column j of the matrix"""
    from cglb_amd.hip_context import _ptr
    N = ctx.N
    eye = torch.eye(N, dtype=torch.float64, device=ctx.device)
    buf = torch.full((N, N), float("nan"), dtype=torch.float64, device=ctx.device)
    for j in range(N):
        _check(ctx.lib, ctx, ctx.lib.cglb_matvec(ctx._ctx, _ptr(eye[j]), _ptr(buf[j])))
    return buf.t().cpu().numpy()


def _matmat_matrix(ctx):
    from cglb_amd.hip_context import _ptr
    N = ctx.N
    eye = torch.eye(N, dtype=torch.float64, device=ctx.device)
    buf = torch.full((N, N), float("nan"), dtype=torch.float64, device=ctx.device)
    for j0 in range(0, N, 8):
        s = min(8, N - j0)   # the last group is short: 276 = 34 * 8 + 4
        _check(ctx.lib, ctx, ctx.lib.cglb_matmat(ctx._ctx, _ptr(eye[j0:j0 + s]), s, _ptr(buf[j0:j0 + s])))
    return buf.t().cpu().numpy()


def _compare(case, tag, dev, g, bound, diag):
    ref = kv.LD(VAR) * g.kap
    extra = None
    if diag:
        n = dev.shape[0]
        ref = ref + kv.LD(NOISE) * np.eye(n, dtype=kv.LD)   # the noise joins the REFERENCE in extended precision
        extra = np.eye(n) * (kv.U * (VAR + NOISE))            # the rounding of fma(noise, 1, var * sum) on the diagonal
    r = kv.ratios(dev, ref, bound, scale=VAR, extra=extra)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # (a reference below the smallest double: masked by `floored`)
        rel = np.where(bound.floored | (ref == 0), 0.0, np.abs((dev - ref) / ref).astype(np.float64))
    w = np.unravel_index(int(np.argmax(rel)), rel.shape)
    print(f"{kv.case_id(case)} {tag}: {kv.locate(case, g, r, bound.floored)}; largest relative error {rel[w]:.2e} at E = {float(g.E[w]) / 256:.1f} octaves")
    return r


MATVEC_CONFIGS = [("sym", {"kff_variant": 2, "precision": 0}), ("sym", {"kff_variant": 2, "precision": 1}),
                  ("sym", {"kff_variant": 2, "precision": 2}), ("plain", {"kff_variant": 0, "kff_rows": 1, "precision": 1}),
                  ("plain", {"kff_variant": 0, "kff_rows": 4, "precision": 1})]


WIDE_CONFIGS = [("mid", {"wide_reg": 1, "precision": 0}), ("mid", {"wide_reg": 1, "precision": 1}), ("mid", {"wide_reg": 1, "precision": 2}),
                ("tiles", {"wide_reg": 0, "precision": 1})]


def _path(family, case, prec, clamp):
    entry = "tiles" if family == "tiles" else {"sym": "matvec_sym", "plain": "matvec_plain", "mid": "matvec_mid"}[family]
    return kv.path_for(entry, case.kind, prec, clamp)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_matvec_values(case):
    configs = list(MATVEC_CONFIGS)
    if case.D > 96:       # Gram tiles whatever the options
        configs = [("tiles", {"precision": 1})]
    elif case.D > 32:     # mid width: register-resident symmetric stream (wide_reg 1) or the tiles (wide_reg 0)
        configs = list(WIDE_CONFIGS)
    if case.name.startswith("C'"):   # both sides of the integer bound run the clamped instances of row C: the default level of either kernel
        configs = [MATVEC_CONFIGS[1], MATVEC_CONFIGS[4]]
    if case.name == "B":
        configs += [("sym", {"kff_variant": 2, "precision": 1, "sym_order": 0}), ("sym", {"kff_variant": 2, "precision": 1, "sym_order": 1})]
    g = kv.set_geometry(case)
    worst = 0.0
    ctx, _, _ = _context(case, {})   # one context per set; every configuration sets its options and the hyper-parameters again
    for family, opts in configs:
        clamp, bias = _configure(ctx, case, opts)
        K = _matvec_matrix(ctx)
        again = _matvec_matrix(ctx)
        assert np.array_equal(K, again, equal_nan=True)
        p = _path(family, case, opts["precision"], clamp)
        r = _compare(case, f"matvec {opts}", K, g, kv.tolerance(case.kind, g, p, bias), diag=True)
        worst = max(worst, r.max())
    ctx.close()
    assert worst <= 1.0


MATMAT_CASES = _cases(("A", "B", "E8", "E32", "F40", "F77"))


def _levels(cases, all_levels_on):
    """every case at the default level, the cases named `all_levels_on` at the other two as well"""
    return [pytest.param(c, prec, id=f"{kv.case_id(c)}-{prec}") for c in cases for prec in ((0, 1, 2) if c.name == all_levels_on else (1,))]


@pytest.mark.parametrize("case,prec", _levels(MATMAT_CASES, "E8"))
def test_matmat_values(case, prec):
    g = kv.set_geometry(case)
    ctx, clamp, bias = _context(case, {"kff_variant": 2, "precision": prec})
    # the shared-kernel instance runs: narrow rows are unclamped, the mid-width instance takes both ranges
    assert int(ctx.get_stat("matmat_native")) == 1 and (case.D > 32 or clamp == 0)
    K = _matmat_matrix(ctx)
    again = _matmat_matrix(ctx)
    ctx.close()
    assert np.array_equal(K, again, equal_nan=True)
    p = kv.path_for("matmat" if case.D <= 32 else "matmat_mid", case.kind, prec, clamp)
    r = _compare(case, f"matmat precision {prec}", K, g, kv.tolerance(case.kind, g, p, bias), diag=True)
    assert r.max() <= 1.0


CROSS_CASES = _cases(("A", "D", "E8", "E12", "E32"))


@pytest.mark.parametrize("case,prec", _levels(CROSS_CASES, "A"))
def test_cross_values(case, prec):
    """cglb_cross_matvec (one unit vector per call) and cglb_cross_matmat (V = identity: the whole cross matrix in one call; the cross_multi_kernel
    instance of every padded width up to 32)"""
    from cglb_amd.hip_context import _ptr
    g = kv.set_geometry(case, cross=True)
    xnew = kv.new_points(case)
    ctx, clamp, bias = _context(case, {"precision": prec})
    N, n_new = ctx.N, xnew.shape[0]
    eye = torch.eye(N, dtype=torch.float64, device=ctx.device)
    xn = ctx._xnew(xnew)

    def by_matvec():
        buf = torch.full((N, n_new), float("nan"), dtype=torch.float64, device=ctx.device)
        for j in range(N):
            _check(ctx.lib, ctx, ctx.lib.cglb_cross_matvec(ctx._ctx, _ptr(xn), n_new, _ptr(eye[j]), _ptr(buf[j])))
        return buf.t().cpu().numpy()

    def by_matmat():
        out = torch.full((n_new, N), float("nan"), dtype=torch.float64, device=ctx.device)
        return ctx.cross_matmat(xnew, eye, out=out).cpu().numpy()

    worst = 0.0
    for entry, fn in (("cross_matvec", by_matvec), ("cross_matmat", by_matmat)):
        K = fn()
        assert np.array_equal(K, fn(), equal_nan=True)
        p = kv.path_for(entry, case.kind, prec, clamp)
        r = _compare(case, f"{entry} precision {prec}", K, g, kv.tolerance(case.kind, g, p, 0.0), diag=False)
        worst = max(worst, r.max())
    ctx.close()
    assert worst <= 1.0


WIDE_CROSS_CASES = _cases(("F40", "F77", "G100"))
TINY = 2.0 ** -1022


@pytest.mark.parametrize("case", WIDE_CROSS_CASES, ids=_ids(WIDE_CROSS_CASES))
def test_cross_matvec_values_wide(case):
    """cglb_cross_matvec on inputs wider than 32 dimensions: rectangular Gram tiles whatever wide_reg says (path `tiles`: exp2_neg, no table, no level and
    NO clamp).  The relative check therefore reaches down to the smallest normal number; where f kappa of the longdouble reference is below 2^-1022 the
    device value must lie in [0, 2^-1022].  Such elements are counted and capped: the row at 1e3, and on rbf-F77 (oct 1200 by design) the corner pairs
    and the off-set rows (`floored_cap`)."""
    from cglb_amd.hip_context import _ptr
    g = kv.set_geometry(case, cross=True)
    xnew = kv.new_points(case)
    ctx, clamp, bias = _context(case, {"precision": 1})
    N, n_new = ctx.N, xnew.shape[0]
    eye = torch.eye(N, dtype=torch.float64, device=ctx.device)
    xn = ctx._xnew(xnew)

    def by_matvec():
        buf = torch.full((N, n_new), float("nan"), dtype=torch.float64, device=ctx.device)
        for j in range(N):
            _check(ctx.lib, ctx, ctx.lib.cglb_cross_matvec(ctx._ctx, _ptr(xn), n_new, _ptr(eye[j]), _ptr(buf[j])))
        return buf.t().cpu().numpy()

    K = by_matvec()
    again = by_matvec()
    ctx.close()
    assert np.array_equal(K, again, equal_nan=True)
    b = kv.tolerance(case.kind, g, kv.path_for("tiles", case.kind, 1, 0), 0.0)
    assert not b.floored.any()
    b.floored = np.asarray(kv.LD(VAR) * g.kap < kv.LD(TINY))
    b.floor = np.full(g.kap.shape, kv.LD(TINY) / kv.LD(VAR))
    assert b.floored[-1].all() and int(b.floored[:-1].sum()) <= kv.floored_cap(case, N)
    r = _compare(case, "cross_matvec (tiles)", K, g, b, diag=False)
    assert r.max() <= 1.0


# ---- input-gradient products: value and gradient of every pair by unit vectors ---------------------------------------------------------------
def _nan(ctx, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=ctx.device)


def _assert_floored_cap(case, floored):
    """only the row at 1e3 is under the floor by design; what else is, is capped by the case table's own range figures"""
    assert floored[-1].all()
    assert int(floored[:-1].sum()) <= kv.floored_cap(case, floored.shape[1])


def _compare_grad(case, tag, entry, prec, K, G, xnew):
    """value [n_new, N] and gradient [n_new, N, D] of a unit-vector read-out against the bounds of the path; the reference of the gradient per
    coordinate.  Returns the worst error / tolerance."""
    X, ls = kv.build_set(case)
    g = kv.set_geometry(case, cross=True)
    p = kv.path_for(entry, case.kind, prec, 1)
    bk, bh = kv.tolerance(case.kind, g, p), kv.tolerance(case.kind, g, p, which="h")
    _assert_floored_cap(case, bk.floored)
    rk = _compare(case, f"{tag} value", K, g, bk, diag=False)
    rg, zeros = np.zeros(rk.shape), 0
    kworst, live = 0, ~bk.floored
    for k in range(case.D):
        r, same = kv.input_grad_ratios(case.kind, g, p, xnew, X, ls, k, bh, G[:, :, k], scale=VAR)
        zeros += same
        if r[live].max() > rg[live].max():
            kworst = k
        rg = np.maximum(rg, r)
    print(f"{kv.case_id(case)} {tag} gradient: {kv.locate(case, g, rg, bk.floored)}, coordinate {kworst} of {case.D}; {zeros} entries of equal coordinates exactly zero")
    return max(rk.max(), rg.max())


def _cross_grad_readout(case, prec, entry, options):
    """ctx.cross_grad_matmat with V the N x N identity: one call returns the whole 282 x 276 cross matrix and its gradient [282, 276, D]; every column
    lands in a position of its group of 8 / 4 / 2.  A second read-out with V = the identity without its first column (S = 275) moves every column to
    another position and leaves the last group short at every width: the same per-element arithmetic, so bitwise the same numbers."""
    xnew = kv.new_points(case)
    ctx, clamp, bias = _context(case, {"precision": prec, **options})
    assert int(ctx.get_stat("input_grad_native")) == 1
    N, n, D = ctx.N, xnew.shape[0], ctx.D
    eye = torch.eye(N, dtype=torch.float64, device=ctx.device)

    def run(V, with_value=True):
        S = V.shape[1]
        out, gout = ctx.cross_grad_matmat(xnew, V, out=_nan(ctx, n, S) if with_value else None, gout=_nan(ctx, n, S, D), with_value=with_value)
        return (out.cpu().numpy() if with_value else None), gout.cpu().numpy()

    K, G = run(eye)
    K2, G2 = run(eye)
    assert np.array_equal(K, K2, equal_nan=True) and np.array_equal(G, G2, equal_nan=True)
    del K2, G2
    _, G3 = run(eye, with_value=False)
    assert np.array_equal(G, G3, equal_nan=True)           # the gradient alone requested: bitwise the same
    del G3
    Ks, Gs = run(eye[:, 1:].contiguous())
    ctx.close()
    assert np.array_equal(Ks, K[:, 1:], equal_nan=True) and np.array_equal(Gs, G[:, 1:], equal_nan=True)
    del Ks, Gs
    worst = _compare_grad(case, f"{entry} precision {prec}", entry, prec, K, G, xnew)
    assert worst <= 1.0


CROSS_GRAD_CASES = _cases(("A", "B", "C", "D", "E8", "E12", "E32"))


@pytest.mark.parametrize("case,prec", _levels(CROSS_GRAD_CASES, "E8"))
def test_cross_grad_values(case, prec):
    """cross_grad_kernel (kernels_input_grad.hip; kappa_hfac_hot_from_d2): out[i, j] = f kappa_ij under the kappa bound of the path, gout[i, j, k] =
    -f h_ij delta_k / l_k under `input_grad_tolerance`; exactly zero where x*_ik == x_jk as doubles (the duplicate row, the coincident new points, every
    off-axis coordinate of the sweep pairs); under the clamp floor the right sign and at most floor_h |delta_k| / l_k.  The row at 1e3 is under the floor;
    on every row but rbf-D and the two Matern D rows (oct 2400 by design) no other pair may be."""
    _cross_grad_readout(case, prec, "cross_grad", {})


MID_ROWS = _cases(("F40", "F64", "F77", "F90"))
MID_CASES = [v for c in MID_ROWS for v in [c] + kv.axis_variants(c)]


def _mid_levels(all_levels_on):
    return [pytest.param(c, prec, id=f"{kv.case_id(c)}-{prec}") for c in MID_CASES for prec in ((0, 1, 2) if c.name == all_levels_on else (1,))]


@pytest.mark.parametrize("case,prec", _mid_levels("F40"))
def test_cross_grad_values_mid_width(case, prec):
    """cross_grad_mid_kernel (kernels_input_grad_mid.hip; options input_grad_mid 1, wide_reg 1): the read-out and the assertions of
    test_cross_grad_values at the four hot widths 48, 64, 80, 96, on the rows and on their axis variants - the sweep, and with it every designed
    exponent, in lane part 0, 2 and 3 of the four a new point is shared by (at D = 40 and 77 the last part is partly zero padding; the form of the
    reference is the same there).  rbf-F77 (oct 1200 by design) is the one row with pairs of the set under the floor."""
    _cross_grad_readout(case, prec, "cross_grad_mid", {"input_grad_mid": 1, "wide_reg": 1})


WEIGHTED_CASES = _cases(("A", "E8", "E32"))


def _weighted_readout(ctx, case, prec, point_set):
    xnew = kv.new_points(case)
    N, n, D = ctx.N, xnew.shape[0], ctx.D
    ldw = n + 3
    dev = ctx.device
    u = torch.zeros(N, dtype=torch.float64, device=dev)
    Wt = _nan(ctx, N, ldw)                   # the spare columns hold NaN: never read
    cols = torch.arange(n, device=dev)

    def run(which):
        """(value, gradient) by u = e_m and by Wt[m, i] = [m == (i + shift) % N], m = shift = 0 .. N - 1; which: 'both' | 'u' | 'w'"""
        Ku, Gu, Kw, Gw = np.full((n, N), np.nan), np.full((n, N, D), np.nan), np.full((n, N), np.nan), np.full((n, N, D), np.nan)
        for m in range(N):
            u[m] = 1.0
            Wt[:, :n] = 0.0
            tgt = (cols + m) % N
            Wt[tgt, cols] = 1.0
            kw = {}
            if which != "w":
                kw.update(u=u, out_u=_nan(ctx, n), gout_u=_nan(ctx, n, D))
            if which != "u":
                kw.update(Wt=Wt, out_w=_nan(ctx, n), gout_w=_nan(ctx, n, D))
            ou, gu, ow, gw = ctx.cross_grad_weighted(xnew, point_set=point_set, **kw)
            u[m] = 0.0
            if which != "w":
                Ku[:, m], Gu[:, m] = ou.cpu().numpy(), gu.cpu().numpy()
            if which != "u":
                t = tgt.cpu().numpy()
                Kw[np.arange(n), t], Gw[np.arange(n), t] = ow.cpu().numpy(), gw.cpu().numpy()
        return Ku, Gu, Kw, Gw

    both = run("both")
    again = run("both")
    for a, b in zip(both, again):
        assert np.array_equal(a, b, equal_nan=True)
    del again
    ua = run("u")
    assert np.array_equal(both[0], ua[0], equal_nan=True) and np.array_equal(both[1], ua[1], equal_nan=True)   # both weights in one call: each as alone
    del ua
    wa = run("w")
    assert np.array_equal(both[2], wa[2], equal_nan=True) and np.array_equal(both[3], wa[3], equal_nan=True)
    del wa
    worst = _compare_grad(case, f"cross_grad_weighted {point_set} u precision {prec}", "cross_grad_weighted", prec, both[0], both[1], xnew)
    return max(worst, _compare_grad(case, f"cross_grad_weighted {point_set} Wt precision {prec}", "cross_grad_weighted", prec, both[2], both[3], xnew))


@pytest.mark.parametrize("case,prec", _levels(WEIGHTED_CASES, "A"))
def test_cross_grad_weighted_values(case, prec):
    """weighted_grad_kernel (kernels_predict_grad.hip; the evaluator of cross_grad_kernel, row-weighted), point set "train": u = e_m for every m (N calls:
    out_u / gout_u are column m) and Wt[m, i] = 1 where m == (i + shift) % N, shift = 0 .. N - 1, with ldw = n_new + 3 and NaN in the spare columns.
    Both weights in one call are bitwise what each gives alone; value and gradient under the bounds of test_cross_grad_values."""
    ctx, clamp, bias = _context(case, {"precision": prec})
    worst = _weighted_readout(ctx, case, prec, "train")
    ctx.close()
    assert worst <= 1.0


@pytest.mark.parametrize("kind", kv.KINDS)
def test_cross_grad_weighted_values_inducing(kind):
    """The same read-out against the inducing points on row A: cglb_set_hypers stages Z in hot units (Zh) on a narrow context at once, without
    cglb_setup, so a context created with num_inducing = N and Z = X has the set itself as its inducing points."""
    from cglb_amd.hip_context import HipContext
    case = kv.find_case(kind, "A")
    X, ls = kv.build_set(case)
    ctx = HipContext(X, np.zeros(X.shape[0]), X.shape[0], kind)
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.set_hypers(ls, VAR, NOISE, 0.0, X, 1e-6)
    assert int(ctx.get_stat("exp_clamp")) == case.clamp
    worst = _weighted_readout(ctx, case, 1, "inducing")
    ctx.close()
    assert worst <= 1.0


GRAD_CASES = _cases(("A", "B", "E8", "E32"))


@pytest.mark.parametrize("case,prec", _levels(GRAD_CASES, "A"))
def test_grad_kff_multi_values(case, prec):
    """U = e_i, V = e_j: out[D] = kappa_ij, out[k] = dK_ij / dl_k.  S = 1 and S = 2 (a zero second pair) are two instances of the multi-pair
    kernel (direct differences, range-clamped 2^x; grad_gram does not reach it on inputs of up to 32 dimensions)."""
    from cglb_amd.hip_context import _ptr
    X, ls = kv.build_set(case)
    g = kv.set_geometry(case)
    pairs = kv.probe_pairs(case)
    ctx, clamp, bias = _context(case, {"precision": prec})
    p = kv.path_for("grad", case.kind, prec, clamp)
    ref, bound = kv.grad_tolerance(case.kind, g, p, X, ls, pairs, VAR)
    N, D = ctx.N, ctx.D
    worst = 0.0
    for S in (1, 2):
        U = torch.zeros((S, N), dtype=torch.float64, device=ctx.device)
        V = torch.zeros((S, N), dtype=torch.float64, device=ctx.device)
        got = np.full((2, len(pairs), D + 1), np.nan)
        for rep in range(2):
            for q, (i, j) in enumerate(pairs):
                U[0, i] = 1.0
                V[0, j] = 1.0
                out = np.full(D + 1, np.nan)
                _check(ctx.lib, ctx, ctx.lib.cglb_grad_kff_multi(ctx._ctx, _ptr(U), _ptr(V), S, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
                got[rep, q] = out
                U[0, i] = 0.0
                V[0, j] = 0.0
        assert np.array_equal(got[0], got[1], equal_nan=True)
        r = kv.ratios(got[0], ref, bound)
        w = np.unravel_index(int(np.argmax(r)), r.shape)
        i, j = pairs[w[0]]
        E = g.E[i, j]
        n = np.floor(-E)
        print(f"{kv.case_id(case)} grad_kff_multi S {S} precision {prec}: worst error / tolerance {r.max():.3f} at pair ({i}, {j}) entry {w[1]} of {D + 1}, "
              f"E = {float(E):.9f} hot units, table index {int(n) & 255}, fraction {float(-E - n):.3e}")
        worst = max(worst, r.max())
    ctx.close()
    assert worst <= 1.0


def _mid_grad_params():
    """rows and axis variants at the default level, F40 at the three; the multi-pair instance switched off (grad_multi_mid 0: S single passes and one
    product, the bound the file held the mid widths to before the multi-pair kernel) on F40 at the default level"""
    out = [pytest.param(c, prec, 1, id=f"{kv.case_id(c)}-{prec}") for c in MID_CASES for prec in ((0, 1, 2) if c.name == "F40" else (1,))]
    return out + [pytest.param(c, 1, 0, id=f"{kv.case_id(c)}-1-single") for c in MID_CASES if c.name == "F40"]


@pytest.mark.parametrize("case,prec,native", _mid_grad_params())
def test_grad_kff_multi_values_mid_width(case, prec, native):
    """Inputs of 33 .. 96 dimensions (wide_reg 1).  cglb_grad_kff_multi cuts S pairs into groups of 8 in order: a group of two or more runs
    grad_kff_multi_mid_kernel (kernels_grad_multi_mid.hip, padded to 4 or 8 pairs: Gram form, both orientations on the two wave halves, out[D] = the
    kappa sum the kernel forms itself from P(r) at the exponent's root), a single pair - S = 1, or the one left over after a group of 8 - the single
    Gram-form pass of kernels_grad_mid.hip with out[D] from one product, u^T ((K_ff + noise I) v - noise v) / variance.  With grad_multi_mid 0 every
    pair takes the single pass.  Both form delta_k^2 from moments (the absolute term of `grad_tolerance(moments=True)`).
    S in (1, 2, 4, 5, 8, 9, 10): the single pass, padded groups of 4 and 8, 8 plus a left-over single pass, 8 plus a group of 2.  The probed pair sits in
    slot q % S, rotating with the pair index, in both orientations (U = e_i, V = e_j and U = e_j, V = e_i); the probe pairs include pairs inside one
    row block and across two (the weight differs between the diagonal block and the blocks to its right); every other slot carries a non-zero U with
    V = 0, or the reverse, alternating, so that all their true terms are exact zeros and cross-talk is not."""
    from cglb_amd.hip_context import _ptr
    X, ls = kv.build_set(case)
    g = kv.set_geometry(case)
    pairs = kv.probe_pairs_blocks(case)
    ctx, clamp, bias = _context(case, {"precision": prec, "wide_reg": 1, "grad_multi_mid": native})
    assert int(ctx.get_stat("grad_multi_native")) == native
    N, D = ctx.N, ctx.D
    # single pass: out[D] from the mid-width product - its own rounding of var * sum (in its path), the subtraction of noise v and the division; on the
    # diagonal fma(noise, 1, var kappa)
    kb = kv.tolerance(case.kind, g, kv.path_for("matvec_mid", case.kind, prec, clamp), bias)
    kb.tol = kb.tol + 2 * kv.U * g.kap + np.eye(N) * (3 * kv.U * (1.0 + NOISE / VAR))
    ref, b_single = kv.grad_tolerance(case.kind, g, kv.path_for("grad_mid", case.kind, prec, clamp), X, ls, pairs, VAR, bias=bias, kappa_bound=kb, moments=True)
    ref_m, b_multi = kv.grad_tolerance(case.kind, g, kv.path_for("grad_multi_mid", case.kind, prec, clamp), X, ls, pairs, VAR, bias=bias, moments=True)
    assert np.array_equal(ref, ref_m)
    worst = 0.0
    for S in kv.MULTI_S:
        got = np.full((2, 2, len(pairs), D + 1), np.nan)
        single = np.zeros(len(pairs), dtype=bool)
        for rep in range(2):
            for q, (i, j) in enumerate(pairs):
                for swap in (0, 1):
                    Um, Vm, slot = kv.multi_probe(N, S, q, i, j, bool(swap))
                    single[q] = kv.multi_single_slot(S, slot, bool(native))
                    U = torch.as_tensor(Um, device=ctx.device)
                    V = torch.as_tensor(Vm, device=ctx.device)
                    out = np.full(D + 1, np.nan)
                    _check(ctx.lib, ctx, ctx.lib.cglb_grad_kff_multi(ctx._ctx, _ptr(U), _ptr(V), S, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
                    got[rep, swap, q] = out
        assert np.array_equal(got[0], got[1], equal_nan=True)
        assert single.all() == (S == 1 or not native) and (single.any() == (S in (1, 9) or not native))
        sel = single[:, None]
        bound = kv.Bound(np.where(sel, b_single.tol, b_multi.tol), np.where(sel, b_single.floored, b_multi.floored), np.where(sel, b_single.floor, b_multi.floor))
        for swap in (0, 1):
            r = kv.ratios(got[0, swap], ref, bound)
            w = np.unravel_index(int(np.argmax(r)), r.shape)
            i, j = pairs[w[0]]
            E = g.E[i, j]
            n = np.floor(-E)
            print(f"{kv.case_id(case)} grad_kff_multi (mid width{'' if native else ', single passes'}) S {S} precision {prec} "
                  f"{'U = e_j, V = e_i' if swap else 'U = e_i, V = e_j'}: worst error / tolerance {r.max():.3f} at pair ({i}, {j}) slot {w[0] % S} entry {w[1]} of "
                  f"{D + 1} ({'single pass' if single[w[0]] else 'multi-pair kernel'}), E = {float(E):.9f} hot units, table index {int(n) & 255}, "
                  f"fraction {float(-E - n):.3e}")
            worst = max(worst, r.max())
    ctx.close()
    assert worst <= 1.0
