"""Single kernel values of every fp64 product entry point against the np.longdouble closed form (tests/kernel_value_cases.py has the point
sets, the derivation of the per-element tolerance and the case table).  Values are read out with unit vectors: every other term of the
fixed-order sums is kappa * 0, so the entry returns one product.  Outputs are pre-filled with NaN, every element is compared, a second
extraction must be bitwise equal, and each configuration shows from cglb_get_stat that it ran the instance its row names."""
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
    with np.errstate(divide="ignore", invalid="ignore"):
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


CROSS_CASES = _cases(("A", "D"))


@pytest.mark.parametrize("case,prec", _levels(CROSS_CASES, "A"))
def test_cross_values(case, prec):
    """cglb_cross_matvec (one unit vector per call) and cglb_cross_matmat (V = identity: the whole cross matrix in one call)"""
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


WIDE_GRAD_CASES = _cases(("F40", "F77"))


@pytest.mark.parametrize("case,prec", _levels(WIDE_GRAD_CASES, "F40"))
def test_grad_kff_multi_values_mid_width(case, prec):
    """Inputs of 33 .. 96 dimensions: cglb_grad_kff_multi runs S single Gram-form passes of kernels_grad_mid.hip (wide_reg 1; the moment form of
    delta_k^2, which has its own absolute term) and takes out[D] from one product, u^T ((K_ff + noise I) v - noise v) / variance."""
    from cglb_amd.hip_context import _ptr
    X, ls = kv.build_set(case)
    g = kv.set_geometry(case)
    pairs = kv.probe_pairs(case)
    ctx, clamp, bias = _context(case, {"precision": prec, "wide_reg": 1})
    N, D = ctx.N, ctx.D
    kb = kv.tolerance(case.kind, g, kv.path_for("matvec_mid", case.kind, prec, clamp), bias)
    # the product's own rounding of var * sum (in its path), the subtraction of noise v and the division; on the diagonal fma(noise, 1, var kappa)
    kb.tol = kb.tol + 2 * kv.U * g.kap + np.eye(N) * (3 * kv.U * (1.0 + NOISE / VAR))
    p = kv.path_for("grad_mid", case.kind, prec, clamp)
    ref, bound = kv.grad_tolerance(case.kind, g, p, X, ls, pairs, VAR, bias=bias, kappa_bound=kb, moments=True)
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
        print(f"{kv.case_id(case)} grad_kff_multi (mid width) S {S} precision {prec}: worst error / tolerance {r.max():.3f} at pair ({i}, {j}) entry {w[1]} of "
              f"{D + 1}, E = {float(E):.9f} hot units, table index {int(n) & 255}, fraction {float(-E - n):.3e}")
        worst = max(worst, r.max())
    ctx.close()
    assert worst <= 1.0
