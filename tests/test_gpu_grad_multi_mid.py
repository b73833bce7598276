"""The multi-pair gradient pass on inputs of 33 - 96 dimensions (cglb_amd/csrc/kernels_grad_multi_mid.hip behind cglb_grad_kff_multi and
cglb_itergp_objective_and_grad): every kernel value and derivative factor once for a group of up to 8 vector pairs, on the decomposition of
the single mid-width pass.  Problems: tests/wide_cases.py, `problem(N, D, 8, seed=D)`; reference: tests/itergp_ref.py `bilinear_forms`;
vector pairs standard normal [N, S].

Tolerances: 1e-11 of the sum of the absolute values of the terms per entry, the figure tests/test_gpu_grad_multi.py holds the narrow kernel
and the fall-back to and tests/test_gpu_wide.py the wide products; twice that between two results that are each inside 1e-11 of one
reference (the sum of the single passes, the option "grad_multi_mid" 0); precision level 2 at 1e-9 as tests/test_gpu_multi_mid.py.
The references are informative on the listed shapes (median off-diagonal kernel value 0.35 - 0.53): a 1e-11 wobble of the kernel values
moves them by at most 6e-13 of that scale (1e-11 at N = 2)."""
import functools

import numpy as np
import pytest
import torch

import itergp_ref as iref
import matern52_ref as m52
import wide_cases as wc

pytestmark = pytest.mark.gpu

TOL = 1e-11
KINDS = ["rbf", "matern32"]
#: (N, D, S): two rows; one row short of, at and past the 128-row workgroup, a ragged batch of 8 columns; the edges of the padded widths
#: 48 / 64 / 80 / 96 with a full group, a full group and a left-over pair, 8 + 3; several row blocks and column chunks
SHAPES = [(2, 40, 2), (127, 40, 3), (128, 40, 3), (129, 33, 5), (257, 48, 8), (300, 49, 2), (300, 64, 9), (129, 65, 11), (300, 77, 11),
          (300, 80, 4), (257, 81, 3), (300, 90, 8), (1100, 96, 11)]
M52_SHAPES = [(129, 33, 5), (300, 64, 9), (300, 77, 11), (300, 90, 8)]
PARENT_SHAPES = [(129, 33, 5), (300, 64, 9), (129, 65, 11), (300, 77, 11), (300, 90, 8)]


def _context(X, kind, hyp, dtype=torch.float64, **options):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, np.zeros(len(X)), 1, kind, dtype=dtype, device=torch.device("cuda", 0))
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, X[:1].copy(), 1e-6)
    return ctx


def _pairs(N, S, seed=0):
    rng = np.random.default_rng(2000 + seed + N + S)
    return rng.standard_normal((N, S)), rng.standard_normal((N, S))


def _problem(N, D, ell_factor=1.0, outlier=False):
    X, _y, _Z, hyp = wc.outlier_problem(N, D, 8, seed=D) if outlier else wc.problem(N, D, 8, seed=D, ell_factor=ell_factor)
    return X, hyp


@functools.lru_cache(maxsize=None)
def _reference(kind, N, D, S, ell_factor=1.0, outlier=False):
    """(values [D + 1], sums of absolute terms [D + 1]): one numpy evaluation per case, shared and never modified."""
    X, hyp = _problem(N, D, ell_factor, outlier)
    if ell_factor == 1.0:
        wc.informative(wc.dense(kind, X, hyp), hyp)
    U, V = _pairs(N, S)
    with m52.oracle_with_matern52():
        g = iref.bilinear_forms(kind, X, hyp.lengthscales, hyp.variance, U, V)
    want = np.concatenate([g["lengthscales"], [g["variance"]]])
    for a in (want, g["abs"]):
        a.setflags(write=False)
    return want, g["abs"]


def _singles(ctx, U, V):
    return sum(ctx.grad_kff_multi(U[:, b:b + 1], V[:, b:b + 1]) for b in range(U.shape[1]))


def _report(label, got, want, scale):
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print(f"{label}: largest difference {err.max():.2e} of the sum of absolute terms (entry {int(err.argmax())} of {len(err)})")
    return err


def test_statistic():
    X, hyp = _problem(200, 40)

    def stat(Xc, h, dtype=torch.float64, **options):
        ctx = _context(Xc, "rbf", h, dtype=dtype, **options)
        try:
            return ctx.get_stat("grad_multi_native")
        finally:
            ctx.close()

    assert stat(X, hyp) == 1
    assert stat(X, hyp, grad_multi_mid=0) == 0
    assert stat(X, hyp, wide_reg=0) == 0
    assert stat(X, hyp, dtype=torch.float32) == 0
    assert stat(*_problem(200, 97)) == 0
    assert stat(*_problem(200, 8)) == 1


def _check_reference(kind, shape, **options):
    N, D, S = shape
    X, hyp = _problem(N, D)
    want, scale = _reference(kind, N, D, S)
    U, V = _pairs(N, S)
    ctx = _context(X, kind, hyp, **options)
    try:
        assert ctx.get_stat("grad_multi_native") == 1
        got = ctx.grad_kff_multi(U, V)
        again = ctx.grad_kff_multi(U, V)
    finally:
        ctx.close()
    err = _report(f"N={N} D={D} S={S} {kind} {options}", got, want, scale)
    assert got.shape == (D + 1,)
    assert np.all(err <= TOL), (got, want, scale)
    assert np.array_equal(got, again)            # two calls: bitwise equal


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_D%d_S%d" % s)
def test_matches_the_numpy_bilinear_forms(shape, kind):
    _check_reference(kind, shape)


@pytest.mark.parametrize("shape", M52_SHAPES, ids=lambda s: "N%d_D%d_S%d" % s)
def test_matches_the_numpy_bilinear_forms_matern52(shape):
    _check_reference("matern52", shape)


def test_exact_level_matern_at_width_96():
    """The instance with a matrix row shared by four lanes (64-row workgroup): one row past it."""
    _check_reference("matern32", (65, 96, 3), precision=0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PARENT_SHAPES, ids=lambda s: "N%d_D%d_S%d" % s)
def test_against_the_single_passes_and_the_option(shape, kind):
    N, D, S = shape
    X, hyp = _problem(N, D)
    _want, scale = _reference(kind, N, D, S)
    U, V = _pairs(N, S)
    ctx = _context(X, kind, hyp)
    try:
        native = ctx.grad_kff_multi(U, V)
        singles = _singles(ctx, U, V)
        ctx.set_option("grad_multi_mid", 0)
        assert ctx.get_stat("grad_multi_native") == 0
        fallback = ctx.grad_kff_multi(U, V)
        ctx.set_option("grad_multi_mid", 1)
        back = ctx.grad_kff_multi(U, V)
        ctx.set_option("grad_multi_mid", 0)
        ctx.grad_kff_multi(U, V)
        ctx.set_option("grad_multi_mid", 1)
        back2 = ctx.grad_kff_multi(U, V)
    finally:
        ctx.close()
    e1 = _report(f"N={N} D={D} S={S} {kind} against the single passes", native, singles, scale)
    e2 = _report(f"N={N} D={D} S={S} {kind} against grad_multi_mid 0", native, fallback, scale)
    assert np.all(e1 <= 2 * TOL) and np.all(e2 <= 2 * TOL)
    assert np.array_equal(native, back) and np.array_equal(native, back2)


#: test_clamped_range_at_short_lengthscales: largest error of the SINGLE passes summed (the path this pass replaces) against the reference on
#: the lengthscale entries, in units of the sum of absolute terms, measured on an MI355X where it exceeds 1e-11 (Matern-3/2: 2.4e-12 and 6.7e-12)
SHORT_SINGLE_PASS_ERROR = {("rbf", 40): 2.61e-7, ("rbf", 77): 1.07e-4}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [40, 77])
def test_clamped_range_at_short_lengthscales(kind, D):
    """Lengthscales shortened until the kernel matrix is the identity to working precision (wide_cases.problem, ell_factor 0.12): no
    informative reference, so the native pass is held to the single passes of the same context, and to finite values.

    Matern-3/2 and the kappa entry of both kinds are held to 2e-11 of the sum of absolute terms.  The lengthscale entries of the RBF cases are
    not: every true term is negligible there (sums of absolute terms of 1e-7 .. 1e-6) and the moment form of the existing single pass leaves
    its round-off at the coincident pairs (i, i), as tests/test_gpu_grad_multi.py describes for the initial hyper-parameters.  Measured on an
    MI355X, S = 5, N = 300, RBF, largest error in units of that scale:
        D = 40: single passes summed against the reference 2.61e-7; native against the reference 1.25e-7, against the single passes 3.35e-7
        D = 77: single passes summed against the reference 1.07e-4; native against the reference 1.15e-4, against the single passes 1.50e-4
    so these entries are held to twice the measured error of the path they replace (SHORT_SINGLE_PASS_ERROR)."""
    N, S = 300, 5
    X, hyp = _problem(N, D, ell_factor=0.12)
    want, scale = _reference(kind, N, D, S, ell_factor=0.12)
    U, V = _pairs(N, S)
    ctx = _context(X, kind, hyp)
    try:
        assert ctx.get_stat("exp_clamp") == 1
        assert ctx.get_stat("grad_multi_native") == 1
        native = ctx.grad_kff_multi(U, V)
        singles = _singles(ctx, U, V)
    finally:
        ctx.close()
    _report(f"D={D} {kind} short lengthscales: the single passes against the reference", singles, want, scale)
    _report(f"D={D} {kind} short lengthscales: native against the reference", native, want, scale)
    err = _report(f"D={D} {kind} short lengthscales: native against the single passes", native, singles, scale)
    assert np.all(np.isfinite(native))
    assert err[D] <= 2 * TOL
    assert np.all(err[:D] <= max(2 * TOL, 2 * SHORT_SINGLE_PASS_ERROR.get((kind, D), 0.0)))


@pytest.mark.parametrize("kind", KINDS)
def test_clamped_range_on_informative_values(kind):
    """One far row widens the exponent range (wide_cases.outlier_problem) while every other kernel value stays where it was."""
    N, D, S = 300, 40, 5
    X, hyp = _problem(N, D, outlier=True)
    med = wc.informative(wc.dense(kind, X, hyp), hyp)
    want, scale = _reference(kind, N, D, S, outlier=True)
    U, V = _pairs(N, S)
    ctx = _context(X, kind, hyp)
    try:
        if kind == "rbf":
            assert ctx.get_stat("exp_clamp") == 1
        assert ctx.get_stat("grad_multi_native") == 1
        got = ctx.grad_kff_multi(U, V)
    finally:
        ctx.close()
    err = _report(f"far row, {kind}, median kernel value {med:.2f}", got, want, scale)
    assert np.all(err <= TOL)


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_precision_levels(kind, precision):
    N, D, S = 300, 77, 11
    X, hyp = _problem(N, D)
    want, scale = _reference(kind, N, D, S)
    U, V = _pairs(N, S)
    ctx = _context(X, kind, hyp, precision=precision)
    try:
        got = ctx.grad_kff_multi(U, V)
        singles = _singles(ctx, U, V)
    finally:
        ctx.close()
    tol = {1: TOL, 2: 1e-9}[precision]
    e1 = _report(f"{kind} precision {precision} against the reference", got, want, scale)
    e2 = _report(f"{kind} precision {precision} against the single passes", got, singles, scale)
    assert np.all(e1 <= tol) and np.all(e2 <= 2 * tol)


@pytest.mark.parametrize("kind", KINDS)
def test_equal_pairs_and_permutations(kind):
    N, D = 300, 77
    X, hyp = _problem(N, D)
    U, V = _pairs(N, 8, seed=5)
    with m52.oracle_with_matern52():
        scale1 = iref.bilinear_forms(kind, X, hyp.lengthscales, hyp.variance, U[:, :1], V[:, :1])["abs"]
        scale8 = iref.bilinear_forms(kind, X, hyp.lengthscales, hyp.variance, U, V)["abs"]
    ctx = _context(X, kind, hyp)
    try:
        one = ctx.grad_kff_multi(U[:, :1], V[:, :1])
        for S in (2, 5, 8, 11):
            many = ctx.grad_kff_multi(np.repeat(U[:, :1], S, axis=1), np.repeat(V[:, :1], S, axis=1))
            err = _report(f"{kind}: one pair {S} times", many, S * one, S * scale1)
            assert np.all(err <= 2 * TOL)
        full = ctx.grad_kff_multi(U, V)
        perm = np.random.default_rng(2).permutation(8)
        permuted = ctx.grad_kff_multi(U[:, perm], V[:, perm])
    finally:
        ctx.close()
    err = _report(f"{kind}: the pairs of one group permuted", permuted, full, scale8)
    assert np.all(err <= 2 * TOL)


@pytest.mark.parametrize("kind", KINDS)
def test_itergp_objective_and_grad_with_and_without_the_native_pass(kind):
    """t = 10 probes: S = 11 pairs in groups of 8 + 3.  The solve does not depend on the option: out4 bitwise; the gradients inside 2e-11 of the
    sums of absolute terms of the restatement's pairs (tests/itergp_ref.py: evaluate, the same fixed step count)."""
    N, D, k, t, iters = 300, 77, 8, 10, 5
    X, y, h, _Xnew = wc.itergp_case(N, D)
    eps = np.random.default_rng(3).standard_normal((t, k + N))
    with m52.oracle_with_matern52():
        base = iref.evaluate(kind, X, y, eps=eps, k=k, max_error=0.0, max_cg_iter=iters, **h)
    scale = base.grad["abs"]
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=torch.float64, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
    try:
        res = {}
        for opt in (1, 0):
            ctx.set_option("grad_multi_mid", opt)
            assert ctx.get_stat("grad_multi_native") == opt
            res[opt] = ctx.itergp_objective_and_grad(eps, torch.zeros(N, dtype=torch.float64, device=ctx.device), max_error=0.0, max_cg_iter=iters)
    finally:
        ctx.close()
    a, b = res[1], res[0]
    assert (a.lml, a.quad, a.logdet, a.logdet_P, a.steps) == (b.lml, b.quad, b.logdet, b.logdet_P, b.steps)
    ga = np.concatenate([a.grad["lengthscales"], [a.grad["variance"]]])
    gb = np.concatenate([b.grad["lengthscales"], [b.grad["variance"]]])
    err = _report(f"{kind}: gradient with the native pass against single passes", ga, gb, scale)
    assert np.all(err <= 2 * TOL)
    assert a.grad["noise"] == b.grad["noise"] and a.grad["mean"] == b.grad["mean"]
