"""The shared-kernel product K_ff V at mid widths (32 < D <= 96, fp64: cglb_amd/csrc/kernels_kff_multi_mid.hip) against the dense oracle,
against the single mat-vec, in its bitwise guarantees and under the batched PCG.  Problems: tests/wide_cases.py.

Tolerances: per column 1e-11 of the largest reference entry, the figure tests/test_gpu_wide.py holds the single mid-width mat-vec to, and
twice that against the context's own mat-vec (two results inside 1e-11 of one reference); precision level 2 at 1e-9, as
tests/test_gpu_multi_output.py holds the narrow product; the solve at the figures of its test_pcg_multi_against_lockstep_loop."""
import functools

import numpy as np
import pytest
import torch

import multi_output_ref as mref
import wide_cases as wc
from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-11
COLUMNS = 9   # a full group of 8 and the single left-over; the shorter groups come from the leading 2 .. 7 columns


def make_ctx(kind, X, Y, hyp, dtype=torch.float64, **options):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, Y, hyp.Z.shape[0], kind, dtype=dtype)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    return ctx


def check_columns(out, ref, what, tol=TOL, scale_of=None):
    """Column by column: |out - ref| <= tol * max |scale_of| (the reference itself unless another array gives the scale)."""
    assert out.shape == ref.shape
    scale_of = ref if scale_of is None else scale_of
    for b in range(ref.shape[1]):
        err = np.abs(out[:, b] - ref[:, b]).max()
        scale = np.abs(scale_of[:, b]).max()
        print(f"{what} column {b}: {err / scale:.3g} of the largest entry (tolerance {tol:.0e})")
        assert err <= tol * scale, f"{what} column {b}: {err:.3g} against {tol * scale:.3g}"


def product_and_singles(ctx, V, P):
    out = ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy()
    single = np.stack([ctx.matvec(torch.from_numpy(V[:, b].copy())).cpu().numpy() for b in range(P)], axis=1)
    return out, single


def check_product(ctx, V, ref, what, columns=(COLUMNS, 2, 3, 4, 7)):
    for P in columns:
        out, single = product_and_singles(ctx, V, P)
        check_columns(out, ref[:, :P], f"{what} P={P}")
        check_columns(out, single, f"{what} P={P} against matvec", 2 * TOL, scale_of=ref[:, :P])


def test_matmat_native_statistic():
    """1 where a product of two or more columns runs through a shared-kernel instance, 0 where it falls back to single mat-vecs."""
    def stat(kind, N, D, dtype=torch.float64, ell_factor=1.0, **options):
        X, _y, _Z, hyp = wc.problem(N, D, 8, seed=D, ell_factor=ell_factor)
        if dtype == torch.float32:
            X = X.astype(np.float32)
        ctx = make_ctx(kind, X, np.zeros(N, dtype=X.dtype), hyp, dtype=dtype, **options)
        try:
            return ctx.get_stat("matmat_native")
        finally:
            ctx.close()
    assert stat("rbf", 200, 40) == 1
    assert stat("rbf", 200, 40, wide_reg=0) == 0
    assert stat("rbf", 200, 40, dtype=torch.float32) == 0
    assert stat("rbf", 200, 97) == 0
    # the narrow scope is unchanged: the unclamped exponent range only
    assert stat("rbf", 200, 8) == 1
    assert stat("rbf", 200, 8, ell_factor=0.12) == 0
    for D in (33, 48, 49, 64, 65, 80, 81, 96):
        for kind in wc.KINDS:
            assert stat(kind, 100, D) == 1, (kind, D)


SHAPES = [(1333, D) for D in (33, 48, 49, 64, 65, 80, 81, 96)] + [(N, D) for N in (37, 300) for D in (33, 96)]


# N: shorter than one 64-row block | not a multiple of 64 | more than four row blocks with a ragged tail and a column count that is no
# multiple of 16; D: both ends of every padded width; sym_chunk 16 (many chunks, several per span) and the default
@pytest.mark.parametrize("N,D", SHAPES)
@pytest.mark.parametrize("kind", wc.KINDS)
def test_matmat_against_dense_and_matvec(kind, N, D):
    X, hyp, V, ref = wc.matmat_case(kind, N, D)
    for chunk in (16, 0):
        ctx = make_ctx(kind, X, np.zeros(N), hyp, sym_chunk=chunk)
        assert ctx.get_stat("matmat_native") == 1
        check_product(ctx, V, ref, f"{kind} N={N} D={D} sym_chunk={chunk}", columns=(COLUMNS, 2, 3, 4, 7) if chunk else (COLUMNS, 5))
        ctx.close()


@pytest.mark.parametrize("order", [0, 1])
def test_matmat_in_both_work_orders(order):
    X, hyp, V, ref = wc.matmat_case("matern32", 1333, 77)
    ctx = make_ctx("matern32", X, np.zeros(1333), hyp, sym_order=order, sym_chunk=128)
    check_product(ctx, V, ref, f"sym_order {order}", columns=(COLUMNS, 4))
    ctx.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("kind", wc.KINDS)
def test_matmat_precision_levels(kind, precision):
    X, hyp, V, ref = wc.matmat_case(kind, 300, 96)
    ctx = make_ctx(kind, X, np.zeros(300), hyp, sym_chunk=16, precision=precision)
    assert ctx.get_stat("matmat_native") == 1
    out, single = product_and_singles(ctx, V, COLUMNS)
    ctx.close()
    # level 2 trades kernel values of ~1e-10 for speed: held to 1e-9, and every level to its own single mat-vec
    tol = {0: TOL, 1: TOL, 2: 1e-9}[precision]
    check_columns(out, ref, f"{kind} precision {precision}", tol)
    check_columns(out, single, f"{kind} precision {precision} against matvec", 2 * tol, scale_of=ref)


@pytest.mark.parametrize("D", [40, 96])
@pytest.mark.parametrize("kind", wc.KINDS)
def test_clamped_instances(kind, D):
    """ell_factor 0.12 (the value of tests/test_gpu_wide.py) selects the range-clamped instances.  At these lengthscales the off-diagonal
    kernel values vanish, so this reference cannot be asked for a median of 0.01: test_clamped_instance_on_informative_values does that."""
    N = 1333
    X, hyp, V, ref = wc.matmat_case(kind, N, D, ell_factor=0.12)
    ctx = make_ctx(kind, X, np.zeros(N), hyp, sym_chunk=16)
    assert ctx.get_stat("matmat_native") == 1
    check_product(ctx, V, ref, f"{kind} D={D} clamped", columns=(COLUMNS, 3))
    ctx.close()
    # the same lengthscale rule on a narrow context is refused by the narrow product: the range is the clamped one
    Xn, _y, _Z, hn = wc.problem(200, 8, 8, seed=8, ell_factor=0.12)
    narrow = make_ctx("rbf", Xn, np.zeros(200), hn)
    assert narrow.get_stat("matmat_native") == 0
    narrow.close()


@pytest.mark.parametrize("D", [40, 96])
def test_clamped_instance_on_informative_values(D):
    """One far row widens the RBF exponent range beyond the unclamped 2^x (wide_cases.outlier_problem) while every other kernel value
    stays of order 0.1: the clamped instance on a reference that passes the median check.  That the range is the clamped one is read off
    a narrow context with the same far row, whose product then falls back."""
    N = 1333
    X, hyp, V, ref = wc.matmat_case("rbf", N, D, outlier=True)
    ctx = make_ctx("rbf", X, np.zeros(N), hyp, sym_chunk=16)
    assert ctx.get_stat("matmat_native") == 1
    check_product(ctx, V, ref, f"D={D} far row", columns=(COLUMNS, 3))
    ctx.close()
    Xn, _y, _Z, hn = wc.outlier_problem(200, 8, 8, seed=8)
    narrow = make_ctx("rbf", Xn, np.zeros(200), hn)
    assert narrow.get_stat("matmat_native") == 0
    narrow.close()
    Xu, _y, _Z, hu = wc.problem(200, 8, 8, seed=8)
    narrow = make_ctx("rbf", Xu, np.zeros(200), hu)
    assert narrow.get_stat("matmat_native") == 1
    narrow.close()


@pytest.mark.parametrize("kind", wc.KINDS)
def test_bitwise_properties(kind):
    N, D = 1333, 77
    X, hyp, V, ref = wc.matmat_case(kind, N, D)
    ctx = make_ctx(kind, X, np.zeros(N), hyp, sym_chunk=16)
    assert ctx.get_stat("matmat_native") == 1
    W = V[:, :4].copy()
    W[:, 2] = 0.0
    out = ctx.matmat(torch.from_numpy(W)).cpu().numpy()
    assert not out[:, 2].any()                            # noise * 0 exactly
    check_columns(out[:, [0, 1, 3]], ref[:, [0, 1, 3]], "beside a zero column")
    same = ctx.matmat(torch.from_numpy(np.repeat(V[:, :1], 3, axis=1))).cpu().numpy()
    assert same[:, 0].tobytes() == same[:, 1].tobytes() == same[:, 2].tobytes()
    # run to run, and under a permutation of the columns inside one group: bitwise
    for P in (2, 4, 7, 8):
        base = ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy()
        assert base.tobytes() == ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy().tobytes()
        perm = np.random.default_rng(P).permutation(P)
        out = ctx.matmat(torch.from_numpy(V[:, perm].copy())).cpu().numpy()
        assert out.tobytes() == np.ascontiguousarray(base[:, perm]).tobytes()
    p = torch.from_numpy(V[:, 0].copy())
    assert ctx.matmat(p).reshape(-1).cpu().numpy().tobytes() == ctx.matvec(p).cpu().numpy().tobytes()
    ctx.close()


def test_alternating_matvec_and_matmat_keep_their_work_lists_apart():
    """One context, mat-vec and mat-mat calls in turn under a shuffled sequence of sym_chunk and sym_order: each kernel caches its own work
    list, keyed by what it was built for.  Every result is held to the dense oracle and every repeat of a configuration to the bits of its
    first occurrence."""
    N, D, kind = 1333, 77, "rbf"
    X, hyp, V, ref = wc.matmat_case(kind, N, D)
    ctx = make_ctx(kind, X, np.zeros(N), hyp)
    settings = [(chunk, order) for chunk in (64, 256, 1024) for order in (0, 1)]
    rng = np.random.default_rng(17)
    vec = [(c, o, 1) for c, o in settings] * 3
    mat = [(c, o, S) for c, o in settings for S in (2, 3, 8)]
    rng.shuffle(vec)
    rng.shuffle(mat)
    first = {}
    for step, (chunk, order, S) in enumerate(x for pair in zip(vec, mat) for x in pair):
        ctx.set_option("sym_chunk", chunk)
        ctx.set_option("sym_order", order)
        if S == 1:
            out = ctx.matvec(torch.from_numpy(V[:, 0].copy())).cpu().numpy()[:, None]
        else:
            out = ctx.matmat(torch.from_numpy(V[:, :S].copy())).cpu().numpy()
        what = f"step {step}: chunk {chunk} order {order} S {S}"
        err = np.abs(out - ref[:, :S]).max(axis=0) / np.abs(ref[:, :S]).max(axis=0)
        assert err.max() <= TOL, what
        assert first.setdefault((chunk, order, S), out.tobytes()) == out.tobytes(), what + " differs from its first occurrence"
    assert len(first) == 24
    ctx.close()


@functools.lru_cache(maxsize=None)
def solve_case(kind, D, P):
    N, M = 300, 24
    X, Y, hyp0 = mref.problem(N, D, M, P, seed=11)
    ls = np.random.default_rng(111).uniform(0.8, 1.6, size=D) * np.sqrt(D)
    hyp = orc.Hypers(ls, wc.VARIANCE, wc.NOISE, wc.MEAN, hyp0.Z, 1e-6)
    cov = wc.dense(kind, X, hyp)
    wc.informative(cov, hyp)
    terms = orc.common_terms(kind, X, hyp)
    pre = lambda r: orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r)
    V, steps, half = mref.stable_steps(cov, Y - hyp.mean, np.zeros_like(Y), pre, 1.0)
    return X, Y, hyp, V, steps, half


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("D", [40, 77])
@pytest.mark.parametrize("kind", ["rbf", "matern32"])
def test_pcg_multi_against_lockstep_loop(kind, D, P):
    X, Y, hyp, Vref, steps, half = solve_case(kind, D, P)
    assert 0 < steps <= 40
    ctx = make_ctx(kind, X, Y, hyp, sym_chunk=16)
    assert ctx.get_stat("matmat_native") == 1
    ctx.setup()
    V, st, total, cols = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64))
    print(f"steps {st} (ref {steps}); 1/2 r^T P r {cols} (ref {half})")
    assert st == steps
    np.testing.assert_allclose(V.cpu().numpy(), Vref, rtol=0, atol=1e-8 * np.abs(Vref).max())
    np.testing.assert_allclose(cols, half, rtol=1e-5)
    assert total == pytest.approx(half.sum(), rel=1e-5) and total <= 1.0
    ctx.close()
