"""The multi-pair gradient pass (cglb_grad_kff_multi, cglb_amd/csrc/kernels_grad_multi.hip) against numpy bilinear forms
(tests/itergp_ref.py: bilinear_forms): sum_b u_b^T (dK_ff / dl_d) v_b for every d and sum_b u_b^T kappa v_b.

Shapes: one lane (N = 1), two rows, a ragged wave (63), one row past the row block of 256 R rows for R = 1 (257 at D > 8) and R = 2 (513 at
D <= 8), several row blocks and column chunks (1100); padded widths 1, 3, 8, 12, 20; S = 1, 2, 3, 5, 8 (the four padded group sizes), 9 (a
group of 8 and a single pair) and 11 (8 + 3).  Tolerance: 1e-11 of the sum of the absolute values of the terms, the scale the single-pass
gradient tests use.

The fall-back (D = 40: S single passes of the existing mid-width kernel and the kappa sums from one product) is checked once, at the
trained-like hyper-parameters, where the kernel matrix is not the identity to working precision.  At the initial ones (lengthscale 1 at
D = 40: off-diagonal kernel values around e^-40) every true term is negligible and the Gram/moment form of that existing single pass leaves
its round-off at the coincident pair (i, i), which direct differences make exactly zero: measured on an MI355X at N = 300, S = 3, RBF, up to
3.1e-14 absolute on lengthscale entries whose sums of absolute terms are 2e-5 .. 8e-5 (5e-10 of that scale, against the 1e-11 asked here);
the native kernel of this file uses direct differences and has no such term."""
import functools

import numpy as np
import pytest
import torch

import gpr_ref as ref
import itergp_ref as iref

pytestmark = pytest.mark.gpu

KINDS = ["rbf", "matern32"]
#: (N, D, S)
SHAPES = [(1, 1, 1), (2, 3, 2), (63, 3, 3), (257, 1, 9), (257, 12, 5), (513, 8, 8), (513, 3, 11), (1100, 8, 2), (1100, 20, 11)]
EPS = 2.0 ** -53


def _context(X, y, kind, h, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, 1, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:1].copy(), 1e-6)
    return ctx


def _pairs(N, S, seed=0):
    rng = np.random.default_rng(1000 + seed + N + S)
    return rng.standard_normal((N, S)), rng.standard_normal((N, S))


@functools.lru_cache(maxsize=None)
def _reference(kind, N, D, S, trained):
    """One numpy evaluation per case, shared and never modified: (values [D + 1], sums of absolute terms [D + 1])."""
    X, _ = ref.problem(N, D)
    h = ref.hypers(D, trained)
    U, V = _pairs(N, S)
    g = iref.bilinear_forms(kind, X, h["lengthscales"], h["variance"], U, V)
    return np.concatenate([g["lengthscales"], [g["variance"]]]), g["abs"]


def _check(shape, kind, trained):
    N, D, S = shape
    X, y = ref.problem(N, D)
    want, scale = _reference(kind, N, D, S, trained)
    U, V = _pairs(N, S)
    ctx = _context(X, y, kind, ref.hypers(D, trained))
    try:
        got = ctx.grad_kff_multi(U, V)
        again = ctx.grad_kff_multi(U, V)
    finally:
        ctx.close()
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print(f"N={N} D={D} S={S} {kind} trained={trained}: largest error {err.max():.2e} of the sum of absolute terms")
    assert got.shape == (D + 1,)
    assert np.all(np.abs(got - want) <= 1e-11 * scale), (got, want, scale)
    assert np.array_equal(got, again)            # two calls: bitwise equal


@pytest.mark.parametrize("trained", [False, True], ids=["init", "trained"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_D%d_S%d" % s)
def test_matches_the_numpy_bilinear_forms(shape, kind, trained):
    _check(shape, kind, trained)


@pytest.mark.parametrize("kind", KINDS)
def test_fall_back_for_wide_inputs(kind):
    _check((300, 40, 3), kind, True)


@pytest.mark.parametrize("kind", KINDS)
def test_equal_pairs_permutations_and_the_variance(kind):
    """Round-off bound of these identities: the pair weights differ by at most S roundings and every partial sum is a chain of at most N
    additions, so the results differ by at most (N + S) 2^-53 of the sum of the absolute terms, doubled for the two sides compared."""
    N, D = 1100, 8
    X, y = ref.problem(N, D)
    h = dict(ref.hypers(D, True), variance=1.7)
    U, V = _pairs(N, 8, seed=5)
    ctx = _context(X, y, kind, h)
    try:
        full = ctx.grad_kff_multi(U, V)
        perm = np.random.default_rng(2).permutation(8)
        permuted = ctx.grad_kff_multi(U[:, perm], V[:, perm])
        for S in (2, 5, 8, 11):
            one = ctx.grad_kff_multi(U[:, :1], V[:, :1])
            many = ctx.grad_kff_multi(np.repeat(U[:, :1], S, axis=1), np.repeat(V[:, :1], S, axis=1))
            scale1 = iref.bilinear_forms(kind, X, h["lengthscales"], h["variance"], U[:, :1], V[:, :1])["abs"]
            print(f"{kind} S={S}: {np.abs(many - S * one).max():.2e} against the bound {(2 * (N + S) * EPS * S * scale1).min():.2e}")
            assert np.all(np.abs(many - S * one) <= 2 * (N + S) * EPS * S * scale1)
    finally:
        ctx.close()
    g = iref.bilinear_forms(kind, X, h["lengthscales"], h["variance"], U, V)
    want = np.concatenate([g["lengthscales"], [g["variance"]]])
    assert np.all(np.abs(full - want) <= 1e-11 * g["abs"])       # the variance 1.7 scales the lengthscale entries and not the kappa sum
    assert np.all(np.abs(permuted - full) <= 2 * (N + 8) * EPS * g["abs"])


def test_refusals():
    N, D = 65, 3
    X, y = ref.problem(N, D)
    h = ref.hypers(D, False)
    U, V = _pairs(N, 2)
    ctx = _context(X, y, "rbf", h, dtype=torch.float32)
    try:
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.grad_kff_multi(U, V)
    finally:
        ctx.close()
    ctx = _context(X, y, "rbf", h)
    try:
        with pytest.raises(ValueError):
            ctx.grad_kff_multi(U, V[:, :1])                       # U and V disagree on the number of pairs
        ctx.set_option("logdet_bound", 1)
        with pytest.raises(ValueError, match="logdet_bound 0"):
            ctx.grad_kff_multi(U, V)
        ctx.set_option("logdet_bound", 0)
        assert np.all(np.isfinite(ctx.grad_kff_multi(U, V)))      # the context is still usable
    finally:
        ctx.close()
