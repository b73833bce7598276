"""The iterative exact-GP class on wide inputs: the predictive by batched solves (cglb_itergp_predict) against the dense tests/gpr_ref.py,
the Lanczos variance cache (cglb_itergp_var_cache, cglb_itergp_predict_cached) against its numpy restatement tests/love_ref.py, and one
run of the command line.  Problems: tests/wide_cases.py (standard-normal inputs, lengthscales ~ sqrt(D)).

Tolerances:
  * predictive: sqrt(2e-12 variance) + 1e-11 (N variance + noise) / noise - the bound of test_predictive_matches_the_dense_one
    (tests/test_gpu_itergp.py: max_error = 1e-12 bounds the K-norm error of every solve) with the kernel-value figure of the wide path,
    1e-11, times the condition number of K;
  * variance cache against the restatement, in units of the kernel variance f: 10x what a relative 1e-11 wobble of every kernel value does
    to the restatement on these very cases, never below 1e-10 (wide_cases.cache_tolerance).  tests/test_love_ref_wide_host.py measures
    it: at most 2.59e-11 f over the cases, ranks, kinds and three seeds (rank 33, Matern-3/2, D = 77; ranks 1 - 9 stay below 4e-12), so
    the tolerance is 2.6e-10 f;
  * exact limit rank = N against the exact variance 1e-9 f, as tests/test_gpu_itergp_var_cache.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpr_ref as ref
import love_ref as lref
import matern52_ref as m52
import wide_cases as wc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_EXACT = 1e-9


def _context(X, y, kind, h, k=8, **options):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=torch.float64, device=torch.device("cuda", 0))
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
    return ctx


@functools.lru_cache(maxsize=None)
def _dense_predictive(kind, N, D):
    X, y, h, Xnew = wc.itergp_case(N, D)
    wc.check_informative(kind, X, h)
    with m52.oracle_with_matern52():
        want = ref.evaluate(kind, X, y, with_grad=False, **h)
        return ref.predict(kind, X, want, h["lengthscales"], h["variance"], h["mean"], Xnew)


# (300, 40) and (300, 77): the shared-kernel product under the batched solves; (200, 120): Gram tiles and the fall-back product
@pytest.mark.parametrize("N,D", [(300, 40), (300, 77), (200, 120)])
@pytest.mark.parametrize("kind", wc.KINDS)
def test_predictive_matches_the_dense_one(kind, N, D):
    X, y, h, Xnew = wc.itergp_case(N, D)
    rm, rv = _dense_predictive(kind, N, D)
    bound = np.sqrt(2e-12 * h["variance"]) + 1e-11 * (N * h["variance"] + h["noise"]) / h["noise"]
    ctx = _context(X, y, kind, h)
    try:
        assert ctx.get_stat("matmat_native") == (1 if D <= 96 else 0)
        mean, var = ctx.itergp_predict(Xnew, max_error=1e-12)           # no evaluation yet: the preconditioner is built first
        ctx.itergp_objective_and_grad(np.random.default_rng(0).standard_normal((2, 8 + N)), torch.zeros(N, dtype=torch.float64, device=ctx.device),
                                      with_grad=False)
        mean2, var2 = ctx.itergp_predict(Xnew, max_error=1e-12)         # ... and this one starts from the alpha of that evaluation
    finally:
        ctx.close()
    for m, v in ((mean, var), (mean2, var2)):
        m, v = m.cpu().numpy(), v.cpu().numpy()
        print(f"{kind} N={N} D={D}: mean error {np.abs(m - rm).max():.2e}, variance error {np.abs(v - rv).max():.2e}, bound {bound:.2e}")
        assert m.shape == v.shape == (len(Xnew),)
        assert np.abs(m - rm).max() <= bound and np.abs(v - rv).max() <= bound


@functools.lru_cache(maxsize=None)
def _want(kind, N, D, r):
    """(f_var, J) of the restatement, computed once per case and never modified."""
    X, y, h, Xnew = wc.itergp_case(N, D)
    with m52.oracle_with_matern52():
        v, c = lref.predict_var(kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Xnew, r)
    v.setflags(write=False)
    return v, c.J


@pytest.mark.parametrize("case", wc.CACHE_CASES, ids=lambda c: "N%d_D%d" % c)
@pytest.mark.parametrize("kind", wc.KINDS)
def test_variance_cache_matches_the_restatement(kind, case):
    """Measured on the host (tests/test_love_ref_wide_host.py), largest change of the restatement under a 1e-11 wobble in units of f:
    2.59e-11 (rank 33), below 4e-12 at ranks 1 - 9; tolerance 10x the largest = 2.6e-10."""
    N, D = case
    X, y, h, Xnew = wc.itergp_case(N, D)
    wc.check_informative(kind, X, h)
    tol = wc.cache_tolerance()
    ctx = _context(X, y, kind, h)
    try:
        for r in wc.CACHE_RANKS:
            want, J = _want(kind, N, D, r)
            assert ctx.itergp_var_cache(r) == J     # rank_out exact
            assert ctx.get_stat("itergp_cache_request") == r
            mean, var = ctx.itergp_predict_cached(Xnew)
            got = var.cpu().numpy()
            err = np.abs(got - want).max() / h["variance"]
            print(f"N={N} D={D} {kind} r={r} J={J}: largest variance error {err:.2e} f, tolerance {tol:.1e}")
            assert got.shape == (len(Xnew),) and np.all(np.isfinite(mean.cpu().numpy()))
            assert err <= tol
    finally:
        ctx.close()


def test_variance_cache_beyond_the_register_resident_width():
    """D = 120: the cache is built through the Gram-tile mat-vec; same tolerance (the wobble figure is that of every wide product)."""
    N, D, kind, r = 200, 120, "matern32", 9
    X, y, h, Xnew = wc.itergp_case(N, D)
    wc.check_informative(kind, X, h)
    want, J = _want(kind, N, D, r)
    ctx = _context(X, y, kind, h)
    try:
        assert ctx.itergp_var_cache(r) == J
        got = ctx.itergp_predict_cached(Xnew)[1].cpu().numpy()
    finally:
        ctx.close()
    err = np.abs(got - want).max() / h["variance"]
    print(f"N={N} D={D}: largest variance error {err:.2e} f")
    assert err <= wc.cache_tolerance()


def test_exact_limit_on_the_device():
    N, D, kind = 67, 40, "matern32"
    X, y, h, Xnew = wc.itergp_case(N, D)
    wc.check_informative(kind, X, h)
    ctx = _context(X, y, kind, h)
    try:
        assert ctx.itergp_var_cache(N) == N
        got = ctx.itergp_predict_cached(Xnew)[1].cpu().numpy()
    finally:
        ctx.close()
    exact = lref.exact_var(kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Xnew)
    err = np.abs(got - exact).max() / h["variance"]
    print(f"N={N} D={D}: J = N, largest error against the exact variance {err:.2e} f")
    assert err <= TOL_EXACT


def test_against_the_solves_of_the_existing_path():
    """The cached variance is an upper bound of what the batched solves give, and the mean is the same call: two contexts in the same state."""
    N, D, r, kind = 300, 40, 33, "matern32"
    X, y, h, Xnew = wc.itergp_case(N, D)
    a, b = _context(X, y, kind, h), _context(X, y, kind, h)
    try:
        mean_a, var_a = a.itergp_predict(Xnew, max_error=1e-10)
        b.itergp_var_cache(r)
        mean_b, var_b = b.itergp_predict_cached(Xnew, max_error=1e-10)
        mean_a, var_a, mean_b, var_b = [t.cpu().numpy() for t in (mean_a, var_a, mean_b, var_b)]
    finally:
        a.close()
        b.close()
    print(f"cached - solved variance: {np.min(var_b - var_a):.2e} .. {np.max(var_b - var_a):.2e}")
    assert np.all(var_b >= var_a - 1e-8 * h["variance"])
    assert np.array_equal(mean_a, mean_b)


def test_set_hypers_invalidates_the_cache():
    N, D, r, kind = 300, 77, 9, "rbf"
    X, y, h, Xnew = wc.itergp_case(N, D)
    ctx = _context(X, y, kind, h)
    try:
        with pytest.raises(RuntimeError, match="call order"):
            ctx.itergp_predict_cached(Xnew)                                 # no cache yet
        assert ctx.itergp_var_cache(r) == r
        first = ctx.itergp_predict_cached(Xnew)[1].cpu().numpy()
        h2 = dict(h, noise=0.3)
        ctx.set_hypers(h2["lengthscales"], h2["variance"], h2["noise"], h2["mean"], X[:8].copy(), 1e-6)
        assert ctx.get_stat("itergp_cache_request") == 0
        with pytest.raises(RuntimeError, match="call order"):
            ctx.itergp_predict_cached(Xnew)                                 # the cache belonged to the old hyper-parameters
        assert ctx.itergp_var_cache(r) == r
        again = ctx.itergp_predict_cached(Xnew)[1].cpu().numpy()
        want, _ = lref.predict_var(kind, X, y, h2["lengthscales"], h2["variance"], h2["noise"], h2["mean"], Xnew, r)
        assert np.abs(again - want).max() <= wc.cache_tolerance() * h["variance"]
        assert np.abs(again - first).max() > 1e-6                          # ... and not the variances of the old cache
    finally:
        ctx.close()


def test_cli_end_to_end_on_a_wide_set(tmp_path):
    from cglb_amd.backend import jsonio
    run = tmp_path / "itergp_wide"
    cmd = [sys.executable, "-m", "cglb_amd.cli", "-b", "hip", "-t", "fp64", "-l", str(run), "train", "-d", "synthetic-300-40", "-n", "3", "-o", "adam_0.1",
           "gpr", "-m", "itergp", "-k", "Matern32", "--pred-var-rank", "33"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(run / "results.json") as f:
        results = jsonio.load(f)
    for key in ("loss", "lml", "train/rmse", "train/nlpd", "test/rmse", "test/nlpd"):
        assert key in results and np.isfinite(float(results[key])), key
