"""The Lanczos variance cache of the iterative exact-GP class (cglb_itergp_var_cache, cglb_itergp_predict_cached) against its numpy
restatement tests/love_ref.py, against the exact predictive of tests/gpr_ref.py where the two must agree, and through the product interface.

Tolerances, all in units of the kernel variance f:
  * against the restatement 1e-10: tests/test_love_ref_host.py measures what a relative 1e-13 wobble of every kernel value (the accuracy of
    the default precision level) does to the restatement on these very cases and holds it below 1e-11 (measured <= 3.2e-13), and shows that
    every planted kernel defect misses 1e-10 by more than 100x;
  * exact limit J = N against gpr_ref.predict 1e-9; after an early stop (RBF) 1e-7 (the restatement itself: 3.7e-10 at this case).
"""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_REF, TOL_EXACT, TOL_EARLY = 1e-10, 1e-9, 1e-7


def _context(X, y, kind, h, k=6):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=torch.float64, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
    return ctx


@functools.lru_cache(maxsize=None)
def _want(kind, N, D, r):
    """(f_var, J) of the restatement, computed once per case and never modified."""
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    with m52.oracle_with_matern52():
        v, c = lref.predict_var(kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], lref.new_points(N, D), r)
    return v, c.J


@functools.lru_cache(maxsize=None)
def _exact(kind, N, D):
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    with m52.oracle_with_matern52():
        return lref.exact_var(kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], lref.new_points(N, D))


CASES = [(c, k) for c in lref.CASES for k in ("matern32", "matern52")] + [((300, 3), "rbf")]


@pytest.mark.parametrize("case,kind", CASES, ids=lambda v: v if isinstance(v, str) else "N%d_D%d" % v)
def test_matches_the_restatement(case, kind):
    N, D = case
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    Xn = lref.new_points(N, D)
    ctx = _context(X, y, kind, h)
    try:
        for r in ([33] if kind == "rbf" else lref.RANKS):
            want, J = _want(kind, N, D, r)
            if kind == "rbf":
                assert J == r                       # no early stop in the restatement at this rank
            assert ctx.itergp_var_cache(r) == J     # rank_out exact
            assert ctx.get_stat("itergp_cache_request") == r
            mean, var = ctx.itergp_predict_cached(Xn)
            got = var.cpu().numpy()
            err = np.abs(got - want).max() / h["variance"]
            print(f"N={N} D={D} {kind} r={r} J={J}: largest variance error {err:.2e} f, tolerance {TOL_REF:.0e}; cache {ctx.get_stat('itergp_cache_ms'):.2f} ms, "
                  f"variance {ctx.get_stat('itergp_var_ms'):.3f} ms")
            assert got.shape == (len(Xn),) and np.all(np.isfinite(mean.cpu().numpy()))
            assert err <= TOL_REF
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [(40, 3), (67, 2)], ids=lambda c: "N%d_D%d" % c)
def test_exact_limit_on_the_device(case):
    N, D = case
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    ctx = _context(X, y, "matern32", h)
    try:
        assert ctx.itergp_var_cache(N) == N
        got = ctx.itergp_predict_cached(lref.new_points(N, D))[1].cpu().numpy()
    finally:
        ctx.close()
    err = np.abs(got - _exact("matern32", N, D)).max() / h["variance"]
    print(f"N={N} D={D}: J = N, largest error against the exact variance {err:.2e} f")
    assert err <= TOL_EXACT


def test_early_stop():
    N, D = 67, 2
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    ctx = _context(X, y, "rbf", h)
    try:
        J = ctx.itergp_var_cache(N)
        got = ctx.itergp_predict_cached(lref.new_points(N, D))[1].cpu().numpy()
    finally:
        ctx.close()
    err = np.abs(got - _exact("rbf", N, D)).max() / h["variance"]
    print(f"RBF N={N} D={D}: J = {J} (restatement {_want('rbf', N, D, N)[1]}), largest error against the exact variance {err:.2e} f")
    assert 1 <= J < N
    assert err <= TOL_EARLY


def test_against_the_solves_of_the_existing_path():
    """The cached variance is an upper bound of what the batched solves give, and the mean is the same call: two contexts in the same state."""
    N, D, r = 300, 3, 33
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    Xn = lref.new_points(N, D)
    a, b = _context(X, y, "matern32", h), _context(X, y, "matern32", h)
    try:
        mean_a, var_a = a.itergp_predict(Xn, max_error=1e-10)
        b.itergp_var_cache(r)
        mean_b, var_b = b.itergp_predict_cached(Xn, max_error=1e-10)
        mean_a, var_a, mean_b, var_b = [t.cpu().numpy() for t in (mean_a, var_a, mean_b, var_b)]
    finally:
        a.close()
        b.close()
    print(f"cached - solved variance: {np.min(var_b - var_a):.2e} .. {np.max(var_b - var_a):.2e}")
    assert np.all(var_b >= var_a - 1e-8 * h["variance"])
    assert np.array_equal(mean_a, mean_b)


def test_cache_validity_and_reuse():
    N, D, r = 300, 3, 9
    X, y = ref.problem(N, D)
    h = lref.hypers(D)
    Xn = lref.new_points(N, D)
    ctx = _context(X, y, "matern52", h)
    try:
        with pytest.raises(RuntimeError, match="call order"):
            ctx.itergp_predict_cached(Xn)                                   # no cache yet
        ctx.itergp_var_cache(r)
        first = ctx.itergp_predict_cached(Xn)[1].cpu().numpy()
        h2 = dict(h, noise=0.3)
        ctx.set_hypers(h2["lengthscales"], h2["variance"], h2["noise"], h2["mean"], X[:6].copy(), 1e-6)
        assert ctx.get_stat("itergp_cache_request") == 0
        with pytest.raises(RuntimeError, match="call order"):
            ctx.itergp_predict_cached(Xn)                                   # the cache belonged to the old hyper-parameters
        with pytest.raises(ValueError):
            ctx.itergp_var_cache(0)
        with pytest.raises(ValueError):
            ctx.itergp_var_cache(N + 1)
        # rebuild, then 4097 -> 5 -> 4097 new points through the same buffers
        assert ctx.itergp_var_cache(r) == r
        big = np.concatenate([Xn, np.random.default_rng(2).standard_normal((4097 - len(Xn), D))], axis=0)
        v1 = ctx.itergp_predict_cached(big)[1].cpu().numpy()
        v2 = ctx.itergp_predict_cached(big[:5])[1].cpu().numpy()
        v3 = ctx.itergp_predict_cached(big)[1].cpu().numpy()
        assert np.array_equal(v1, v3) and np.array_equal(v1[:5], v2)
        with m52.oracle_with_matern52():
            want, _ = lref.predict_var("matern52", X, y, h2["lengthscales"], h2["variance"], h2["noise"], h2["mean"], Xn, r)
        assert np.abs(v1[:len(Xn)] - want).max() <= TOL_REF * h["variance"]
        assert np.abs(v1[:len(Xn)] - first).max() > 1e-6                  # ... and not the variances of the old cache
        # a second build on the same inputs: bitwise equal variances
        assert ctx.itergp_var_cache(r) == r
        assert np.array_equal(ctx.itergp_predict_cached(big)[1].cpu().numpy(), v1)
        # var_rank of itergp_predict: builds when the valid cache has another rank, and only then
        v33 = ctx.itergp_predict(Xn, var_rank=33)[1].cpu().numpy()
        assert ctx.get_stat("itergp_cache_request") == 33
        assert np.all(v33 <= v1[:len(Xn)] + 1e-12)                         # the bound tightens with the rank
    finally:
        ctx.close()


# ---- through the backend interface and the command line -------------------------------------------------------------------------------
@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


def _model_hypers(backend, model):
    p = backend.model_parameters(model)
    return (np.asarray(p[".kernel.lengthscales"], dtype=np.float64).reshape(-1), float(p[".kernel.variance"]), float(p[".likelihood.variance"]),
            float(p[".mean_function.c"]))


def test_predictor_and_metrics_take_the_rank(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import PredictIterGPR, gaussian
    N, D = 300, 3
    X, y = ref.problem(N, D)
    Xt = lref.new_points(N, D, 20)
    yt = np.sin(Xt.sum(axis=1))
    model = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), (X, y))
    assert model.pred_var_rank == 0 and config.IterGPRConfig(config.Matern32Config()).pred_var_rank == 0
    ls, var, noise, c = _model_hypers(backend, model)
    want, _ = lref.predict_var("matern32", X, y, ls, var, noise, c, Xt, 33)
    f_mean, f_var = PredictIterGPR(model, var_rank=33)(torch.as_tensor(Xt))
    assert f_var.shape == (20, 1)
    assert np.abs(f_var.cpu().numpy().reshape(-1) - want).max() <= TOL_REF * var
    # the model's own rank, through the metrics: what the library call of the metrics received and returned
    ranked = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8, pred_var_rank=33), (X, y))
    calls, library_call = [], ranked.hip.itergp_predict

    def spy(xnew, *args, **kwargs):
        out = library_call(xnew, *args, **kwargs)
        calls.append((kwargs.get("var_rank"), out))
        return out
    ranked.hip.itergp_predict = spy
    metrics = backend.metrics_fn(ranked, ((X, y), (Xt, yt)))()
    assert len(calls) == 1 and calls[0][0] == 33
    m_all, v_all = [t.cpu().numpy().reshape(-1) for t in calls[0][1]]
    want_all, _ = lref.predict_var("matern32", X, y, ls, var, noise, c, np.concatenate([X, Xt], axis=0), 33)
    assert np.abs(v_all - want_all).max() <= TOL_REF * var
    lpd = gaussian(torch.as_tensor(yt).reshape(-1, 1), torch.as_tensor(m_all[N:]).reshape(-1, 1), torch.as_tensor(want_all[N:]).reshape(-1, 1) + noise)
    print(f"test/nlpd {metrics['test/nlpd']!r} against {-float(lpd.mean())!r} from the restatement's variances")
    assert abs(metrics["test/nlpd"] + float(lpd.mean())) <= 1e-8
    # rank 0 is the path of a model built without the field: bitwise
    zero = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8, pred_var_rank=0), (X, y))
    plain = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), (X, y))
    got0 = [t.cpu().numpy() for t in PredictIterGPR(zero)(torch.as_tensor(Xt))]
    ref0 = [t.cpu().numpy() for t in PredictIterGPR(plain)(torch.as_tensor(Xt))]
    assert np.array_equal(got0[0], ref0[0]) and np.array_equal(got0[1], ref0[1])


def test_cli_flag_end_to_end(tmp_path):
    from cglb_amd.backend import jsonio
    run = tmp_path / "itergp"
    cmd = [sys.executable, "-m", "cglb_amd.cli", "-b", "hip", "-t", "fp64", "-l", str(run), "train", "-d", "synthetic-2000-3", "-n", "2", "-o", "adam_0.1",
           "gpr", "-m", "itergp", "-k", "Matern32", "--pred-var-rank", "100"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(run / "results.json") as f:
        results = jsonio.load(f)
    for key in ("loss", "lml", "train/rmse", "train/nlpd", "test/rmse", "test/nlpd"):
        assert key in results and np.isfinite(float(results[key])), key
    res = subprocess.run(cmd[:-6] + ["-m", "gpr", "-k", "Matern32", "--pred-var-rank", "100"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "itergp" in (res.stderr + res.stdout)
