"""The exact GPR class on the HIP backend: the library's log marginal likelihood, its gradient and its predictive against the dense numpy
restatement (tests/gpr_ref.py), reproducibility, a changed block edge, the order bound <= lml, the refusals, the model class through
`create_model`, and the command line end to end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpr_ref as ref
from cglb_amd.data import synthetic_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["rbf", "matern32"]
SHAPE_IDS = ["N%d_D%d" % s[:2] for s in ref.SHAPES]


def _context(X, y, kind, block=None, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, 1, kind, dtype=dtype, device=torch.device("cuda", 0))   # M = 1: the class has no inducing points
    if block is not None:
        ctx.set_option("gpr_block", block)
    return ctx


@functools.lru_cache(maxsize=None)
def _reference(kind, N, D, trained):
    """One dense evaluation per (kernel, shape, hyper-parameter set), shared by every test that needs it and never modified."""
    X, y = ref.problem(N, D)
    return ref.evaluate(kind, X, y, **ref.hypers(D, trained))


def _assert_matches(res, want, N, what):
    scale = abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi)
    for name in ("lml", "quad", "logdet"):
        got, exp = getattr(res, name), getattr(want, name)
        print(f"{what}: {name} {got!r} vs {exp!r}: {abs(got - exp) / scale:.2e} of the scale")
        assert abs(got - exp) <= 1e-10 * scale, (what, name, got, exp)
    g, rg = ref.grad_vector(res.grad), ref.grad_vector(want.grad)
    err = np.abs(g - rg).max() / max(np.abs(rg).max(), 1e-300)
    print(f"{what}: gradient {err:.2e} of the largest entry")
    assert np.abs(g - rg).max() <= 1e-8 * np.abs(rg).max(), (what, g, rg)


@pytest.mark.parametrize("trained", [False, True], ids=["init", "trained"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_value_and_gradient_match_the_restatement(shape, kind, trained):
    N, D, block = shape
    X, y = ref.problem(N, D)
    h = ref.hypers(D, trained)
    want = _reference(kind, N, D, trained)
    ctx = _context(X, y, kind, block)
    try:
        ctx.gpr_set_hypers(**h)
        first = ctx.gpr_objective_and_grad()
        _assert_matches(first, want, N, "first evaluation")
        assert ctx.get_stat("gpr_bytes") >= 16 * N * N
        # the same inputs again: bitwise the same numbers
        again = ctx.gpr_objective_and_grad()
        assert (first.lml, first.quad, first.logdet) == (again.lml, again.quad, again.logdet)
        assert np.array_equal(ref.grad_vector(first.grad), ref.grad_vector(again.grad))
        # value only: the same value without forming the inverse
        value = ctx.gpr_objective_and_grad(with_grad=False)
        assert value.grad is None and (value.lml, value.quad, value.logdet) == (first.lml, first.quad, first.logdet)
        # another block edge on the same context: the pool is released and rebuilt
        ctx.set_option("gpr_block", 128 if (block or 2048) != 128 else 64)
        assert ctx.get_stat("gpr_bytes") == 0
        _assert_matches(ctx.gpr_objective_and_grad(), want, N, "after a changed gpr_block")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[0] in (300, 1500)], ids=lambda s: "N%d_D%d" % s[:2])
def test_predictive_matches_the_restatement(shape, kind):
    N, D, block = shape
    X, y = ref.problem(N, D)
    Xnew = np.concatenate([X[:128], np.random.default_rng(5).standard_normal((129, D))], axis=0)   # 257 points, half of them training rows
    for trained in (False, True):
        h = ref.hypers(D, trained)
        want = _reference(kind, N, D, trained)
        rm, rv = ref.predict(kind, X, want, h["lengthscales"], h["variance"], h["mean"], Xnew)
        ctx = _context(X, y, kind, block)
        try:
            ctx.gpr_set_hypers(**h)
            mean, var = ctx.gpr_predict(Xnew)             # no evaluation yet: predict factors first
            res = ctx.gpr_objective_and_grad(with_grad=False)
            mean2, var2 = ctx.gpr_predict(Xnew)           # ... and this one uses the factor of that evaluation
        finally:
            ctx.close()
        assert abs(res.lml - want.lml) <= 1e-10 * (abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi))
        for m, v in ((mean, var), (mean2, var2)):
            m, v = m.cpu().numpy(), v.cpu().numpy()
            print(f"N={N} {kind} trained={trained}: mean {np.abs(m - rm).max() / np.abs(rm).max():.2e}, variance {np.abs(v - rv).max() / np.abs(rv).max():.2e}")
            assert np.abs(m - rm).max() <= 1e-8 * np.abs(rm).max()
            assert np.abs(v - rv).max() <= 1e-8 * np.abs(rv).max()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[0] in (300, 1500)], ids=lambda s: "N%d_D%d" % s[:2])
def test_cglb_bound_is_below_the_lml(shape, kind):
    from cglb_amd.hip_context import HipContext
    N, D, block = shape
    X, y, Z = synthetic_problem(N, D, 16, seed=N + D)
    for trained in (False, True):
        h = ref.hypers(D, trained)
        sparse = HipContext(X, y, 16, kind, device=torch.device("cuda", 0))
        exact = _context(X, y, kind, block)
        try:
            sparse.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
            v = torch.zeros(N, dtype=torch.float64, device=sparse.device)
            bound = sparse.objective_and_grad(v, run_cg=True, max_error=1.0, with_grad=False).bound
            exact.gpr_set_hypers(**h)
            lml = exact.gpr_objective_and_grad(with_grad=False).lml
        finally:
            sparse.close()
            exact.close()
        print(f"N={N} {kind} trained={trained}: bound {bound!r} lml {lml!r}")
        assert bound <= lml + 1e-9 * N, (bound, lml)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_fp32_context_is_refused():
    X, y = ref.problem(65, 3)
    ctx = _context(X, y, "rbf", dtype=torch.float32)
    try:
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.gpr_set_hypers(**ref.hypers(3, False))
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.gpr_objective_and_grad()
        # the context itself is still usable: the sparse classes run at fp32
        Z = X[:1].copy()
        ctx.set_hypers(np.ones(3), 1.0, 1.0, 0.0, Z, 1e-6)
        ctx.setup()
    finally:
        ctx.close()


def test_refusals_leave_the_context_usable():
    N, D = 65, 3
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    want = _reference("matern32", N, D, True)
    ctx = _context(X, y, "matern32", 64)
    try:
        ctx.gpr_set_hypers(**h)
        # two target columns
        ctx.set_targets(np.stack([y, -y], axis=1))
        with pytest.raises(ValueError, match="one target column"):
            ctx.gpr_objective_and_grad()
        with pytest.raises(ValueError, match="one target column"):
            ctx.gpr_predict(X[:3])
        ctx.set_targets(y)
        _assert_matches(ctx.gpr_objective_and_grad(), want, N, "after two target columns")
        # a block edge that is no multiple of 64
        for bad in (100, 0, 32, 8192):
            with pytest.raises(ValueError, match="multiple of 64"):
                ctx.set_option("gpr_block", bad)
        _assert_matches(ctx.gpr_objective_and_grad(), want, N, "after a refused gpr_block")
        # a matrix that is not positive definite: variance 1 on the diagonal, noise -1
        ctx.gpr_set_hypers(np.ones(D), 1.0, -1.0, 0.0)
        with pytest.raises(RuntimeError, match="not positive definite.*pivot at row 0 ") as info:
            ctx.gpr_objective_and_grad()
        assert "error" not in str(info.value)      # CGLB_ERR_NOT_PD, not a HIP or BLAS error (cglb_amd/_lib.py: check)
        with pytest.raises(RuntimeError, match="not positive definite"):
            ctx.gpr_predict(X[:3])
        ctx.gpr_set_hypers(**h)
        _assert_matches(ctx.gpr_objective_and_grad(), want, N, "after a non-positive pivot")
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pivot_index_is_global(kind):
    """Points 0 .. 99 are far apart (K = I there), point 100 repeats point 0: with noise -0.5 the pivots are 0.5 up to row 100, where
    0.5 - 1 / 0.5 < 0.  With blocks of 64 that is local row 36 of the second block."""
    N = 130
    X = 100.0 * np.arange(N, dtype=np.float64).reshape(-1, 1)
    X[100] = X[0]
    ctx = _context(X, np.zeros(N), kind, 64)
    try:
        ctx.gpr_set_hypers(np.ones(1), 1.0, -0.5, 0.0)
        with pytest.raises(RuntimeError, match="pivot at row 100 "):
            ctx.gpr_objective_and_grad(with_grad=False)
    finally:
        ctx.close()


# ---- through the backend interface -------------------------------------------------------------------------------------------------
@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


def _restated(data, p, kind="matern32"):
    return ref.evaluate(kind, data[0], data[1], p[".kernel.lengthscales"], float(p[".kernel.variance"]), float(p[".likelihood.variance"]),
                        float(p[".mean_function.c"]))


def test_model_objective_and_autograd(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import ExactGPR, LogMarginalLikelihood, PredictGPR, PredictLogdensityGPR
    X, y = ref.problem(300, 3)
    model = backend.create_model(config.GPRConfig(config.Matern32Config()), (X, y))
    assert isinstance(model, ExactGPR)
    assert sorted(backend.model_parameters(model)) == [".kernel.lengthscales", ".kernel.variance", ".likelihood.variance", ".mean_function.c"]
    lml = LogMarginalLikelihood(model)
    value = lml((X, y))
    # the four parameter tensors: three behind softplus (d value / d raw = sigmoid(raw)) and the constant mean
    k = model.covar_module
    params = [k.base_kernel._lengthscale.raw, k._outputscale.raw, model.likelihood.noise_covar._noise.raw, model.mean_module.constant]
    assert {id(p) for p in params} == {id(p) for p in model.parameters()}
    grads = torch.autograd.grad(value, params)
    want = _restated((X, y), backend.model_parameters(model))
    N = 300
    assert abs(float(value.detach()) - want.lml) <= 1e-10 * (abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi))
    got = np.concatenate([g.detach().numpy().reshape(-1) for g in grads])
    chain = np.concatenate([torch.sigmoid(p.detach()).numpy().reshape(-1) for p in params[:3]] + [np.ones(1)])
    rg = ref.grad_vector(want.grad) * chain
    assert np.abs(got - rg).max() <= 1e-8 * np.abs(rg).max(), (got, rg)
    with pytest.raises(ValueError):
        lml((X[:10], y[:10]))
    with pytest.raises(NotImplementedError):
        PredictGPR(model)(torch.as_tensor(X[:5]), full_cov=True)
    f_mean, f_var = PredictGPR(model)(torch.as_tensor(X[:5]))
    assert f_mean.shape == (5, 1) and f_var.shape == (5, 1)
    lpd = PredictLogdensityGPR(model)((torch.as_tensor(X[:5]), torch.as_tensor(y[:5])))
    assert lpd.shape == (5,) and bool(torch.isfinite(lpd).all())


def test_exactgp_is_not_implemented(backend):
    from cglb_amd.backend import config
    X, y = ref.problem(64, 3)
    with pytest.raises(NotImplementedError, match="exactgp"):
        backend.create_model(config.ExactGPConfig(config.Matern32Config()), (X, y))


def test_fp32_model_names_the_float_type_option(backend):
    from cglb_amd.backend import config
    X, y = ref.problem(64, 3)
    backend.set_default_float("fp32")
    try:
        with pytest.raises(ValueError, match="-t fp64"):
            backend.create_model(config.GPRConfig(config.Matern32Config()), (X, y))
    finally:
        backend.set_default_float("fp64")


def test_optimize_metrics_save_load(backend, tmp_path):
    from cglb_amd.backend import config
    from cglb_amd.backend.callbacks import Logger
    from cglb_amd.cli import get_dataset
    bundle = get_dataset("synthetic-450-3", 0)          # 301 training points
    data = bundle.to_tuple()
    cfg = config.GPRConfig(config.Matern32Config())
    model = backend.create_model(cfg, bundle.train)
    metrics_fn = backend.metrics_fn(model, data)
    before = metrics_fn()
    assert sorted(before) == ["lml", "loss", "test/nlpd", "test/rmse", "train/nlpd", "train/rmse"]
    assert before["loss"] == -before["lml"]
    logger = Logger(str(tmp_path), metrics_fn, lambda: backend.model_parameters(model), 1, verbose=False)
    results = backend.optimize(model, data, 5, logger, "scipy")
    assert sum(r.nit for r in results) <= 5
    losses = logger.logs["loss"]                        # one entry per accepted step
    assert len(losses) >= 2 and all(b < a for a, b in zip(losses, losses[1:])), losses
    after = metrics_fn()
    assert after["loss"] < before["loss"]
    want = _restated(bundle.train, backend.model_parameters(model))
    assert abs(after["lml"] - want.lml) <= 1e-10 * (abs(want.quad) + abs(want.logdet) + 0.5 * 301 * np.log(2.0 * np.pi))
    # save -> load round-trips into a fresh model
    backend.save(model, str(tmp_path))
    fresh = backend.load(backend.create_model(cfg, bundle.train), str(tmp_path / "model.json"))
    saved, loaded = backend.model_parameters(model), backend.model_parameters(fresh)
    for key, value in saved.items():
        np.testing.assert_allclose(loaded[key], value, rtol=1e-12, atol=1e-14, err_msg=key)
    assert abs(backend.metrics_fn(fresh, data)()["lml"] - after["lml"]) <= 1e-10 * abs(after["lml"])


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _cli(tmp, *args, float_type="fp64"):
    cmd = [sys.executable, "-m", "cglb_amd.cli", "-b", "hip", "-t", float_type, "-l", str(tmp), *args]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_cli_train_and_metric(tmp_path):
    from cglb_amd.backend import jsonio
    from cglb_amd.cli import get_dataset
    run = tmp_path / "gpr"
    res = _cli(run, "train", "-d", "synthetic-300-3", "-n", "5", "gpr", "-m", "gpr", "-k", "Matern32")
    assert res.returncode == 0, res.stdout + res.stderr
    with open(run / "results.json") as f:
        results = jsonio.load(f)
    for key in ("loss", "lml", "train/rmse", "train/nlpd", "test/rmse", "test/nlpd", "id"):
        assert key in results, key
    params = {k: np.asarray(v) for k, v in jsonio.load(str(run / "model.json")).items()}
    assert ".inducing_variable.Z" not in params
    want = _restated(get_dataset("synthetic-300-3", 0).train, params)
    assert abs(results["lml"] - want.lml) <= 1e-10 * (abs(want.quad) + abs(want.logdet) + 0.5 * 201 * np.log(2.0 * np.pi))
    res = _cli(run, "metric", "-d", "synthetic-300-3", "gpr", "-m", "gpr", "-k", "Matern32", "-p", str(run / "model.json"))
    assert res.returncode == 0, res.stdout + res.stderr
    again = np.load(run / "metric.npy", allow_pickle=True).item()
    assert abs(again["lml"] - results["lml"]) <= 1e-10 * abs(results["lml"])


def test_cli_gpr_metric_of_a_cglb_run(tmp_path):
    from cglb_amd.backend import jsonio
    run = tmp_path / "cglb"
    res = _cli(run, "train", "-d", "synthetic-300-3", "-n", "5", "cglb", "-m", "cglb", "-k", "Matern32", "-i", "cv", "-M", "16")
    assert res.returncode == 0, res.stdout + res.stderr
    with open(run / "results.json") as f:
        bound = -jsonio.load(f)["loss"]                  # the run's final cg lower bound
    res = _cli(tmp_path / "exact", "gpr_metric", "-d", "synthetic-300-3", "-k", "Matern32", "-p", str(run / "model.json"))
    assert res.returncode == 0, res.stdout + res.stderr
    exact = np.load(run / "gpr_metric.npy", allow_pickle=True).item()      # next to the parameter file
    assert sorted(k for k in exact if k != "id") == ["lml", "loss", "test/nlpd", "test/rmse", "train/nlpd", "train/rmse"]
    assert json.loads(res.stdout.strip().splitlines()[-1])["lml"] == exact["lml"]
    print(f"cglb bound {bound!r}, exact lml {exact['lml']!r}")
    assert exact["lml"] >= bound - 1e-9 * 201, (exact["lml"], bound)


def test_cli_fp32_is_refused_with_the_option_to_use(tmp_path):
    res = _cli(tmp_path, "train", "-d", "synthetic-300-3", "-n", "1", "gpr", "-m", "gpr", "-k", "Matern32", float_type="fp32")
    assert res.returncode != 0 and "-t fp64" in res.stderr, res.stdout + res.stderr
