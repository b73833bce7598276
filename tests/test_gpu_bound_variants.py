"""SGPR, SGPRN2M, CGLBN2M and CGLBNM2 on the HIP backend: values and gradients of the library against the dense torch restatement
(tests/bound_variants_ref.py), the model classes through `create_model`, the CLI end to end, and the default path left untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bound_variants_ref as ref
from cglb_amd.data import synthetic_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = {"cglb": (0, 0), "cglbnm2": (1, 0), "cglbn2m": (2, 0), "sgpr": (1, 1), "sgprn2m": (2, 1)}
VARIANTS = ("cglbnm2", "cglbn2m", "sgpr", "sgprn2m")
SHAPES = [(300, 16, 1), (2999, 128, 3), (2999, 16, 8), (300, 16, 40)]  # (N, M, D): ragged N, narrow, mid and wide inputs


def _hypers(D, trained):
    if trained:
        return dict(lengthscales=np.full(D, 1.5 if D < 8 else 2.5), variance=1.0, noise=0.05, mean=0.1)
    return dict(lengthscales=np.ones(D), variance=1.0, noise=1.0, mean=0.0)


def _context(X, y, M, kind, cls, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, M, kind, dtype=dtype, device=torch.device("cuda", 0))
    ld, qt = OPTIONS[cls]
    if cls != "cglb":
        ctx.set_option("logdet_bound", ld)
        ctx.set_option("quad_term", qt)
    return ctx


def _evaluate(ctx, h, Z, cls):
    """(bound, gradient, v) of one library evaluation; CG classes: solved first, then evaluated at that v with K v recomputed."""
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
    v = torch.zeros(ctx.N, dtype=ctx.dtype, device=ctx.device)
    if OPTIONS[cls][1] == 0:
        ctx.objective_and_grad(v, run_cg=True, max_error=1.0, with_grad=False)
    res = ctx.objective_and_grad(v, run_cg=False)
    return res, v.double().cpu().numpy()


def _assert_grad_close(g, rg, rel):
    scale = max(max(np.abs(np.asarray(rg[k])).max() for k in rg), 1e-300)
    for k in rg:
        np.testing.assert_allclose(np.asarray(g[k], dtype=np.float64).reshape(np.shape(rg[k])), rg[k], rtol=0, atol=rel * scale, err_msg=k)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_M%d_D%d" % s)
@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("cls", VARIANTS)
def test_value_and_gradient_match_the_restatement(cls, kind, shape):
    N, M, D = shape
    X, y, Z = synthetic_problem(N, D, M, seed=N + D)
    for trained in (False, True):
        h = _hypers(D, trained)
        ctx = _context(X, y, M, kind, cls)
        try:
            res, v = _evaluate(ctx, h, Z, cls)
        finally:
            ctx.close()
        b, g = ref.bound_and_grad(cls, kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Z,
                                  v=None if OPTIONS[cls][1] else v, device="cuda")
        assert abs(res.bound - b) <= 1e-10 * abs(b), (trained, res.bound, b)
        _assert_grad_close(res.grad, g, 1e-8)


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("cls", ["cglbn2m", "sgprn2m"])
def test_n2m_with_many_ragged_tiles(cls, kind):
    """The N^2M pass over 24 x 24 tiles of 128 (the last one 55 wide): diagonal, off-diagonal and ragged tiles all contribute."""
    N, M, D = 2999, 16, 3
    X, y, Z = synthetic_problem(N, D, M, seed=9)
    h = _hypers(D, True)
    ctx = _context(X, y, M, kind, cls)
    try:
        ctx.set_option("n2m_tile", 128)
        res, v = _evaluate(ctx, h, Z, cls)
    finally:
        ctx.close()
    b, g = ref.bound_and_grad(cls, kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Z,
                              v=None if OPTIONS[cls][1] else v, device="cuda")
    assert abs(res.bound - b) <= 1e-10 * abs(b), (res.bound, b)
    _assert_grad_close(res.grad, g, 1e-8)


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("cls", ["cglbnm2", "sgpr"])
def test_nm2_and_exact_quad_at_fp32(cls, kind):
    N, M, D = 1000, 32, 3
    X, y, Z = synthetic_problem(N, D, M, seed=5)
    h = _hypers(D, True)
    ctx = _context(X, y, M, kind, cls, dtype=torch.float32)
    try:
        res, v = _evaluate(ctx, h, Z, cls)
    finally:
        ctx.close()
    b, g = ref.bound_and_grad(cls, kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Z,
                              v=None if OPTIONS[cls][1] else v, device="cuda")
    assert abs(res.bound - b) <= 2e-4 * abs(b), (res.bound, b)
    _assert_grad_close(res.grad, g, 2e-3)


def test_n2m_is_refused_at_fp32():
    X, y, Z = synthetic_problem(200, 2, 8, seed=1)
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, 8, "rbf", dtype=torch.float32, device=torch.device("cuda", 0))
    try:
        with pytest.raises(ValueError, match="fp64"):
            ctx.set_option("logdet_bound", 2)
        ctx.set_option("logdet_bound", 1)      # nm2 and the exact term are available at fp32
        ctx.set_option("quad_term", 1)
    finally:
        ctx.close()


def test_n2m_is_refused_with_the_implicit_preconditioner():
    X, y, Z = synthetic_problem(200, 2, 8, seed=1)
    ctx = _context(X, y, 8, "rbf", "cglb")
    try:
        ctx.set_option("precond_mode", 1)
        with pytest.raises(ValueError, match="precond_mode"):
            ctx.set_option("logdet_bound", 2)
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


def _model_bound(backend, cfg_cls, data):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import CGLB, LowerBoundCG, LowerBoundSGPR
    cfg = cfg_cls(config.Matern32Config(), config.InducingVariableConfig(24))
    model = backend.create_model(cfg, data)
    bound = LowerBoundCG(model) if isinstance(model, CGLB) else LowerBoundSGPR(model)
    with torch.no_grad():
        value = float(bound(None))
    p = backend.model_parameters(model)
    v = model.v_vec.detach().reshape(-1).cpu().numpy() if isinstance(model, CGLB) else None
    return model, value, p, v


def _restated(cls, data, p, v):
    return ref.bound_and_grad(cls, "matern32", data[0], data[1], p[".kernel.lengthscales"], p[".kernel.variance"], p[".likelihood.variance"],
                              p[".mean_function.c"], p[".inducing_variable.Z"], v=v, device="cuda")[0]


def test_cglb_variants_are_not_plain_cglb(backend):
    """Fails before this feature: CGLBN2MConfig / CGLBNM2Config built plain CGLB models."""
    from cglb_amd.backend import config
    X, y, _ = synthetic_problem(800, 3, 1, seed=7)
    data = (X, y)
    _, base, _, _ = _model_bound(backend, config.CGLBConfig, data)
    for cls, cfg in (("cglbn2m", config.CGLBN2MConfig), ("cglbnm2", config.CGLBNM2Config)):
        model, value, p, v = _model_bound(backend, cfg, data)
        assert type(model).__name__ == cls.upper()
        assert abs(value - base) > 1e-6 * abs(base), (cls, value, base)
        assert abs(value - _restated(cls, data, p, v)) <= 1e-10 * abs(value)


def test_sgpr_models_are_created(backend):
    from cglb_amd.backend import config
    X, y, _ = synthetic_problem(800, 3, 1, seed=7)
    data = (X, y)
    for cls, cfg in (("sgpr", config.SGPRConfig), ("sgprn2m", config.SGPRN2MConfig)):
        model, value, p, _ = _model_bound(backend, cfg, data)
        assert not hasattr(model, "v_vec")
        assert abs(value - _restated(cls, data, p, None)) <= 1e-10 * abs(value)


# ---- at size -----------------------------------------------------------------------------------------------------------------------
def test_n2m_at_size_against_dense_torch():
    """N = 30 000, D = 8, M = 512: tau (through the bound) and dT/dl (through the lengthscale gradient) of sgprn2m against dense fp64
    torch on the same GPU (K_ff alone is 7.2 GB); sgpr issues no launch of the symmetric pair kernel."""
    N, M, D = 30000, 512, 8
    X, y, Z = synthetic_problem(N, D, M, seed=3)
    h = _hypers(D, True)
    for cls in ("sgprn2m", "sgpr"):
        ctx = _context(X, y, M, "rbf", cls)
        try:
            ctx.set_option("k1_profile", 1)
            res, _ = _evaluate(ctx, h, Z, cls)
            ctx.set_option("k1_profile", 0)
            assert ctx.get_stat("k1_launches") == 0
        finally:
            ctx.close()
        b, g = ref.bound_and_grad(cls, "rbf", X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, device="cuda")
        torch.cuda.empty_cache()
        assert abs(res.bound - b) <= 1e-10 * abs(b), (cls, res.bound, b)
        _assert_grad_close(res.grad, g, 1e-8)


# ---- the default path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rbf", "matern32"])
def test_default_options_are_bitwise_the_old_path(kind):
    N, M, D = 1500, 64, 3
    X, y, Z = synthetic_problem(N, D, M, seed=2)
    h = _hypers(D, True)
    out = []
    for set_options in (False, True):
        ctx = _context(X, y, M, kind, "cglb")
        try:
            if set_options:
                ctx.set_option("logdet_bound", 2)
                ctx.set_option("quad_term", 1)
                ctx.set_option("logdet_bound", 0)
                ctx.set_option("quad_term", 0)
            ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
            v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
            res = ctx.objective_and_grad(v, run_cg=True, max_error=1.0)
            out.append((res, v.cpu().numpy(), ctx.logdet()))
        finally:
            ctx.close()
    (a, va, la), (b, vb, lb) = out
    assert (a.bound, a.lower, a.upper, a.logdet, a.steps, la) == (b.bound, b.lower, b.upper, b.logdet, b.steps, lb)
    assert np.array_equal(va, vb)
    for k in a.grad:
        assert np.array_equal(np.asarray(a.grad[k]), np.asarray(b.grad[k])), k


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _cli(tmp, *args):
    cmd = [sys.executable, "-m", "cglb_amd.cli", "-b", "hip", "-t", "fp64", "-l", str(tmp), *args]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    return res


def test_cli_end_to_end(tmp_path):
    from cglb_amd.backend import jsonio
    from cglb_amd.cli import get_dataset
    train = get_dataset("synthetic-2000-3", 0).train
    sg = tmp_path / "sgpr"
    _cli(sg, "train", "-d", "synthetic-2000-3", "-n", "8", "sgpr", "-k", "Matern32", "-m", "sgpr", "-i", "cv", "-M", "64")
    with open(sg / "results.json") as f:
        results = jsonio.load(f)
    for key in ("loss", "elbo", "train/rmse", "train/nlpd", "test/rmse", "test/nlpd", "id"):
        assert key in results, key
    params = jsonio.load(str(sg / "model.json"))
    b = _restated("sgpr", train, {k: np.asarray(v) for k, v in params.items()}, None)
    assert abs(results["loss"] + b) <= 1e-10 * abs(b)
    _cli(sg, "metric", "-d", "synthetic-2000-3", "sgpr", "-k", "Matern32", "-m", "sgpr", "-i", "cv", "-M", "64", "-p", str(sg / "model.json"))
    again = np.load(sg / "metric.npy", allow_pickle=True).item()
    assert abs(again["loss"] - results["loss"]) <= 1e-10 * abs(results["loss"])

    cg = tmp_path / "cglbn2m"
    _cli(cg, "train", "-d", "synthetic-2000-3", "-n", "8", "cglb", "-k", "Matern32", "-m", "cglbn2m", "-i", "cv", "-M", "64")
    with open(cg / "results.json") as f:
        results = jsonio.load(f)
    for key in ("loss", "train/rmse", "train/nlpd", "test/rmse", "test/nlpd", "cg/steps", "cg/error", "id"):
        assert key in results, key
    assert np.isfinite(results["loss"])
    assert (cg / "model.json").exists()
