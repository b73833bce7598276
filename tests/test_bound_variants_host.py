"""The five bounds of SGPR_CONFIGS in their dense restatement (tests/bound_variants_ref.py), on the CPU: the order of the log-det
bounds, the SGPR ELBO below the exact marginal likelihood, the restatement against the numpy oracle, and the command line."""
import numpy as np
import pytest
import torch
from click.testing import CliRunner

import bound_variants_ref as ref
from oracle import cglb_oracle as orc

F64 = dict(dtype=torch.float64)
CASES = [(kind, hyp, D) for kind in ("rbf", "matern32") for hyp in ("init", "trained") for D in (1, 3)]


def _problem(kind, hyp, D, N=400, M=24):
    X, y, Z = orc.synthetic_problem(N, D, M, seed=D + (hyp == "trained"))
    h = orc.reference_init_hypers(D, Z) if hyp == "init" else orc.trained_like_hypers(D, Z)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return kind, t(X), t(y), t(h.lengthscales), t(h.variance), t(h.noise), t(h.mean), t(Z), h


@pytest.mark.parametrize("kind,hyp,D", CASES)
def test_logdet_bounds_are_ordered(kind, hyp, D):
    kind, X, y, ls, var, noise, mean, Z, _ = _problem(kind, hyp, D)
    A, AAt, LB = ref.common_terms(kind, X, ls, var, noise, Z, 1e-6)
    upper = {w: -float(ref.logdet_term(w, kind, X, ls, var, noise, A, AAt, LB)) for w in ("jensen", "nm2", "n2m")}
    exact = float(ref.exact_half_logdet(kind, X, ls, var, noise))
    tol = 1e-10 * abs(exact)
    assert exact <= upper["n2m"] + tol
    assert upper["n2m"] <= upper["jensen"] + tol
    assert upper["jensen"] <= upper["nm2"] + tol


@pytest.mark.parametrize("kind,hyp,D", CASES)
def test_sgpr_elbo_is_below_the_marginal_likelihood(kind, hyp, D):
    kind, X, y, ls, var, noise, mean, Z, _ = _problem(kind, hyp, D)
    elbo = float(ref.bound("sgpr", kind, X, y, ls, var, noise, mean, Z))
    assert elbo <= float(ref.exact_log_marginal(kind, X, y, ls, var, noise, mean))
    assert float(ref.bound("sgprn2m", kind, X, y, ls, var, noise, mean, Z)) >= elbo


@pytest.mark.parametrize("kind,hyp,D", CASES)
def test_n2m_bound_is_above_cglb_at_the_same_v(kind, hyp, D):
    kind, X, y, ls, var, noise, mean, Z, h = _problem(kind, hyp, D)
    v = torch.as_tensor(orc.objective(kind, X.numpy(), y.numpy(), h, np.zeros(X.shape[0])).v)
    assert float(ref.bound("cglbn2m", kind, X, y, ls, var, noise, mean, Z, v=v)) >= float(ref.bound("cglb", kind, X, y, ls, var, noise, mean, Z, v=v))


@pytest.mark.parametrize("kind,hyp,D", CASES)
def test_sgpr_is_cglb_at_v_zero_with_the_trace_term_swapped(kind, hyp, D):
    kind, X, y, ls, var, noise, mean, Z, _ = _problem(kind, hyp, D)
    zero = torch.zeros(X.shape[0], **F64)
    for sg, cg in (("sgpr", "cglbnm2"), ("sgprn2m", "cglbn2m")):
        a = float(ref.bound(sg, kind, X, y, ls, var, noise, mean, Z))
        b = float(ref.bound(cg, kind, X, y, ls, var, noise, mean, Z, v=zero))
        assert abs(a - b) <= 1e-12 * abs(a)


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
def test_cglb_restatement_is_the_oracle(kind):
    """The torch restatement of the cglb class against the numpy oracle: value and gradient at a CG solution."""
    X, y, Z = orc.synthetic_problem(300, 3, 16, seed=4)
    h = orc.trained_like_hypers(3, Z)
    o = orc.objective(kind, X, y, h, np.zeros(300))
    g = orc.objective(kind, X, y, h, o.v, run_cg=False, with_grad=True).grad
    b, rg = ref.bound_and_grad("cglb", kind, X, y, h.lengthscales, h.variance, h.noise, h.mean, Z, v=o.v)
    assert abs(b - o.bound) <= 1e-12 * abs(o.bound)
    for k in rg:
        np.testing.assert_allclose(rg[k], np.asarray(g[k]), rtol=1e-9, atol=1e-10 * np.abs(np.asarray(g[k])).max())
    np.testing.assert_allclose(ref.kernel_matrix(kind, torch.as_tensor(X), torch.as_tensor(Z), torch.as_tensor(h.lengthscales), 1.0).numpy(),
                               orc.kernel_matrix(kind, X, Z, h.lengthscales, 1.0), rtol=0, atol=1e-15)


@pytest.fixture
def cli(monkeypatch, tmp_path):
    from cglb_amd import cli as cli_mod
    from cglb_amd.backend import interface
    monkeypatch.setattr(interface, "configure_backend", lambda **kw: None)  # no HIP device here: nothing below reaches the GPU
    return lambda *args: CliRunner().invoke(cli_mod.main, ["-l", str(tmp_path), *args])


@pytest.mark.parametrize("cls", ["sgpr", "sgprn2m"])
def test_cli_cglb_command_points_sgpr_classes_to_the_sgpr_command(cli, cls):
    res = cli("train", "-d", "synthetic-60-2", "cglb", "-k", "Matern32", "-m", cls, "-i", "cv", "-M", "8")
    assert res.exit_code == 2, res.output
    assert "Usage" in res.output and "sgpr" in res.output and "TypeError" not in res.output


@pytest.mark.parametrize("group", ["train", "metric"])
def test_cli_sgpr_command_options(cli, group):
    res = cli(group, "-d", "synthetic-60-2", "sgpr", "--help")
    assert res.exit_code == 0, res.output
    for opt in ("-m, --model-class", "-k, --kernel", "-i, --inducing-variable", "-M, --num-inducing-variables", "-p, --param_file"):
        assert opt in res.output, opt
    assert "sgprn2m" in res.output and "--vjoint" not in res.output


def test_multi_rank_request_is_refused_before_the_gpu(monkeypatch):
    """Under a process group of more than one rank the four new classes raise NotImplementedError at model creation, before the
    inducing-point selection or any other GPU work (only the world size is read)."""
    import torch.distributed as dist
    from cglb_amd.backend import config, interface
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    X, y, _ = orc.synthetic_problem(50, 2, 4, seed=0)
    for cfg in (config.SGPRConfig, config.SGPRN2MConfig, config.CGLBN2MConfig, config.CGLBNM2Config):
        c = cfg(config.Matern32Config(), config.InducingVariableConfig(4))
        with pytest.raises(NotImplementedError, match="more than one rank"):
            interface.create_model(c, (X, y))
