"""The iterative exact-GP class on the HIP backend (cglb_itergp_*, model class `itergp`) against its numpy restatement (tests/itergp_ref.py)
and the dense class (tests/gpr_ref.py).

Exact limit.  With the unit probes eps = sqrt(t) I, t = k + N, run to convergence (max_cg_iter = lanczos_iter = N, max_error = 1e-20), the
estimator is the dense log marginal likelihood and its gradient the exact one.  The restatement itself reaches (tests/test_itergp_ref_host.py,
measured on the CPU; value error of the scale |quad| + |logdet| + N/2 log 2 pi, gradient error of the largest entry):
    (N, D, k) = (40, 3, 6):  rbf 1.2e-15 / 9.8e-14,  matern32 3.0e-16 / 2.9e-14
    (N, D, k) = (67, 2, 9):  rbf 5.6e-16 / 8.7e-16,  matern32 3.2e-15 / 2.5e-13
The tolerance is 100 times that (the library's kernel values are good to 1e-13 where numpy's are to 1e-16) and not below the dense class's own
1e-10 of the scale / 1e-8 of the largest entry; with the numbers above the floor decides in every case.

Same algorithm, random probes.  t = 10, k = 8 and a fixed step count forced by max_error = 0: the GPU and the restatement take the same
number of steps by construction.  The tolerance of each compared quantity is 10 times the largest change of that quantity of the restatement
when every kernel value is perturbed by 1e-13 relative (three seeds of the perturbation; computed by `_random_probe_reference`, printed by
the test).  Measured on the CPU, relative to the largest entry of the quantity: after 5 steps 4e-14 (quad), 5e-13 (correction), 3e-13
(gradient), 1e-12 (rz log); after 20 steps 1e-5 .. 1e-3 (quad), 1e-9 .. 1e-5 (correction), 3e-6 .. 4e-3 (gradient), 3e-4 .. 3e-2 (rz log):
the recurrence is not restarted, so once the leading Ritz values have converged the Lanczos vectors lose their orthogonality and a
perturbation grows by many orders of magnitude while the converged answers do not move."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpr_ref as ref
import itergp_ref as iref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["rbf", "matern32"]
#: measured errors of the restatement in the exact limit (module docstring): (value / scale, gradient / largest entry)
RESTATEMENT_ERRORS = {(40, "rbf"): (1.2e-15, 9.8e-14), (40, "matern32"): (3.0e-16, 2.9e-14), (67, "rbf"): (5.6e-16, 8.7e-16),
                      (67, "matern32"): (3.2e-15, 2.5e-13)}


def _context(X, y, kind, h, k, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)   # Z is a placeholder: the class selects its own
    return ctx


def _zeros(ctx):
    return torch.zeros(ctx.N, dtype=torch.float64, device=ctx.device)


# ---- exact limit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", iref.EXACT_LIMIT_CASES, ids=lambda c: "N%d_D%d_k%d" % c)
def test_unit_probes_give_the_dense_value_and_gradient(case, kind):
    N, D, k = case
    X, y = ref.problem(N, D)
    h = iref.exact_limit_hypers(D)
    want = ref.evaluate(kind, X, y, **h)
    ctx = _context(X, y, kind, h, k)
    try:
        res = ctx.itergp_objective_and_grad(iref.unit_probes(k, N), _zeros(ctx), max_error=1e-20, max_cg_iter=N, lanczos_iter=N)
    finally:
        ctx.close()
    verr, gerr = RESTATEMENT_ERRORS[(N, kind)]
    scale = abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi)
    vtol, gtol = max(100 * verr, 1e-10), max(100 * gerr, 1e-8)
    for name, got, exp in (("lml", res.lml, want.lml), ("quad", res.quad, want.quad), ("logdet", res.logdet, want.logdet)):
        print(f"N={N} {kind}: {name} {got!r} vs {exp!r}: {abs(got - exp) / scale:.2e} of the scale (steps {res.steps})")
        assert abs(got - exp) <= vtol * scale, (name, got, exp)
    g, rg = ref.grad_vector(res.grad), ref.grad_vector(want.grad)
    print(f"N={N} {kind}: gradient {np.abs(g - rg).max() / np.abs(rg).max():.2e} of the largest entry")
    assert np.abs(g - rg).max() <= gtol * np.abs(rg).max(), (g, rg)


# ---- same algorithm, random probes ---------------------------------------------------------------------------------------------------
T, K = 10, 8


def _eps(N):
    return np.random.default_rng(N).standard_normal((T, K + N))


def _quantities(r):
    return {"rz": r.rz_log, "pap": r.pap_log, "correction": np.array([r.correction]), "lml": np.array([r.lml]), "quad": np.array([r.quad]),
            "grad": iref.grad_vector(r.grad)}


@functools.lru_cache(maxsize=None)
def _random_probe_reference(kind, N, D, iters):
    """The restatement, and per quantity 10 times its largest change under a 1e-13 relative perturbation of the kernel values (three seeds)."""
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    args = dict(eps=_eps(N), k=K, max_error=0.0, max_cg_iter=iters, **h)
    base = iref.evaluate(kind, X, y, **args)
    q0 = _quantities(base)
    tol = {name: 0.0 for name in q0}
    for seed in range(3):
        q = _quantities(iref.evaluate(kind, X, y, perturb=1e-13, perturb_seed=seed, **args))
        for name in q0:
            tol[name] = max(tol[name], 10.0 * float(np.abs(q[name] - q0[name]).max()))
    return base, q0, tol


@pytest.mark.parametrize("iters", [5, 20])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(300, 3), (300, 8), (1100, 3), (1100, 8)], ids=lambda s: "N%d_D%d" % s)
def test_random_probes_match_the_restatement(shape, kind, iters):
    N, D = shape
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    base, want, tol = _random_probe_reference(kind, N, D, iters)
    ctx = _context(X, y, kind, h, K)
    try:
        res = ctx.itergp_objective_and_grad(_eps(N), _zeros(ctx), max_error=0.0, max_cg_iter=iters, lanczos_iter=20)
        rz, pap = ctx.itergp_coefficients()
    finally:
        ctx.close()
    assert res.steps == base.steps == iters
    assert abs(res.logdet_P - base.logdet_P) <= 1e-10 * abs(base.logdet_P)
    correction = -2.0 * res.logdet - res.logdet_P
    got = {"rz": rz, "pap": pap, "correction": np.array([correction]), "lml": np.array([res.lml]), "quad": np.array([res.quad]),
           "grad": ref.grad_vector(res.grad)}
    failed = []
    for name in want:
        err = float(np.abs(got[name] - want[name]).max())
        print(f"N={N} D={D} {kind} {iters} steps: {name} differs by {err:.3e}, tolerance {tol[name]:.3e} (largest entry {np.abs(want[name]).max():.3e})")
        if not err <= tol[name]:
            failed.append(name)
    assert not failed, failed


# ---- further checks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_warm_start_repeatability_and_value_only(kind):
    """The warm start serves the data column only and the stop test sums over all columns, so the saving shows where the data column holds the
    loop: the targets are scaled by 30 (its r^T P^-1 r by 900) and two probes are used."""
    N, D, k = 300, 3, 8
    X, y = ref.problem(N, D)
    y = 30.0 * y
    h = ref.hypers(D, True)
    eps = np.random.default_rng(1).standard_normal((2, k + N))
    ctx = _context(X, y, kind, h, k)
    try:
        v = _zeros(ctx)
        cold = ctx.itergp_objective_and_grad(eps, v, max_error=1e-6)
        assert float(v.abs().max()) > 0.0                              # the solution came back in v
        warm = ctx.itergp_objective_and_grad(eps, v, max_error=1e-6)
        print(f"{kind}: cold {cold.steps} steps, warm {warm.steps}")
        assert warm.steps < cold.steps
        assert abs(warm.lml - cold.lml) <= 1e-6 * abs(cold.lml)
        # the same eps and the same start: bitwise equal
        a = ctx.itergp_objective_and_grad(eps, _zeros(ctx), max_error=1e-6)
        b = ctx.itergp_objective_and_grad(eps, _zeros(ctx), max_error=1e-6)
        assert (a.lml, a.quad, a.logdet, a.logdet_P, a.steps) == (b.lml, b.quad, b.logdet, b.logdet_P, b.steps)
        assert np.array_equal(ref.grad_vector(a.grad), ref.grad_vector(b.grad))
        assert (a.lml, a.steps) == (cold.lml, cold.steps)
        value = ctx.itergp_objective_and_grad(eps, _zeros(ctx), max_error=1e-6, with_grad=False)
        assert value.grad is None and value.lml == a.lml
        for name in ("itergp_select_ms", "itergp_solve_ms"):
            assert ctx.get_stat(name) > 0.0
        assert ctx.get_stat("itergp_grad_ms") == 0.0                   # the last evaluation asked for no gradient
    finally:
        ctx.close()


def test_refusals():
    N, D, k = 65, 3, 4
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    eps = np.random.default_rng(0).standard_normal((2, k + N))
    ctx = _context(X, y, "rbf", h, k, dtype=torch.float32)
    try:
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.itergp_objective_and_grad(eps, torch.zeros(N, dtype=torch.float32, device=ctx.device))
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.itergp_predict(X[:3])
    finally:
        ctx.close()
    ctx = _context(X, y, "rbf", h, k)
    try:
        good = ctx.itergp_objective_and_grad(eps, _zeros(ctx))
        ctx.set_targets(np.stack([y, -y], axis=1))
        with pytest.raises(ValueError, match="logdet_bound 0|one target column"):
            ctx.itergp_objective_and_grad(eps, _zeros(ctx))
        ctx.set_targets(y)
        ctx.set_option("logdet_bound", 1)
        with pytest.raises(ValueError, match="logdet_bound 0"):
            ctx.itergp_objective_and_grad(eps, _zeros(ctx))
        with pytest.raises(ValueError, match="logdet_bound 0"):
            ctx.itergp_predict(X[:3])
        ctx.set_option("logdet_bound", 0)
        with pytest.raises(ValueError):
            ctx.itergp_objective_and_grad(eps, torch.zeros(N - 1, dtype=torch.float64, device=ctx.device))   # v_inout of the wrong length
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
        again = ctx.itergp_objective_and_grad(eps, _zeros(ctx))
        assert again.lml == good.lml                                    # the context is still usable
    finally:
        ctx.close()


# ---- predictive ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_predictive_matches_the_dense_one(kind):
    """max_error = 1e-12 bounds 1/2 r^T P^-1 r of every solve (summed over a group of 8).  A Nystrom P = Q_ff + s I satisfies P <= K, hence
    K^-1 <= P^-1 and the error of a solution |x - x*|_K^2 = r^T K^-1 r <= 2e-12.  The mean error is |k_*^T (alpha - alpha*)| <=
    |k_*|_{K^-1} |alpha - alpha*|_K <= sqrt(variance) sqrt(2e-12) (k_*^T K^-1 k_* <= variance: the predictive variance is not negative), and
    the variance error |k_*^T (w - w*)| has the same bound: 1.4e-6 at variance 1.  The kernel values (1e-13 relative) times the condition number
    of K, at most (N variance + noise) / noise = 6e3, add 1e-9."""
    N, D, k, n_new = 300, 3, 8, 19
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    Xnew = np.concatenate([X[:7], np.random.default_rng(5).standard_normal((n_new - 7, D))], axis=0)
    want = ref.evaluate(kind, X, y, with_grad=False, **h)
    rm, rv = ref.predict(kind, X, want, h["lengthscales"], h["variance"], h["mean"], Xnew)
    bound = np.sqrt(h["variance"] * 2e-12) + 1e-9
    ctx = _context(X, y, kind, h, k)
    try:
        mean, var = ctx.itergp_predict(Xnew, max_error=1e-12)           # no evaluation yet: the preconditioner is built first
        ctx.itergp_objective_and_grad(np.random.default_rng(0).standard_normal((2, k + N)), _zeros(ctx), with_grad=False)
        mean2, var2 = ctx.itergp_predict(Xnew, max_error=1e-12)         # ... and this one starts from the alpha of that evaluation
    finally:
        ctx.close()
    for m, v in ((mean, var), (mean2, var2)):
        m, v = m.cpu().numpy(), v.cpu().numpy()
        print(f"{kind}: mean error {np.abs(m - rm).max():.2e}, variance error {np.abs(v - rv).max():.2e}, bound {bound:.2e}")
        assert m.shape == v.shape == (n_new,)
        assert np.abs(m - rm).max() <= bound and np.abs(v - rv).max() <= bound


# ---- through the backend interface -----------------------------------------------------------------------------------------------------
@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


def test_model_class_autograd_probes_save_load(backend, tmp_path):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import IterGPR, PredictIterGPR, PredictLogdensityIterGPR, StochasticLogMarginalLikelihood
    X, y = ref.problem(300, 3)
    cfg = config.IterGPRConfig(config.Matern32Config(), prec_size=8)
    assert (cfg.num_probes, cfg.max_error, cfg.max_cg_iter, cfg.lanczos_iter, cfg.seed) == (10, 1.0, 1000, 20, 0)
    assert config.IterGPRConfig(config.Matern32Config()).prec_size == 100 and config.GPR_CONFIGS["itergp"] is config.IterGPRConfig
    model = backend.create_model(cfg, (X, y))
    assert isinstance(model, IterGPR)
    assert sorted(backend.model_parameters(model)) == [".kernel.lengthscales", ".kernel.variance", ".likelihood.variance", ".mean_function.c"]
    assert model.likelihood.noise_covar._noise.lower_bound == 1e-4
    lml = StochasticLogMarginalLikelihood(model)
    # fresh probes at every call: two values differ; one kept draw: they repeat
    first, second = float(lml((X, y)).detach()), float(lml(None).detach())
    assert first != second and abs(first - second) <= 0.05 * abs(first)
    model.deterministic_probes = True
    model.v_vec.zero_()
    value = lml(None)
    k = model.covar_module
    params = [k.base_kernel._lengthscale.raw, k._outputscale.raw, model.likelihood.noise_covar._noise.raw, model.mean_module.constant]
    assert {id(p) for p in params} == {id(p) for p in model.parameters()}
    grads = torch.autograd.grad(value, params)
    model.v_vec.zero_()
    assert float(lml(None).detach()) == float(value.detach())
    # the library's gradient at the same probes and start, times the chain factors of the softplus transforms
    p = backend.model_parameters(model)
    model.v_vec.zero_()
    model._pushed = None
    model.push_hypers(1e-6)
    res = model.hip.itergp_objective_and_grad(model.probes(), model.v_vec, model.max_error, model.max_cg_iter, model.lanczos_iter)
    assert res.lml == float(value.detach())
    got = np.concatenate([g.detach().numpy().reshape(-1) for g in grads])
    chain = np.concatenate([torch.sigmoid(q.detach()).numpy().reshape(-1) for q in params[:3]] + [np.ones(1)])
    want = ref.grad_vector(res.grad) * chain
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (got, want)
    with pytest.raises(ValueError):
        lml((X[:10], y[:10]))
    with pytest.raises(NotImplementedError):
        PredictIterGPR(model)(torch.as_tensor(X[:5]), full_cov=True)
    f_mean, f_var = PredictIterGPR(model)(torch.as_tensor(X[:5]))
    assert f_mean.shape == (5, 1) and f_var.shape == (5, 1)
    lpd = PredictLogdensityIterGPR(model)((torch.as_tensor(X[:5]), torch.as_tensor(y[:5])))
    assert lpd.shape == (5,) and bool(torch.isfinite(lpd).all())
    # save -> load round-trips into a fresh model
    model.likelihood.noise = 0.3
    backend.save(model, str(tmp_path))
    fresh = backend.load(backend.create_model(cfg, (X, y)), str(tmp_path / "model.json"))
    for key, val in p.items():
        if key != ".likelihood.variance":
            np.testing.assert_allclose(backend.model_parameters(fresh)[key], val, rtol=1e-12, atol=1e-14, err_msg=key)
    np.testing.assert_allclose(backend.model_parameters(fresh)[".likelihood.variance"], 0.3, rtol=1e-12)


def test_exactgp_still_raises_and_scipy_is_refused(backend, tmp_path):
    from cglb_amd.backend import config
    from cglb_amd.backend.callbacks import Logger
    X, y = ref.problem(64, 3)
    with pytest.raises(NotImplementedError, match="exactgp"):
        backend.create_model(config.ExactGPConfig(config.Matern32Config()), (X, y))
    model = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=4), (X, y))
    data = ((X, y), (X[:8], y[:8]))
    logger = Logger(str(tmp_path), backend.metrics_fn(model, data), lambda: backend.model_parameters(model), 1, verbose=False)
    with pytest.raises(ValueError, match="not the derivative"):
        backend.optimize(model, data, 1, logger, "scipy")
    with pytest.raises(ValueError, match="adam_<learning rate>"):
        backend.optimize(model, data, 1, logger, "sgd_0.1")
    # ... and the classes with an exact gradient refuse adam, naming the class that takes it
    exact = backend.create_model(config.GPRConfig(config.Matern32Config()), (X, y))
    with pytest.raises(ValueError, match="itergp"):
        backend.optimize(exact, data, 1, logger, "adam_0.1")


def _adam_on_exact_gradients(kind, X, y, p0, steps, lr):
    """The same Adam loop (torch.optim.Adam on the raw parameters behind softplus) fed with the exact gradients of tests/gpr_ref.py."""
    raw = [torch.tensor(np.log(np.expm1(np.asarray(v, dtype=np.float64))), requires_grad=True) for v in
           (p0[".kernel.lengthscales"], p0[".kernel.variance"], p0[".likelihood.variance"] - 1e-4)]
    mean = torch.tensor(float(p0[".mean_function.c"]), dtype=torch.float64, requires_grad=True)
    adam = torch.optim.Adam(raw + [mean], lr=lr)

    def constrained():
        ls, var, noise = [torch.nn.functional.softplus(r).detach().numpy() for r in raw]
        return ls.reshape(-1), float(var), float(noise) + 1e-4, float(mean.detach())
    for _ in range(steps):
        ls, var, noise, c = constrained()
        g = ref.evaluate(kind, X, y, ls, var, noise, c).grad
        chain = [torch.sigmoid(r.detach()) for r in raw]
        adam.zero_grad()
        raw[0].grad = -torch.as_tensor(g["lengthscales"]).reshape(raw[0].shape) * chain[0]
        raw[1].grad = -torch.as_tensor(g["variance"]).reshape(raw[1].shape) * chain[1]
        raw[2].grad = -torch.as_tensor(g["noise"]).reshape(raw[2].shape) * chain[2]
        mean.grad = -torch.tensor(g["mean"], dtype=torch.float64)
        adam.step()
    return ref.lml_only(kind, X, y, *constrained())


def test_adam_training_gains_half_of_the_exact_gradient_loop(backend, tmp_path):
    from cglb_amd.backend import config
    from cglb_amd.backend.callbacks import Logger
    from cglb_amd.cli import get_dataset
    bundle = get_dataset("synthetic-450-3", 0)          # 301 training points
    data = bundle.to_tuple()
    X, y = bundle.train
    model = backend.create_model(config.IterGPRConfig(config.Matern32Config(), seed=0), bundle.train)
    p0 = backend.model_parameters(model)

    def exact_lml(p):
        return ref.lml_only("matern32", X, y, p[".kernel.lengthscales"], float(p[".kernel.variance"]), float(p[".likelihood.variance"]),
                            float(p[".mean_function.c"]))
    before = exact_lml(p0)
    logger = Logger(str(tmp_path), lambda: {}, lambda: backend.model_parameters(model), 1000, verbose=False)
    losses = backend.optimize(model, data, 30, logger, "adam_0.1")
    assert len(losses) == 30
    after = exact_lml(backend.model_parameters(model))
    exact = _adam_on_exact_gradients("matern32", X, y, p0, 30, 0.1)
    print(f"exact lml: initial {before!r}, after 30 Adam steps on the estimator {after!r}, on exact gradients {exact!r}")
    assert exact > before
    assert after - before >= 0.5 * (exact - before)
    metrics = backend.metrics_fn(model, data)()
    assert sorted(metrics) == ["cg/error", "cg/steps", "lml", "loss", "test/nlpd", "test/rmse", "train/nlpd", "train/rmse"]
    assert all(np.isfinite(float(v)) for v in metrics.values())


# ---- command line --------------------------------------------------------------------------------------------------------------------
def _cli(tmp, *args):
    cmd = [sys.executable, "-m", "cglb_amd.cli", "-b", "hip", "-t", "fp64", "-l", str(tmp), *args]
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_cli_train_and_metric(tmp_path):
    from cglb_amd.backend import jsonio
    run = tmp_path / "itergp"
    res = _cli(run, "train", "-d", "synthetic-300-3", "-n", "3", "-o", "adam_0.1", "gpr", "-m", "itergp", "-k", "Matern32")
    assert res.returncode == 0, res.stdout + res.stderr
    with open(run / "results.json") as f:
        results = jsonio.load(f)
    for key in ("loss", "lml", "train/rmse", "train/nlpd", "test/rmse", "test/nlpd"):
        assert key in results and np.isfinite(float(results[key])), key
    params = jsonio.load(str(run / "model.json"))
    assert sorted(params) == [".kernel.lengthscales", ".kernel.variance", ".likelihood.variance", ".mean_function.c"]
    res = _cli(run, "metric", "-d", "synthetic-300-3", "gpr", "-m", "itergp", "-k", "Matern32", "-p", str(run / "model.json"))
    assert res.returncode == 0, res.stdout + res.stderr
    again = np.load(run / "metric.npy", allow_pickle=True).item()
    for key in ("lml", "train/rmse", "test/nlpd"):
        assert np.isfinite(float(again[key])), key
    # training this class with L-BFGS-B is refused with the reason
    res = _cli(tmp_path / "bad", "train", "-d", "synthetic-300-3", "-n", "1", "gpr", "-m", "itergp", "-k", "Matern32")
    assert res.returncode != 0 and "not the derivative" in (res.stderr + res.stdout)
    res = _cli(tmp_path / "bad", "train", "-d", "synthetic-300-3", "-n", "1", "-o", "adam_0.1", "gpr", "-m", "gpr", "-k", "Matern32")
    assert res.returncode != 0 and "itergp" in (res.stderr + res.stdout)
