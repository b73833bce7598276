"""Gradients with respect to the TRAINING inputs on the HIP backend (csrc/kernels_train_input_grad.hip; cglb_grad_x_kff_multi,
cglb_itergp_objective_and_grad_x, cglb_gpr_objective_and_grad_x, cglb_set_inputs; InputGrad*LogMarginalLikelihood) against the np.longdouble
restatement tests/train_input_grad_ref.py.

The product, every element: 1e-11 of the per-element sum of absolute terms f sum_j |w_ij| h_ij |delta_ijk| / l_k - the figure
tests/test_gpu_input_grad.py and tests/test_gpu_grad_multi.py hold the same pair evaluator (direct differences, kappa_hfac_hot_from_d2) to - plus
that file's floor of the range-clamped 2^x where the sum underflows.  Cells: train_input_grad_ref.covering_table (every (R, G) class at one row past
its row block, S in 1, G, G + 1, 9, 11, forced splits 1, 3, 7, one row past a launch block), each with a duplicated row and a row at 10^3.
A second call is bitwise equal.  S equal pairs give S times one pair and a permutation of the pairs agrees within the bound derived in
tests/test_gpu_grad_multi.py: the pair weights differ by at most S roundings and every partial sum is a chain of at most N additions, so
(N + S) 2^-53 of the sum of absolute terms, doubled for the two sides compared.

Identities against grad_kff_multi on the same U, V: scaling sum_i x_ik gx[i, k] = -l_k G_l[k] within 2e-11 of the sum of absolute terms (each
pass is held to 1e-11 of that scale); translation sum_i gx[i, k] = 0 within 2 (N + S) 2^-53 of it.

itergp: out4 / grad bitwise those of the entry without gx_out; the scaling identity between grad_x and grad["lengthscales"] of one evaluation;
the exact limit of tests/test_gpu_itergp.py (unit probes, run to convergence) against the dense gradient by that test's rule, max(100 times the
restatement's distance, 1e-8 of the largest entry) - the restatement is the dense formula itself (np.longdouble on a float64 inverse, 1e-13), so
the floor 1e-8 decides.  gpr: out3 / grad bitwise, grad_x against the restatement to the dense class's 1e-8 of the largest entry.
End to end: x = raw @ A through InputGradLogMarginalLikelihood against torch autograd on the CPU lml, 1e-8 of the largest entry."""
import functools

import numpy as np
import pytest
import torch

import gpr_ref as ref
import itergp_ref as iref
import train_input_grad_ref as tr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def _context(X, y, kind, h, k=1, dtype=torch.float64, jsplit=0):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=dtype, device=torch.device("cuda", 0))
    if jsplit:
        ctx.set_option("kff_jsplit", jsplit)
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
    return ctx


def _pairs(N, S, seed=0):
    rng = np.random.default_rng(1000 + seed + N + S)
    return rng.standard_normal((N, S)), rng.standard_normal((N, S))


def _inputs(N, D):
    """the problem of the shape with one duplicated row and one row at 10^3 (value and gradient underflow there), where there are rows for them"""
    X, y = ref.problem(N, D)
    X = X.copy()
    if N >= 4:
        X[1] = X[0]
        X[2] = 1.0e3
    return X, y


@functools.lru_cache(maxsize=None)
def _reference(kind, N, D, S, trained):
    """One np.longdouble evaluation per cell, shared and never modified: (gx, tolerance) as float64"""
    X, _ = _inputs(N, D)
    h = ref.hypers(D, trained)
    U, V = _pairs(N, S)
    gx, scale = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U, V)
    wsum = np.concatenate([np.abs(tr.pair_weights(U, V, rows=slice(i, i + 512))).sum(axis=1) for i in range(0, N, 512)])
    out = gx.astype(np.float64), tr.tolerance(scale, wsum, h["variance"]), scale.astype(np.float64)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the product, every element -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", tr.covering_table(), ids=lambda c: "N%d_D%d_S%d_js%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], "trained" if c[5] else "init"))
def test_every_element_matches_the_restatement(cell):
    N, D, S, jsplit, kind, trained = cell
    X, y = _inputs(N, D)
    want, tol, scale = _reference(kind, N, D, S, trained)
    U, V = _pairs(N, S)
    ctx = _context(X, y, kind, ref.hypers(D, trained), jsplit=jsplit)
    try:
        assert ctx.get_stat("train_input_grad_native") == 1.0
        got = ctx.grad_x_kff_multi(U, V).cpu().numpy()
        again = ctx.grad_x_kff_multi(U, V).cpu().numpy()
    finally:
        ctx.close()
    assert got.shape == (N, D) and np.all(np.isfinite(got))     # the buffer starts as NaN: every element was written
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print(f"{cell}: largest error {err[scale > 0].max() if (scale > 0).any() else 0.0:.2e} of the sum of absolute terms")
    assert np.all(np.abs(got - want) <= tol), (np.abs(got - want).max(), err.max())
    assert np.array_equal(got, again)                            # two calls: bitwise equal
    if N >= 4:
        assert np.all(np.abs(got[2]) <= tol[2])                  # the row at 10^3: everything underflows


def test_the_table_reaches_every_class():
    seen = {(tr.rows_per_lane(c[1]), tr.group_width(c[1])) for c in tr.covering_table()}
    assert seen == {(tr.rows_per_lane(d), tr.group_width(d)) for d in range(1, 33)}


@pytest.mark.parametrize("kind", tr.KINDS)
def test_equal_pairs_and_permutations(kind):
    N, D = 1100, 8
    X, y = ref.problem(N, D)
    h = dict(ref.hypers(D, True), variance=1.7)
    U, V = _pairs(N, 11, seed=5)
    ctx = _context(X, y, kind, h)
    try:
        full = ctx.grad_x_kff_multi(U, V).cpu().numpy()
        perm = np.random.default_rng(2).permutation(11)
        permuted = ctx.grad_x_kff_multi(U[:, perm], V[:, perm]).cpu().numpy()
        one = ctx.grad_x_kff_multi(U[:, :1], V[:, :1]).cpu().numpy()
        scale1 = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U[:, :1], V[:, :1])[1].astype(np.float64)
        for S in (2, 8, 9, 11):
            many = ctx.grad_x_kff_multi(np.repeat(U[:, :1], S, axis=1), np.repeat(V[:, :1], S, axis=1)).cpu().numpy()
            print(f"{kind} S={S}: {(np.abs(many - S * one) / (S * scale1)).max():.2e} against {2 * (N + S) * EPS:.2e}")
            assert np.all(np.abs(many - S * one) <= 2 * (N + S) * EPS * S * scale1)
    finally:
        ctx.close()
    want, scale = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U, V)
    assert np.all(np.abs(full - want.astype(np.float64)) <= tr.TOL * scale.astype(np.float64))
    assert np.all(np.abs(permuted - full) <= 2 * (N + 11) * EPS * scale.astype(np.float64))


# ---- the identities on the GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("shape", [(257, 3, 1), (513, 8, 9), (300, 20, 11)], ids=lambda s: "N%d_D%d_S%d" % s)
def test_scaling_and_translation_against_grad_kff_multi(shape, kind):
    N, D, S = shape
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    U, V = _pairs(N, S)
    ctx = _context(X, y, kind, h)
    try:
        gx = ctx.grad_x_kff_multi(U, V).cpu().numpy()
        Gl = ctx.grad_kff_multi(U, V)[:D]
    finally:
        ctx.close()
    scale = tr.grad_x(kind, X, h["lengthscales"], h["variance"], U, V)[1].astype(np.float64)
    ls = np.asarray(h["lengthscales"], dtype=np.float64)
    lhs = (X * gx).sum(axis=0)
    bound = (np.abs(X) * scale).sum(axis=0)          # sum of the absolute terms of sum_i x_ik gx[i, k]
    print(f"{kind} {shape}: scaling {np.abs(lhs + ls * Gl).max():.2e} of {bound.max():.2e}; translation {np.abs(gx.sum(axis=0)).max():.2e} of {scale.sum(axis=0).max():.2e}")
    assert np.all(np.abs(lhs + ls * Gl) <= 2e-11 * bound)
    assert np.all(np.abs(gx.sum(axis=0)) <= 2 * (N + S) * EPS * scale.sum(axis=0))


# ---- itergp ----------------------------------------------------------------------------------------------------------------------------------------
def _zeros(ctx):
    return torch.zeros(ctx.N, dtype=torch.float64, device=ctx.device)


@pytest.mark.parametrize("max_error", [1.0, 1e-6])
@pytest.mark.parametrize("kind", tr.KINDS)
def test_itergp_bitwise_and_the_scaling_identity(kind, max_error):
    N, D, k, t = 300, 3, 8, 10
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    eps = np.random.default_rng(N).standard_normal((t, k + N))
    ctx = _context(X, y, kind, h, k)
    try:
        plain = ctx.itergp_objective_and_grad(eps, _zeros(ctx), max_error=max_error)
        ctx.itergp_var_cache(16)
        withx = ctx.itergp_objective_and_grad(eps, _zeros(ctx), max_error=max_error, with_input_grad=True)
        assert int(ctx.get_stat("itergp_cache_request")) == 16       # a plain evaluation keeps the variance cache
        assert ctx.get_stat("itergp_grad_ms") > 0.0
    finally:
        ctx.close()
    assert (plain.lml, plain.quad, plain.logdet, plain.logdet_P, plain.steps, plain.residual_error) == \
        (withx.lml, withx.quad, withx.logdet, withx.logdet_P, withx.steps, withx.residual_error)
    assert np.array_equal(ref.grad_vector(plain.grad), ref.grad_vector(withx.grad)) and plain.grad_x is None
    gx = withx.grad_x.cpu().numpy()
    assert gx.shape == (N, D) and np.all(np.isfinite(gx))
    # sum_i x_ik gx[i, k] = -l_k grad["lengthscales"][k] for the estimator's own vectors.  Each side is held to 1e-11 of the sum of absolute terms
    # sum_ij |x_ik| |w_ij| h_ij |delta_ijk| / l_k, which cannot be formed without the evaluation's vectors; sum_i |x_ik gx[i, k]| is below it by the
    # cancellation inside gx[i, k], N terms of mixed sign: about sqrt(N) = 17 here.  100 is allowed for it: 2e-11 x 100 of sum_i |x_ik gx[i, k]|
    ls = np.asarray(h["lengthscales"], dtype=np.float64)
    lhs = (X * gx).sum(axis=0)
    print(f"{kind} max_error={max_error}: scaling identity {np.abs(lhs + ls * withx.grad['lengthscales']).max():.2e} of {(np.abs(X) * np.abs(gx)).sum(axis=0).max():.2e}")
    assert np.all(np.abs(lhs + ls * withx.grad["lengthscales"]) <= 2e-9 * (np.abs(X) * np.abs(gx)).sum(axis=0))


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("case", iref.EXACT_LIMIT_CASES + [(300, 3, 20)], ids=lambda c: "N%d_D%d_k%d" % c)
def test_itergp_unit_probes_give_the_dense_input_gradient(case, kind):
    N, D, k = case
    X, y = ref.problem(N, D)
    h = iref.exact_limit_hypers(D)
    w, _ = tr.gpr_weight(kind, X, y, h)
    want = tr.grad_x(kind, X, h["lengthscales"], h["variance"], w=w)[0].astype(np.float64)
    ctx = _context(X, y, kind, h, k)
    try:
        res = ctx.itergp_objective_and_grad(iref.unit_probes(k, N), _zeros(ctx), max_error=1e-20, max_cg_iter=N, lanczos_iter=N, with_input_grad=True)
    finally:
        ctx.close()
    got = res.grad_x.cpu().numpy()
    print(f"N={N} {kind}: input gradient {np.abs(got - want).max() / np.abs(want).max():.2e} of the largest entry (steps {res.steps})")
    assert np.abs(got - want).max() <= max(100 * 1e-13, 1e-8) * np.abs(want).max()


# ---- gpr -------------------------------------------------------------------------------------------------------------------------------------------
GPR_SHAPES = [(1, 1, None), (2, 3, None), (65, 3, 64), (257, 1, 128), (1500, 8, 128)]


@pytest.mark.parametrize("kind", tr.KINDS)
@pytest.mark.parametrize("shape", GPR_SHAPES, ids=lambda s: "N%d_D%d_b%s" % s)
def test_gpr_bitwise_and_the_dense_input_gradient(shape, kind):
    from cglb_amd.hip_context import HipContext
    N, D, block = shape
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    w, _ = tr.gpr_weight(kind, X, y, h)
    want = tr.grad_x(kind, X, h["lengthscales"], h["variance"], w=w)[0].astype(np.float64)
    ctx = HipContext(X, y, 1, kind, device=torch.device("cuda", 0))
    try:
        if block:
            ctx.set_option("gpr_block", block)
        assert ctx.get_stat("train_input_grad_native") == 1.0
        ctx.gpr_set_hypers(**h)
        plain = ctx.gpr_objective_and_grad()
        withx = ctx.gpr_objective_and_grad(with_input_grad=True)
    finally:
        ctx.close()
    assert (plain.lml, plain.quad, plain.logdet) == (withx.lml, withx.quad, withx.logdet)
    assert np.array_equal(ref.grad_vector(plain.grad), ref.grad_vector(withx.grad)) and plain.grad_x is None
    got = withx.grad_x.cpu().numpy()
    assert got.shape == (N, D) and np.all(np.isfinite(got))
    print(f"N={N} D={D} {kind}: {np.abs(got - want).max() / max(np.abs(want).max(), 1e-300):.2e} of the largest entry")
    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


def _params(model):
    k = model.covar_module
    return [k.base_kernel._lengthscale.raw, k._outputscale.raw, model.likelihood.noise_covar._noise.raw, model.mean_module.constant]


def test_feature_map_through_the_exact_objective(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import InputGradLogMarginalLikelihood
    N, d_raw, d = 200, 5, 3
    raw_np, y = ref.problem(N, d_raw)
    raw = torch.as_tensor(raw_np)
    A = (0.5 * torch.as_tensor(np.random.default_rng(3).standard_normal((d_raw, d)))).requires_grad_(True)
    model = backend.create_model(config.GPRConfig(config.Matern32Config()), ((raw @ A).detach().numpy(), y))
    objective = InputGradLogMarginalLikelihood(model)
    params = _params(model)
    value = objective(raw @ A)
    grads = torch.autograd.grad(value, [A] + params)
    # torch autograd on the CPU lml at the same constrained values, through the same softplus transforms
    p = backend.model_parameters(model)
    A2 = A.detach().clone().requires_grad_(True)
    raws = [q.detach().clone().requires_grad_(True) for q in params]
    k = model.covar_module
    lower = [k.base_kernel._lengthscale.lower_bound, k._outputscale.lower_bound, model.likelihood.noise_covar._noise.lower_bound]
    ls, f, s = [torch.nn.functional.softplus(q) + lo for q, lo in zip(raws[:3], lower)]
    assert np.allclose(ls.detach().numpy().reshape(-1), p[".kernel.lengthscales"], rtol=1e-14)
    assert abs(float(s.detach()) - float(p[".likelihood.variance"])) <= 1e-14
    cpu = tr.torch_lml("matern32", raw @ A2, torch.as_tensor(y), ls.reshape(-1), f.reshape(()), s.reshape(()), raws[3].reshape(()))
    want = torch.autograd.grad(cpu, [A2] + raws)
    assert abs(float(value.detach()) - float(cpu.detach())) <= 1e-10 * (abs(float(cpu.detach())) + 0.5 * N * np.log(2.0 * np.pi))
    for name, g, wv in zip(["A", "lengthscales", "variance", "noise", "mean"], grads, want):
        g, wv = g.detach().numpy().reshape(-1), wv.detach().numpy().reshape(-1)
        print(f"{name}: {np.abs(g - wv).max() / np.abs(wv).max():.2e} of the largest entry")
        assert np.abs(g - wv).max() <= 1e-8 * np.abs(wv).max(), (name, g, wv)
    # two steps of a torch optimiser on the map and the hyper-parameters raise the exact lml
    opt = torch.optim.Adam([A] + params, lr=0.01)
    values = [float(value.detach())]
    for _ in range(2):
        opt.zero_grad()
        (-objective(raw @ A)).backward()
        opt.step()
    values.append(float(objective(raw @ A).detach()))
    assert values[1] > values[0], values


def test_feature_map_through_the_iterative_objective(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import InputGradStochasticLogMarginalLikelihood
    N, d_raw, d = 200, 5, 3
    raw_np, y = ref.problem(N, d_raw)
    raw = torch.as_tensor(raw_np)
    A = (0.5 * torch.as_tensor(np.random.default_rng(3).standard_normal((d_raw, d)))).requires_grad_(True)
    model = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), ((raw @ A).detach().numpy(), y))
    objective = InputGradStochasticLogMarginalLikelihood(model)
    params = _params(model)
    opt = torch.optim.Adam([A] + params, lr=0.01)
    for _ in range(2):
        opt.zero_grad()
        (-objective(raw @ A)).backward()
        assert A.grad.shape == (d_raw, d) and bool(torch.isfinite(A.grad).all()) and float(A.grad.abs().max()) > 0
        for q in params:
            assert q.grad.shape == q.shape and bool(torch.isfinite(q.grad).all())
        opt.step()
    # no gradient asked of x: none is computed, the value comes all the same
    assert bool(torch.isfinite(objective((raw @ A).detach()).detach()))


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------
def test_set_inputs_voids_the_hyper_parameters_and_the_cache():
    N, D, k = 130, 3, 8
    X, y = ref.problem(N, D)
    X2 = X + 0.25 * np.random.default_rng(7).standard_normal(X.shape)
    h = ref.hypers(D, True)
    eps = np.random.default_rng(N).standard_normal((4, k + N))
    U, V = _pairs(N, 2)
    ctx = _context(X, y, "matern32", h, k)
    fresh = _context(X2, y, "matern32", h, k)
    try:
        ctx.gpr_set_hypers(**h)
        ctx.itergp_objective_and_grad(eps, _zeros(ctx))
        ctx.itergp_var_cache(8)
        mean_before = ctx.itergp_predict(X[:5], var_rank=8)[0].cpu().numpy()
        ctx.set_inputs(X2)
        assert int(ctx.get_stat("itergp_cache_request")) == 0        # the variance cache went with the inputs
        with pytest.raises(RuntimeError, match="call order"):
            ctx.grad_x_kff_multi(U, V)
        with pytest.raises(RuntimeError, match="call order"):
            ctx.itergp_objective_and_grad(eps, _zeros(ctx), with_input_grad=True)
        with pytest.raises(RuntimeError, match="call order"):
            ctx.gpr_objective_and_grad(with_input_grad=True)
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X2[:k].copy(), 1e-6)
        ctx.gpr_set_hypers(**h)
        assert np.array_equal(ctx.grad_x_kff_multi(U, V).cpu().numpy(), fresh.grad_x_kff_multi(U, V).cpu().numpy())
        a = ctx.itergp_objective_and_grad(eps, _zeros(ctx), with_input_grad=True)
        b = fresh.itergp_objective_and_grad(eps, _zeros(fresh), with_input_grad=True)
        assert a.lml == b.lml and np.array_equal(a.grad_x.cpu().numpy(), b.grad_x.cpu().numpy())
        assert not np.array_equal(ctx.itergp_predict(X[:5])[0].cpu().numpy(), mean_before)
        fresh.gpr_set_hypers(**h)
        ga, gb = ctx.gpr_objective_and_grad(with_input_grad=True), fresh.gpr_objective_and_grad(with_input_grad=True)
        assert ga.lml == gb.lml and np.array_equal(ga.grad_x.cpu().numpy(), gb.grad_x.cpu().numpy())
    finally:
        ctx.close()
        fresh.close()


def test_set_train_inputs_equals_a_fresh_model(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import InputGradLogMarginalLikelihood, LogMarginalLikelihood, PredictGPR
    N, D = 130, 3
    X, y = ref.problem(N, D)
    X2 = X + 0.25 * np.random.default_rng(7).standard_normal(X.shape)
    model = backend.create_model(config.GPRConfig(config.Matern32Config()), (X, y))
    fresh = backend.create_model(config.GPRConfig(config.Matern32Config()), (X2, y))
    before = PredictGPR(model)(torch.as_tensor(X[:5]))[0]
    model.set_train_inputs(torch.as_tensor(X2))
    a, b = LogMarginalLikelihood(model)((X2, y)), LogMarginalLikelihood(fresh)(None)
    assert float(a.detach()) == float(b.detach())                     # bitwise
    x = torch.as_tensor(X2).clone().requires_grad_(True)
    ga = torch.autograd.grad(InputGradLogMarginalLikelihood(model)(x), [x])[0]
    x2 = torch.as_tensor(X2).clone().requires_grad_(True)
    gb = torch.autograd.grad(InputGradLogMarginalLikelihood(fresh)(x2), [x2])[0]
    assert torch.equal(ga, gb) and ga.shape == (N, D)
    # the neighbouring predictor follows the new inputs and is otherwise left alone
    after, after_fresh = PredictGPR(model)(torch.as_tensor(X[:5]))[0], PredictGPR(fresh)(torch.as_tensor(X[:5]))[0]
    assert torch.equal(after, after_fresh) and not torch.equal(after, before)
    with pytest.raises(ValueError):
        model.set_train_inputs(torch.as_tensor(X2[:10]))


def test_refusals_agree_with_the_stat():
    from cglb_amd.hip_context import HipContext
    dev = torch.device("cuda", 0)
    # d = 40
    N = 65
    X, y = ref.problem(N, 40)
    h = ref.hypers(40, True)
    U, V = _pairs(N, 2)
    ctx = _context(X, y, "rbf", h, 4)
    try:
        assert ctx.get_stat("train_input_grad_native") == 0.0
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.grad_x_kff_multi(U, V)
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.itergp_objective_and_grad(np.ones((2, 4 + N)), _zeros(ctx), with_input_grad=True)
        ctx.gpr_set_hypers(**h)
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.gpr_objective_and_grad(with_input_grad=True)
        assert ctx.gpr_objective_and_grad().grad_x is None             # the plain entries still run there
    finally:
        ctx.close()
    # fp32
    X, y = ref.problem(N, 3)
    h = ref.hypers(3, True)
    ctx = _context(X, y, "rbf", h, 4, dtype=torch.float32)
    try:
        assert ctx.get_stat("train_input_grad_native") == 0.0
        with pytest.raises(ValueError, match="fp64"):
            ctx.grad_x_kff_multi(U, V)
        with pytest.raises(ValueError, match="fp64"):
            ctx.itergp_objective_and_grad(np.ones((2, 4 + N)), torch.zeros(N, dtype=torch.float32, device=dev), with_input_grad=True)
        with pytest.raises(ValueError, match="fp64"):
            ctx.gpr_objective_and_grad(with_input_grad=True)
    finally:
        ctx.close()
    # P > 1
    Y = np.stack([y, -y], axis=1)
    ctx = HipContext(X, Y, 4, "rbf", device=dev)
    try:
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:4].copy(), 1e-6)
        assert ctx.get_stat("train_input_grad_native") == 0.0
        with pytest.raises(ValueError, match="one target column"):
            ctx.grad_x_kff_multi(U, V)
        with pytest.raises(ValueError, match="one target column"):
            ctx.itergp_objective_and_grad(np.ones((2, 4 + N)), _zeros(ctx), with_input_grad=True)
        with pytest.raises(ValueError, match="one target column"):
            ctx.gpr_objective_and_grad(with_input_grad=True)
    finally:
        ctx.close()
