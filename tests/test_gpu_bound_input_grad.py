"""Training-input gradients of the CGLB / SGPR bounds on the GPU (cglb_objective_and_grad_x, cglb_grad_x_kuf, cglb_grad_x_kff_pair).

1. The transposed panel pass, every element, per cell of bound_input_grad_ref.kuf_cells (every rows-per-lane class at one row past its row block and
   one row past 4096; M in 1, 16, 130; forced splits of the inducing points 1, 3, 7 and the rule; ldg > N; cvec / wvec NULL; a training point equal to
   an inducing point, which must add exactly zero; a row at 10^3; the three kinds at both hyper-parameter sets) against the np.longdouble
   restatement: 1e-11 of sum_m |G_mn + c_m w_n| h |delta_k| / l_k.  Two calls bitwise equal; the buffer starts NaN and every element is written.
2. The single-pair K_ff pass, every element, per cell of pair_cells (every rows-per-lane class at one row past its row block with forced splits 1,
   3, 7; one row past a launch block, checked on its first row block and the 513 rows around the boundary) to train_input_grad_ref.tolerance, and against grad_x_kff_multi at S = 1 within 2 * 2 (N + 1) 2^-53 of the sum
   of absolute terms (the permutation bound of tests/test_gpu_train_input_grad.py, doubled: two summation orders of the same terms).
3. The evaluation: shapes, hyper-parameters, solve-then-evaluate protocol and gradient rule of tests/test_gpu_bound_variants.py for cglb / cglbnm2 /
   sgpr x three kinds x two hyper-parameter sets: grad_x to 1e-8 of the largest entry of the autograd gradient of the dense restatement; out4, grad,
   steps and v bitwise those of the call without the input gradient; the translation and scaling identities within 2e-8 of their sums of absolute
   terms.
4. Refusals with their messages and the statistic; the forgotten set_hypers after set_inputs.
5. End to end: x = raw @ A through InputGradLowerBoundCG / InputGradLowerBoundSGPR.
"""
import functools

import numpy as np
import pytest
import torch

import bound_input_grad_ref as br
import gpr_ref
import train_input_grad_ref as tr
from cglb_amd.data import synthetic_problem
from test_gpu_bound_variants import SHAPES, _assert_grad_close, _context, _hypers

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


# ---- the transposed panel pass, every element ---------------------------------------------------------------------------------------------------
def _panel_problem(c):
    """inputs with a row at 10^3, inducing points of which one IS a training point, panel with padding columns set to NaN (never read)"""
    N, M, D = c["N"], c["M"], c["D"]
    rng = np.random.default_rng(7 * N + 3 * M + D)
    X = gpr_ref.problem(N, D)[0].copy()
    y = rng.standard_normal(N)
    Z = rng.standard_normal((M, D))
    if N >= 4:
        X[2] = 1.0e3
    Z[0] = X[N // 2]                       # a coincident pair
    G = np.full((M, N + c["pad"]), np.nan)
    G[:, :N] = rng.standard_normal((M, N))
    cvec, wvec = (rng.standard_normal(M), rng.standard_normal(N)) if c["rank_one"] else (None, None)
    return X, y, Z, G, cvec, wvec


@functools.lru_cache(maxsize=None)
def _panel_reference(idx):
    c = br.kuf_cells()[idx]
    X, _, Z, G, cvec, wvec = _panel_problem(c)
    h = gpr_ref.hypers(c["D"], c["trained"])
    gx, scale = br.kuf_grad_x(c["kind"], X, Z, h["lengthscales"], h["variance"], G[:, :c["N"]], cvec, wvec)
    out = gx.astype(np.float64), scale.astype(np.float64)
    for a in out:
        a.setflags(write=False)
    return out


def _cell_id(c):
    return "N%d_M%d_D%d_ms%d_pad%d_%s_%s_%s" % (c["N"], c["M"], c["D"], c["msplit"], c["pad"], "c" if c["rank_one"] else "noc", c["kind"],
                                               "trained" if c["trained"] else "init")


@pytest.mark.parametrize("idx", range(len(br.kuf_cells())), ids=lambda i: _cell_id(br.kuf_cells()[i]))
def test_panel_pass_every_element(idx):
    from cglb_amd.hip_context import HipContext
    c = br.kuf_cells()[idx]
    X, y, Z, G, cvec, wvec = _panel_problem(c)
    h = gpr_ref.hypers(c["D"], c["trained"])
    want, scale = _panel_reference(idx)
    ctx = HipContext(X, y, c["M"], c["kind"], device=torch.device("cuda", 0))
    try:
        if c["msplit"]:
            ctx.set_option("kuf_msplit", c["msplit"])
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
        assert ctx.get_stat("train_input_grad_native") == 1.0
        got = ctx.grad_x_kuf(G, cvec, wvec).cpu().numpy()
        again = ctx.grad_x_kuf(G, cvec, wvec).cpu().numpy()
        # the coincident pair adds exactly zero whatever its weight: another panel entry there leaves that training point's row bitwise the same
        G0 = G.copy()
        G0[0, c["N"] // 2] = 12345.0
        other = ctx.grad_x_kuf(G0, cvec, wvec).cpu().numpy()
    finally:
        ctx.close()
    assert got.shape == (c["N"], c["D"]) and np.all(np.isfinite(got))     # the buffer starts as NaN: every element was written
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print(f"{_cell_id(c)}: largest error {err[scale > 0].max() if (scale > 0).any() else 0.0:.2e} of the sum of absolute terms; chunks "
          f"{br.kuf_split(c['N'], c['M'], c['D'], c['msplit'])}")
    assert np.all(np.abs(got - want) <= br.TOL * scale), (np.abs(got - want).max(), err.max())
    assert np.array_equal(got, again)
    n0 = c["N"] // 2
    assert np.array_equal(got, other)
    if c["M"] == 1:                                                       # the only inducing point of that training point IS it: exactly zero
        assert np.all(got[n0] == 0.0)
    if c["N"] >= 4:
        assert np.all(np.abs(got[2]) <= br.TOL * scale[2])               # the row at 10^3: everything underflows


def test_the_tables_reach_every_class():
    assert {br.kuf_rows_per_lane(c["D"]) for c in br.kuf_cells()} == {br.kuf_rows_per_lane(d) for d in range(1, 33)}
    assert {br.pair_rows_per_lane(c[1]) for c in br.pair_cells()} == {br.pair_rows_per_lane(d) for d in range(1, 33)}


# ---- the single-pair K_ff pass, every element --------------------------------------------------------------------------------------------------
def _pair_problem(N, D):
    X, y = gpr_ref.problem(N, D)
    X = X.copy()
    if N >= 4:
        X[1] = X[0]
        X[2] = 1.0e3
    rng = np.random.default_rng(1000 + N + D)
    return X, y, rng.standard_normal(N), rng.standard_normal(N)


def _pair_rows(N):
    """the rows a cell is checked on: all of them, or - past a launch block, where the np.longdouble square would take many seconds - the first row
    block and the 513 rows around the boundary of the launch blocks"""
    return np.arange(N) if N <= 4200 else np.concatenate([np.arange(256), np.arange(N - 513, N)])


@functools.lru_cache(maxsize=None)
def _pair_reference(kind, N, D, trained):
    X, _, u, v = _pair_problem(N, D)
    h = gpr_ref.hypers(D, trained)
    if N <= 4200:
        gx, scale = br.kff_pair_grad_x(kind, X, h["lengthscales"], h["variance"], u, v)
        U, V = u.reshape(-1, 1), v.reshape(-1, 1)
        wsum = np.concatenate([np.abs(tr.pair_weights(U, V, rows=slice(i, i + 512))).sum(axis=1) for i in range(0, N, 512)])
    else:
        gx, scale, wsum = br.kff_pair_grad_x_rows(kind, X, h["lengthscales"], h["variance"], u, v, _pair_rows(N))
    out = gx.astype(np.float64), tr.tolerance(scale, wsum, h["variance"]), scale.astype(np.float64)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("cell", br.pair_cells(), ids=lambda c: "N%d_D%d_js%d_%s_%s" % (c[0], c[1], c[2], c[3], "trained" if c[4] else "init"))
def test_pair_pass_every_element(cell):
    from cglb_amd.hip_context import HipContext
    N, D, jsplit, kind, trained = cell
    X, y, u, v = _pair_problem(N, D)
    h = gpr_ref.hypers(D, trained)
    want, tol, scale = _pair_reference(kind, N, D, trained)
    ctx = HipContext(X, y, 1, kind, device=torch.device("cuda", 0))
    try:
        if jsplit:
            ctx.set_option("kff_jsplit", jsplit)
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:1].copy(), 1e-6)
        got = ctx.grad_x_kff_pair(u, v).cpu().numpy()
        again = ctx.grad_x_kff_pair(u, v).cpu().numpy()
        multi = ctx.grad_x_kff_multi(u.reshape(-1, 1), v.reshape(-1, 1)).cpu().numpy()
    finally:
        ctx.close()
    assert got.shape == (N, D) and np.all(np.isfinite(got))
    assert np.array_equal(got, again)
    rows = _pair_rows(N)
    got, multi = got[rows], multi[rows]
    err = np.abs(got - want) / np.maximum(scale, 1e-300)
    print(f"{cell}: largest error {err[scale > 0].max() if (scale > 0).any() else 0.0:.2e} of the sum of absolute terms; against the G-wide instance "
          f"{(np.abs(got - multi) / np.maximum(scale, 1e-300)).max():.2e} (bound {4 * (N + 1) * EPS:.2e})")
    assert np.all(np.abs(got - want) <= tol), (np.abs(got - want).max(), err.max())
    assert np.all(np.abs(got - multi) <= 2 * 2 * (N + 1) * EPS * scale)
    if N >= 4:
        assert np.all(np.abs(got[2]) <= tol[2])


# ---- the evaluation ----------------------------------------------------------------------------------------------------------------------------------
def _solve_then_evaluate(ctx, h, Z, cls, with_x):
    """the protocol of tests/test_gpu_bound_variants.py (_evaluate), with the input gradient asked of the evaluation"""
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
    v = torch.zeros(ctx.N, dtype=ctx.dtype, device=ctx.device)
    if br.OPTIONS[cls][1] == 0:
        ctx.objective_and_grad(v, run_cg=True, max_error=1.0, with_grad=False)
    return ctx.objective_and_grad(v, run_cg=False, with_input_grad=with_x), v


def _same_result(a, b):
    assert (a.bound, a.lower, a.upper, a.logdet, a.steps) == (b.bound, b.lower, b.upper, b.logdet, b.steps)
    assert (a.residual_error == b.residual_error) or (np.isnan(a.residual_error) and np.isnan(b.residual_error))
    for k in a.grad:
        assert np.array_equal(np.asarray(a.grad[k]), np.asarray(b.grad[k])), k


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] <= 32], ids=lambda s: "N%d_M%d_D%d" % s)
@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("cls", br.CLASSES)
def test_evaluation_matches_the_restatement(cls, kind, shape):
    N, M, D = shape
    assert shape in [(300, 16, 1), (2999, 128, 3), (2999, 16, 8)]
    X, y, Z = synthetic_problem(N, D, M, seed=N + D)
    for trained in (False, True):
        h = _hypers(D, trained)
        ctx = _context(X, y, M, kind, cls)
        try:
            assert ctx.get_stat("bound_input_grad_native") == 1.0
            plain, v0 = _solve_then_evaluate(ctx, h, Z, cls, False)
            res, v = _solve_then_evaluate(ctx, h, Z, cls, True)
        finally:
            ctx.close()
        _same_result(plain, res)                                   # out4, grad, steps: bitwise those of the call without gx_out
        assert torch.equal(v0, v) and plain.grad_x is None
        vv = None if br.OPTIONS[cls][1] else v.cpu().numpy()
        b, gx_ref, g_ref = br.bound_and_grad_x(cls, kind, X, y, h, Z, v=vv, device="cuda")
        assert abs(res.bound - b) <= 1e-10 * abs(b), (trained, res.bound, b)
        _assert_grad_close(res.grad, g_ref, 1e-8)
        gx = res.grad_x.cpu().numpy()
        assert gx.shape == (N, D) and np.all(np.isfinite(gx))
        big = np.abs(gx_ref).max()
        # the two identities within one evaluation, each within 2e-8 of its sum of absolute terms
        gZ, gl, ls = np.asarray(res.grad["Z"]), np.asarray(res.grad["lengthscales"]), np.asarray(h["lengthscales"], dtype=np.float64)
        t_res = np.abs(gx.sum(axis=0) + gZ.sum(axis=0))
        t_abs = np.abs(gx).sum(axis=0) + np.abs(gZ).sum(axis=0)
        s_res = np.abs((X * gx).sum(axis=0) + (Z * gZ).sum(axis=0) + ls * gl)
        s_abs = np.abs(X * gx).sum(axis=0) + np.abs(Z * gZ).sum(axis=0) + np.abs(ls * gl)
        print(f"{cls} {kind} {shape} trained={trained}: grad_x {np.abs(gx - gx_ref).max() / big:.2e} of the largest entry {big:.3g}; translation "
              f"{(t_res / t_abs).max():.2e}, scaling {(s_res / s_abs).max():.2e} of the sums of absolute terms")
        assert np.abs(gx - gx_ref).max() <= 1e-8 * big
        assert np.all(t_res <= 2e-8 * t_abs)
        assert np.all(s_res <= 2e-8 * s_abs)


@pytest.mark.parametrize("cls", ["cglb", "cglbnm2"])
def test_a_solve_with_the_input_gradient_is_bitwise_the_solve_without(cls):
    N, M, D = 1500, 64, 3
    X, y, Z = synthetic_problem(N, D, M, seed=2)
    h = _hypers(D, True)
    ctx = _context(X, y, M, "matern32", cls)
    try:
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
        va = torch.zeros(N, dtype=torch.float64, device=ctx.device)
        vb = va.clone()
        a = ctx.objective_and_grad(va, run_cg=True, max_error=1.0)
        gv_a = ctx.objective_grad_v()
        b = ctx.objective_and_grad(vb, run_cg=True, max_error=1.0, with_input_grad=True)
        gv_b = ctx.objective_grad_v()                              # the state left behind: r and w of the evaluation
        again = ctx.objective_and_grad(va.clone().zero_(), run_cg=True, max_error=1.0, with_input_grad=True)
        with pytest.raises(ValueError, match="with_grad"):
            ctx.objective_and_grad(va, run_cg=False, with_grad=False, with_input_grad=True)
    finally:
        ctx.close()
    assert a.steps > 0
    _same_result(a, b)
    assert torch.equal(va, vb) and torch.equal(gv_a, gv_b)
    assert torch.equal(b.grad_x, again.grad_x)                     # two evaluations: bitwise equal input gradients


# ---- refusals and state --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["logdet_bound 2", "D = 40", "fp32", "P = 2"])
def test_refusals_name_their_reason(case):
    from cglb_amd.hip_context import HipContext
    N, M = 200, 8
    D = 40 if case == "D = 40" else 3
    dtype = torch.float32 if case == "fp32" else torch.float64
    X, y, Z = synthetic_problem(N, D, M, seed=1)
    if case == "P = 2":
        y = np.stack([y, y[::-1]], axis=1)
    ctx = HipContext(X, y, M, "rbf", dtype=dtype, device=torch.device("cuda", 0))
    match = {"logdet_bound 2": "logdet_bound 2", "D = 40": "32 input dimensions", "fp32": "fp64", "P = 2": "one target column"}[case]
    try:
        if case == "logdet_bound 2":
            ctx.set_option("logdet_bound", 2)
        h = _hypers(D, True)
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
        assert ctx.get_stat("bound_input_grad_native") == 0.0
        v = torch.zeros((N, 2) if case == "P = 2" else N, dtype=dtype, device=ctx.device)
        with pytest.raises(ValueError, match=match):
            ctx.objective_and_grad(v, run_cg=False, with_input_grad=True)
        res = ctx.objective_and_grad(v, run_cg=False)              # the refusal left the context usable
        assert np.isfinite(res.bound)
    finally:
        ctx.close()


def test_an_evaluation_after_set_inputs_needs_set_hypers():
    N, M, D = 300, 16, 3
    X, y, Z = synthetic_problem(N, D, M, seed=4)
    X2 = X + 0.25 * np.random.default_rng(7).standard_normal(X.shape)
    h = _hypers(D, True)
    ctx = _context(X, y, M, "matern32", "cglb")
    fresh = _context(X2, y, M, "matern32", "cglb")
    try:
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
        v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
        ctx.objective_and_grad(v, run_cg=True, with_input_grad=True)
        ctx.set_inputs(X2)
        with pytest.raises(RuntimeError):
            ctx.objective_and_grad(v, run_cg=False, with_input_grad=True)
        with pytest.raises(RuntimeError):
            ctx.grad_x_kff_pair(np.ones(N), np.ones(N))
        a, va = _solve_then_evaluate(ctx, h, Z, "cglb", True)      # after the push: the evaluation of a context built on the new inputs
        b, vb = _solve_then_evaluate(fresh, h, Z, "cglb", True)
    finally:
        ctx.close()
        fresh.close()
    _same_result(a, b)
    assert torch.equal(va, vb) and torch.equal(a.grad_x, b.grad_x)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


@pytest.mark.parametrize("cls", ["cglb", "sgpr"])
def test_feature_map_through_the_bound(backend, cls):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import InputGradLowerBoundCG, InputGradLowerBoundSGPR, LowerBoundCG, LowerBoundSGPR
    N, d_raw, d = 400, 5, 3
    raw_np, y = gpr_ref.problem(N, d_raw)
    raw = torch.as_tensor(raw_np)
    A = (0.5 * torch.as_tensor(np.random.default_rng(3).standard_normal((d_raw, d)))).requires_grad_(True)
    cfg = (config.CGLBConfig if cls == "cglb" else config.SGPRConfig)(config.Matern32Config(), config.InducingVariableConfig(24))
    model = backend.create_model(cfg, ((raw @ A).detach().numpy(), y))
    params = [p for p in model.parameters()]
    if cls == "cglb":
        first = InputGradLowerBoundCG(model)(raw @ A)              # solves: model.v_vec is the solution from here on
        assert model.cg_stats is not None and bool(torch.isfinite(first.detach()))
        objective = InputGradLowerBoundCG(model, use_cache=True, cached_v_vec_initial=True)   # evaluates at that v, as the plain objective below
        plain = LowerBoundCG(model, use_cache=True, cached_v_vec_initial=True)
        v = model.v_vec.detach().reshape(-1).cpu().numpy()
    else:
        objective, plain, v = InputGradLowerBoundSGPR(model), LowerBoundSGPR(model), None
    value = objective(raw @ A)
    grads = torch.autograd.grad(value, [A] + params)
    value_plain = plain(None)
    grads_plain = torch.autograd.grad(value_plain, params)
    assert float(value.detach()) == float(value_plain.detach())
    for p, g, gp in zip(params, grads[1:], grads_plain):           # hyper-parameters and Z: those of the plain objective at the same inputs
        assert g.shape == p.shape and torch.equal(g, gp)
    q = backend.model_parameters(model)
    h = dict(lengthscales=q[".kernel.lengthscales"], variance=float(q[".kernel.variance"]), noise=float(q[".likelihood.variance"]),
             mean=float(q[".mean_function.c"]))
    b, gA, _ = br.bound_and_grad_x(cls, "matern32", None, y, h, q[".inducing_variable.Z"], v=v, device="cuda", x_map=(raw_np, A.detach().numpy()))
    got = grads[0].detach().numpy()
    print(f"{cls}: A.grad {np.abs(got - gA).max() / np.abs(gA).max():.2e} of the largest entry {np.abs(gA).max():.3g}")
    assert abs(float(value.detach()) - b) <= 1e-10 * abs(b)
    assert got.shape == (d_raw, d) and np.abs(got - gA).max() <= 1e-8 * np.abs(gA).max()
    # no gradient asked of x: none is computed, the value comes all the same
    assert float(objective((raw @ A).detach()).detach()) == float(value.detach())
