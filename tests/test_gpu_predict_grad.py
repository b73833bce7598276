"""Input gradients of the CGLB / SGPR / exact-GP predictive (cglb_cross_grad_weighted, cglb_predict_grad, cglb_gpr_predict_grad,
`PredictGradCG`, `PredictGradSGPR`, `PredictGradGPR`) against tests/predict_grad_ref.py.  Small shapes; every output is pre-filled with NaN.

1. The row-weighted product, every element against the longdouble restatement: the table predict_grad_ref.product_cells (rows-per-lane classes at
   D in 1, 3, 8, 9, 20, 32; n_new in 1, B - 1, B, B + 1, 4097; 1, 65, 300 points; both point sets; kff_jsplit forced to 1, 3, 7; the three kinds;
   precision levels 0 and 1; ldw > n_new with NaN in the padding columns).  u-only, Wt-only and both are bitwise equal where they overlap, a second
   run is bitwise equal; a new point on a point of the set whose weight is the only non-zero one has gradient exactly 0.0; at the point at 10^3
   every kernel value underflows and the outputs are within the floor of the range-clamped 2^x (2^-1000 times the weights: the kernel always runs
   the clamped exponential, so an exact 0.0 is not what it returns there; the floor term of the tolerance is all that is left).
2. cglb_predict_grad on the fp64 cells of group B of predict_ref.CASES and one Matern-5/2 cell, quad_term 0 and 1 (v holds NaN there): f_mean /
   f_var bitwise those of cglb_predict, gradients within 1e-8 max(max |ref|, G_k) of the autograd reference, with_var False bitwise the same mean
   outputs; one cell with n_new = 4097.
3. cglb_gpr_predict_grad on group D up to n_new = 4097: bitwise values, gradients against the dense autograd reference.
4. The backend classes, `mean_and_variance` under autograd, their refusals.  5. The library's refusals.  6. The neighbours' state.
"""
import numpy as np
import pytest
import torch

import gpr_ref
import input_grad_ref as ig
import predict_grad_ref as pg
import predict_ref as pr

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _nan(ctx, *shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=ctx.device)


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


# ---- 1. the product ----------------------------------------------------------------------------------------------------------------------------
CELLS = pg.product_cells()


def test_the_cells_reach_every_instance_class():
    assert {pg.rows_per_lane(c["D"]) for c in CELLS} == set(pg.CLASSES) == {4, 2, 1}


def _product_context(c, X, y, Z):
    from cglb_amd.hip_context import HipContext
    h = ig.cell_hypers(c["D"])
    ctx = HipContext(X, y, len(Z), c["kind"], dtype=torch.float64, device=torch.device("cuda", 0))
    ctx.set_option("precision", c["precision"])
    ctx.set_option("kff_jsplit", c["jsplit"])
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
    return ctx, h


@pytest.mark.parametrize("c", CELLS, ids=pg.cell_id)
def test_product_matches_the_restatement(c):
    X, y, Z, xnew, u, Wt = pg.cell_problem(c)
    P = X if c["set"] == "train" else Z
    n, D = c["n_new"], c["D"]
    ctx, h = _product_context(c, X, y, Z)
    try:
        outs = lambda: dict(out_u=_nan(ctx, n), gout_u=_nan(ctx, n, D), out_w=_nan(ctx, n), gout_w=_nan(ctx, n, D))
        both = _np(ctx.cross_grad_weighted(xnew, u, Wt, c["set"], **outs()))
        again = _np(ctx.cross_grad_weighted(xnew, u, Wt, c["set"], **outs()))
        only_u = _np(ctx.cross_grad_weighted(xnew, u, None, c["set"], out_u=_nan(ctx, n), gout_u=_nan(ctx, n, D)))
        only_w = _np(ctx.cross_grad_weighted(xnew, None, Wt, c["set"], out_w=_nan(ctx, n), gout_w=_nan(ctx, n, D)))
        grads = _np(ctx.cross_grad_weighted(xnew, u, Wt, c["set"], with_value=False))
        # the coincident pair alone: new point 0 sits on point j0 of the set; every other weight zero
        j0 = min(3, len(P) - 1)
        u1, W1 = np.zeros(len(P)), np.zeros((len(P), n))
        u1[j0], W1[j0, 0] = 1.5, -2.5
        lone = _np(ctx.cross_grad_weighted(xnew, u1, W1, c["set"]))
    finally:
        ctx.close()
    want = pg.weighted_product(c["kind"], xnew, P, h["lengthscales"], h["variance"], u, Wt)
    tol = pg.weighted_tolerance(c["kind"], xnew, P, h["lengthscales"], h["variance"], u, Wt)
    worst = []
    for got, w, t in zip(both, want, tol):
        assert got.shape == w.shape and np.all(np.isfinite(got))
        worst.append(float((np.abs(got - w) / t).max()))
    print(f"{pg.cell_id(c)}: out_u {worst[0]:.2e}, gout_u {worst[1]:.2e}, out_w {worst[2]:.2e}, gout_w {worst[3]:.2e} of the tolerance")
    assert max(worst) <= 1.0
    for a, b in zip(both, again):
        assert np.array_equal(a, b)
    assert np.array_equal(only_u[0], both[0]) and np.array_equal(only_u[1], both[1]) and only_u[2] is None and only_u[3] is None
    assert np.array_equal(only_w[2], both[2]) and np.array_equal(only_w[3], both[3]) and only_w[0] is None and only_w[1] is None
    assert grads[0] is None and grads[2] is None and np.array_equal(grads[1], both[1]) and np.array_equal(grads[3], both[3])
    assert np.all(lone[1][0] == 0.0) and np.all(lone[3][0] == 0.0)            # exactly zero, not merely small
    assert abs(lone[0][0] - 1.5 * h["variance"]) <= ig.TOL * 1.5 * h["variance"] and abs(lone[2][0] + 2.5 * h["variance"]) <= ig.TOL * 2.5 * h["variance"]
    if n > 1:   # the point at 10^3: the kernel values underflow; the range-clamped 2^x leaves at most its floor (the floor term of the tolerance alone)
        fu, fw = ig.FLOOR * h["variance"] * np.abs(u).sum(), ig.FLOOR * h["variance"] * np.abs(Wt[:, 1]).sum()
        assert abs(both[0][1]) <= fu and np.all(np.abs(both[1][1]) <= fu) and abs(both[2][1]) <= fw and np.all(np.abs(both[3][1]) <= fw)


def test_out_tensors_are_checked():
    X, y = gpr_ref.problem(65, 3)
    c = dict(D=3, kind="rbf", precision=0, jsplit=0)
    ctx, _ = _product_context(c, X, y, X[:7].copy())
    try:
        with pytest.raises(ValueError, match="gout_u"):
            ctx.cross_grad_weighted(X[:4], np.ones(65), gout_u=torch.zeros((4, 2), dtype=torch.float64, device=ctx.device))
        with pytest.raises(ValueError, match="out_w"):
            ctx.cross_grad_weighted(X[:4], np.ones(65), out_w=torch.zeros(4, dtype=torch.float64, device=ctx.device))
        with pytest.raises(ValueError, match="Wt"):
            ctx.cross_grad_weighted(X[:4], None, np.ones((65, 3)))
        with pytest.raises(ValueError, match="g_mean"):
            ctx.predict_grad(np.zeros(65), X[:4], g_mean=torch.zeros((4, 3), dtype=torch.float32, device=ctx.device))
    finally:
        ctx.close()


# ---- 2. cglb_predict_grad ---------------------------------------------------------------------------------------------------------------------
def _check_grad(case, hyp, outs, ref: pg.Grad, what):
    tol = pg.predictor_tolerance(case.kind, hyp, ref)
    got = pg.Grad(*outs)
    for name in ("mean", "g_mean", "var", "g_var"):
        a = getattr(got, name)
        assert a.shape == getattr(ref, name).shape and np.all(np.isfinite(a)), (what, name)
    miss = {name: float((np.abs(getattr(got, name) - getattr(ref, name)) / tol[name]).max()) for name in ("mean", "g_mean", "var", "g_var")}
    print(f"{case.id} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in miss.items()) + " of the tolerance")
    assert max(miss.values()) <= 1.0, (what, miss)


def _run_cglb_case(case):
    X, y, hyp, v = pr.problem(case)
    xn = pr.xnew(case)
    n, D = case.n_new, case.D
    ctx = pr.make_ctx(case, device=torch.device("cuda", 0))
    try:
        for q in (0, 1):
            ctx.set_option("logdet_bound", q)      # quad_term 1 with the NM^2 bound: the SGPR class, as tests/test_gpu_predict_geometry.py sets it
            ctx.set_option("quad_term", q)
            ctx.setup()
            vq = np.full(case.N, NAN) if q else v
            mean, var = pr.predict(ctx, vq, xn)
            outs = _np(ctx.predict_grad(vq, xn, f_mean=_nan(ctx, n), g_mean=_nan(ctx, n, D), f_var=_nan(ctx, n), g_var=_nan(ctx, n, D)))
            assert np.array_equal(outs[0], mean) and np.array_equal(outs[2], var)       # bitwise cglb_predict
            _check_grad(case, hyp, outs, pg.cglb_reference(case, q), f"quad_term {q}")
            m2, g2, v2, gv2 = _np(ctx.predict_grad(vq, xn, with_var=False, f_mean=_nan(ctx, n), g_mean=_nan(ctx, n, D)))
            assert v2 is None and gv2 is None and np.array_equal(m2, outs[0]) and np.array_equal(g2, outs[1])
    finally:
        ctx.close()


@pytest.mark.parametrize("case", pg.CGLB_CASES, ids=lambda c: c.id)
def test_cglb_predict_grad(case):
    _run_cglb_case(case)


def test_cglb_predict_grad_beyond_one_launch():
    _run_cglb_case(pg.LARGE_CASE)


# ---- 3. cglb_gpr_predict_grad -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pg.GPR_CASES, ids=lambda c: c.id)
def test_gpr_predict_grad(case):
    X, y, hyp, _ = pr.problem(case)
    xn = pr.xnew(case)
    n, D = case.n_new, case.D
    ctx = pr.make_ctx(case, M=1, device=torch.device("cuda", 0))
    try:
        ctx.gpr_set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean)
        mean, var = pr.gpr_predict(ctx, xn)
        outs = _np(ctx.gpr_predict_grad(xn, f_mean=_nan(ctx, n), g_mean=_nan(ctx, n, D), f_var=_nan(ctx, n), g_var=_nan(ctx, n, D)))
        again = _np(ctx.gpr_predict_grad(xn))
        m2, g2, v2, gv2 = _np(ctx.gpr_predict_grad(xn, with_var=False))
        mean3, var3 = pr.gpr_predict(ctx, xn)
    finally:
        ctx.close()
    assert np.array_equal(outs[0], mean) and np.array_equal(outs[2], var)
    assert np.array_equal(mean3, mean) and np.array_equal(var3, var)
    for a, b in zip(outs, again):
        assert np.array_equal(a, b)
    assert v2 is None and gv2 is None and np.array_equal(m2, mean) and np.array_equal(g2, outs[1])
    _check_grad(case, hyp, outs, pg.gpr_reference(case), "gpr")


# ---- 4. the backend -------------------------------------------------------------------------------------------------------------------------
N_B, D_B, M_B = 160, 3, 16


def _model(name, columns=1):
    from cglb_amd.backend import config
    from cglb_amd.backend import interface as backend
    from cglb_amd.data import synthetic_problem
    backend.set_default_float("fp64")
    backend.set_default_jitter(1e-6)
    X, y, _Z = synthetic_problem(N_B + 9, D_B, M_B, seed=5, P=columns)
    kernel = config.Matern32Config()
    cfg = config.GPRConfig(kernel) if name == "gpr" else config.SGPR_CONFIGS[name](kernel=kernel, inducing_variable=config.InducingVariableConfig(M_B))
    return backend.create_model(cfg, (X[:N_B], y[:N_B])), torch.as_tensor(X[N_B:], dtype=torch.float64)


@pytest.mark.parametrize("name", ["cglb", "cglbn2m", "cglbnm2", "sgpr", "sgprn2m", "gpr"])
def test_backend_classes(name):
    from cglb_amd.backend import models
    model, xs = _model(name)
    hip = model.hip
    if name == "gpr":
        pred, plain = models.PredictGradGPR(model), models.PredictGPR(model)
    elif name.startswith("sgpr"):
        pred, plain = models.PredictGradSGPR(model), models.PredictSGPR(model)
    else:
        pred, plain = models.PredictGradCG(model), models.PredictCG(model)
    mean, dmean, var, dvar = pred(xs)
    assert mean.shape == (9, 1) and var.shape == (9, 1) and dmean.shape == (9, D_B) and dvar.shape == (9, D_B)
    # against the context calls at the same state
    if name == "gpr":
        want = hip.gpr_predict_grad(xs)
    else:
        want = hip.predict_grad(pred.v_vec.reshape(-1) if name.startswith("cglb") else model._zero_v, xs)
    for got, w in zip((mean, dmean, var, dvar), want):
        assert torch.equal(got.reshape(w.shape), w)
    pm, pv = plain(xs)
    assert torch.equal(pm, mean) and torch.equal(pv, var)                     # the value predictor's numbers
    # autograd through mean_and_variance: the upper confidence bound mean + 2 sqrt(var)
    x = xs.clone().requires_grad_(True)
    m, s2 = pred.mean_and_variance(x)
    assert torch.equal(m.detach(), mean) and torch.equal(s2.detach(), var)
    (m + 2.0 * torch.sqrt(s2)).sum().backward()
    hand = dmean.cpu() + dvar.cpu() / torch.sqrt(var.cpu())
    assert x.grad.shape == xs.shape
    assert float((x.grad - hand).abs().max()) <= 8 * 2.0 ** -53 * float(hand.abs().max() + dmean.abs().max().cpu() + (dvar.cpu() / torch.sqrt(var.cpu())).abs().max())
    m0, v0 = pred.mean_and_variance(xs)                                       # without requires_grad: plain tensors
    assert not m0.requires_grad and torch.equal(m0, mean) and torch.equal(v0, var)


def test_backend_refusals():
    from cglb_amd.backend import models
    cglb, _ = _model("cglb")
    sgpr, _ = _model("sgpr")
    gpr, _ = _model("gpr")
    for cls, wrong in ((models.PredictGradCG, sgpr), (models.PredictGradCG, gpr), (models.PredictGradSGPR, cglb), (models.PredictGradSGPR, gpr),
                       (models.PredictGradGPR, cglb), (models.PredictGradGPR, sgpr)):
        with pytest.raises(ValueError, match="model expected"):
            cls(wrong)
    two, _ = _model("cglb", columns=2)
    with pytest.raises(NotImplementedError, match="more than one target column"):
        models.PredictGradCG(two)
    cglb.hip.world = 2            # what a rank of a row-sharded context reports
    try:
        with pytest.raises(NotImplementedError, match="more than one rank"):
            models.PredictGradCG(cglb)
    finally:
        cglb.hip.world = 1


# ---- 5. refusals of the library ---------------------------------------------------------------------------------------------------------------
def _ctx(X, y, M, kind="rbf", dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    D = X.shape[1]
    ctx = HipContext(X, y, M, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(np.full(D, 1.3), 1.1, 0.2, 0.1, X[:M].copy(), 1e-6)
    return ctx


def test_refusals():
    N, D, M = 65, 3, 8
    X, y = gpr_ref.problem(N, D)

    def each(ctx, xs, match, n=N):
        for call in (lambda: ctx.cross_grad_weighted(xs, np.ones(n)), lambda: ctx.predict_grad(np.zeros(n), xs), lambda: ctx.time_predict_grad(3, True, 1)):
            with pytest.raises(ValueError, match=match):
                call()

    ctx = _ctx(X, y, M, dtype=torch.float32)
    try:
        ctx.setup()
        each(ctx, X[:3], "-t fp64")
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.gpr_predict_grad(X[:3])
    finally:
        ctx.close()
    Xw, yw = gpr_ref.problem(N, 33)
    ctx = _ctx(Xw, yw, M)
    try:
        ctx.setup()
        each(ctx, Xw[:3], "no wide path yet")
        ctx.gpr_set_hypers(np.full(33, 2.0), 1.0, 0.1, 0.0)
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.gpr_predict_grad(Xw[:3])
    finally:
        ctx.close()
    ctx = _ctx(X, y, M)
    try:
        ctx.setup()
        v = np.linspace(-1, 1, N)
        good = _np(ctx.predict_grad(v, X[:5])) + _np(ctx.cross_grad_weighted(X[:5], np.ones(M), np.ones((M, 8)), "inducing"))
        ctx.set_targets(np.stack([y, -y], axis=1))
        each(ctx, X[:3], "one target column")
        ctx.set_targets(y)
        from cglb_amd import _lib
        from ctypes import c_void_p
        xs = ctx._xnew(X[:3])
        o = _nan(ctx, 3)
        p = lambda t: c_void_p(t.data_ptr())
        rc = ctx.lib.cglb_cross_grad_weighted(ctx._ctx, 0, p(xs), 3, None, None, 0, None, None, None, None)          # u and Wt both NULL
        assert rc == _lib.ERR_BAD_ARG
        with pytest.raises(ValueError, match="at least one of the weights"):
            _lib.check(rc, ctx._ctx)
        u = ctx._dev(np.ones(N), N)
        rc = ctx.lib.cglb_cross_grad_weighted(ctx._ctx, 0, p(xs), 3, p(u), None, 0, None, None, p(o), None)          # an output of the absent Wt
        with pytest.raises(ValueError, match="absent weight"):
            _lib.check(rc, ctx._ctx)
        assert bool(torch.isnan(o).all())
        ctx.set_hypers(np.full(D, 1.3), 1.1, 0.2, 0.1, X[:M].copy(), 1e-6)
        ctx.setup()
        again = _np(ctx.predict_grad(v, X[:5])) + _np(ctx.cross_grad_weighted(X[:5], np.ones(M), np.ones((M, 8)), "inducing"))
        for a, b in zip(good, again):
            assert np.array_equal(a, b)                                         # the context still answers, bitwise as before
        assert ctx.time_predict_grad(5, True, 1) > 0 and ctx.time_predict_grad(5, False, 1) > 0
        assert ctx.get_stat("predict_grad_kernel_ms") > 0
    finally:
        ctx.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------------
def test_the_new_calls_leave_the_neighbours_alone():
    N, D, M = 130, 3, 33
    X, y = gpr_ref.problem(N, D)
    xs = X[:17] + 0.25

    def run(with_new_calls):
        ctx = _ctx(X, y, M, "matern32")
        out = []
        try:
            v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
            ctx.gpr_set_hypers(np.full(D, 1.3), 1.1, 0.2, 0.1)
            for _ in range(2):
                r = ctx.objective_and_grad(v, True, 1e-3, 100, 40)
                out += [np.array([r.bound, r.upper, r.lower]), r.grad["lengthscales"], r.grad["Z"], v.cpu().numpy().copy()]
                out += _np(ctx.predict(v, xs))
                out += _np(ctx.gpr_predict(xs))
                if with_new_calls:
                    ctx.predict_grad(v, xs)
                    ctx.predict_grad(v, xs, with_var=False)
                    ctx.gpr_predict_grad(xs)
                    ctx.cross_grad_weighted(xs, np.ones(N), np.ones((N, 17)))
                    ctx.cross_grad_weighted(xs, np.ones(M), None, "inducing")
                    ctx.time_predict_grad(9, True, 1)
                out += _np(ctx.predict(v, xs))
                out += _np(ctx.gpr_predict(xs))
                out.append(v.cpu().numpy().copy())
        finally:
            ctx.close()
        return out

    with_calls, plain = run(True), run(False)
    assert len(with_calls) == len(plain)
    for got, want in zip(with_calls, plain):
        assert np.array_equal(got, want)
