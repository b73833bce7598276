"""Input gradients of the CGLB / SGPR / exact-GP predictive at mid widths (33 - 96 input dimensions) behind the option "input_grad_mid"
(csrc/kernels_predict_grad_mid.hip): cglb_cross_grad_weighted, cglb_predict_grad, cglb_time_predict_grad, cglb_gpr_predict_grad,
`PredictGradCG` / `PredictGradSGPR` / `PredictGradGPR(wide=True)`, against tests/predict_grad_ref.py at the cells, cases and tolerances of
tests/predict_grad_mid_ref.py.  Small shapes; every output is pre-filled with NaN.

1. The option: a D = 33 context reports "predict_grad_native" 0 and refuses; with the option on it reports 1 and every entry returns finite values;
   off again it refuses again.
2. The row-weighted product, every element against the longdouble reference: predict_grad_mid_ref.product_cells (D in 33, 48, 49, 64, 65, 80, 81, 96;
   n_new in 1, 2, 63, 64, 65 and 4097 once; 1, 65, 300 points; both point sets; kff_jsplit 1, 3, 7; the three kinds; precision levels 0 and 1, 2 on
   one cell per kind; ldw > n_new with NaN in the padding columns).  u-only, Wt-only and both bitwise equal where they overlap, a second run and
   the gradients alone bitwise equal; the lone coincident pair has gradient exactly 0.0; the point at 10^3 stays within the clamp floor.
3. Single kernel values: the sets F40, F64, F77, F90 of tests/kernel_value_cases.py and their axis variants, read through u = e_m and a
   shifted-diagonal Wt, under the bounds of the mid-width input-gradient path (c = 19: predict_grad_mid_ref.VALUE_ENTRY).
4. cglb_predict_grad at (N, D, M) = (300, 40, 33) and (300, 77, 33), the three kinds, quad_term 0 and 1 (v full of NaN at 1), n_new 1 and 65, 4097
   once: f_mean / f_var bitwise cglb_predict's, gradients against fp64 autograd and against the analytic form, with_var False bitwise the same
   mean outputs.  cglb_gpr_predict_grad at (300, 40) and (300, 77): bitwise values, gradients against the dense autograd reference.
5. The backend classes with wide=True: shapes, backpropagation through mean_and_variance; without it they raise as before.
6. Neighbours: D = 97, wide_reg 0, fp32 and two target columns stay refused with the option on; a narrow context is bitwise unchanged by the option;
   cglb_predict and objective_and_grad are bitwise the same before and after a predict_grad call; after set_hypers with new lengthscales predict_grad
   is bitwise that of a fresh context (the inducing-point operand is refreshed).
"""
import numpy as np
import pytest
import torch

import gpr_ref
import input_grad_mid_ref as igm
import input_grad_ref as ig
import kernel_value_cases as kv
import predict_grad_mid_ref as pgm
import predict_grad_ref as pg
import predict_ref as pr

pytestmark = pytest.mark.gpu
NAN = float("nan")
CELLS = pgm.product_cells()


def _nan(ctx, *shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=ctx.device)


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _context(X, y, Z, kind, h, mid=True, dtype=torch.float64, options=(), jitter=1e-6):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, len(Z), kind, dtype=dtype, device=torch.device("cuda", 0))
    try:
        for k, v in options:
            ctx.set_option(k, v)
        if mid:
            ctx.set_option("input_grad_mid", 1)
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, jitter)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _hypers(hyp):
    return dict(lengthscales=np.asarray(hyp.lengthscales, dtype=np.float64), variance=hyp.variance, noise=hyp.noise, mean=hyp.mean)


# ---- 1. the option ------------------------------------------------------------------------------------------------------------------------------
def test_the_option_opens_the_mid_width_path():
    N, D, M = 65, 33, 8
    X, y = gpr_ref.problem(N, D)
    h = dict(lengthscales=np.full(D, 6.0), variance=1.1, noise=0.2, mean=0.1)
    ctx = _context(X, y, X[:M].copy(), "rbf", h, mid=False)
    xs = X[:3] + 0.25
    calls = (lambda: ctx.cross_grad_weighted(xs, np.ones(N), np.ones((N, 8))), lambda: ctx.cross_grad_weighted(xs, np.ones(M), None, "inducing"),
             lambda: ctx.predict_grad(np.zeros(N), xs), lambda: ctx.time_predict_grad(3, True, 1), lambda: ctx.gpr_predict_grad(xs))
    try:
        ctx.setup()
        ctx.gpr_set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"])
        for state in (0, 1, 0):
            ctx.set_option("input_grad_mid", state)
            assert ctx.get_stat("predict_grad_native") == float(state)
            for call in calls:
                if state:
                    res = call()
                    for t in (res if isinstance(res, tuple) else ()):
                        assert t is None or bool(torch.isfinite(t).all())
                    assert not isinstance(res, float) or res > 0.0
                else:
                    with pytest.raises(ValueError, match="no wide path yet"):
                        call()
            if state:
                assert ctx.get_stat("predict_grad_kernel_ms") > 0
    finally:
        ctx.close()


# ---- 2. the product, cell by cell -----------------------------------------------------------------------------------------------------------------
def _check_cell(c, precision):
    X, y, Z, h, xnew, u, Wt = pgm.cell_problem(c)
    P = X if c["set"] == "train" else Z
    n, D, kind, ps = c["n_new"], c["D"], c["kind"], c["set"]
    ls, f = h["lengthscales"], h["variance"]
    ctx = _context(X, y, Z, kind, h, options=(("precision", precision), ("kff_jsplit", c["jsplit"])))
    try:
        assert ctx.get_stat("predict_grad_native") == 1.0
        outs = lambda: dict(out_u=_nan(ctx, n), gout_u=_nan(ctx, n, D), out_w=_nan(ctx, n), gout_w=_nan(ctx, n, D))
        both = _np(ctx.cross_grad_weighted(xnew, u, Wt, ps, **outs()))
        again = _np(ctx.cross_grad_weighted(xnew, u, Wt, ps, **outs()))
        only_u = _np(ctx.cross_grad_weighted(xnew, u, None, ps, out_u=_nan(ctx, n), gout_u=_nan(ctx, n, D)))
        only_w = _np(ctx.cross_grad_weighted(xnew, None, Wt, ps, out_w=_nan(ctx, n), gout_w=_nan(ctx, n, D)))
        grads = _np(ctx.cross_grad_weighted(xnew, u, Wt, ps, gout_u=_nan(ctx, n, D), gout_w=_nan(ctx, n, D), with_value=False))
        # the coincident pair alone: new point 0 sits on point j0 of the set; every other weight zero
        j0 = min(3, len(P) - 1)
        u1, W1 = np.zeros(len(P)), np.zeros((len(P), n))
        u1[j0], W1[j0, 0] = 1.5, -2.5
        lone = _np(ctx.cross_grad_weighted(xnew, u1, W1, ps))
    finally:
        ctx.close()
    want = pg.weighted_product(kind, xnew, P, ls, f, u, Wt)
    tol = pgm.level_tolerance(kind, xnew, P, ls, f, u, Wt, precision)
    worst = []
    for got, w, t in zip(both, want, tol):
        assert got.shape == w.shape and np.all(np.isfinite(got))
        worst.append(float((np.abs(got - w) / t).max()))
    print(f"{pgm.cell_id(c)} precision {precision}: out_u {worst[0]:.2e}, gout_u {worst[1]:.2e}, out_w {worst[2]:.2e}, gout_w {worst[3]:.2e} of the tolerance")
    assert max(worst) <= 1.0
    for a, b in zip(both, again):
        assert np.array_equal(a, b)
    assert np.array_equal(only_u[0], both[0]) and np.array_equal(only_u[1], both[1]) and only_u[2] is None and only_u[3] is None
    assert np.array_equal(only_w[2], both[2]) and np.array_equal(only_w[3], both[3]) and only_w[0] is None and only_w[1] is None
    assert grads[0] is None and grads[2] is None and np.array_equal(grads[1], both[1]) and np.array_equal(grads[3], both[3])
    assert np.all(lone[1][0] == 0.0) and np.all(lone[3][0] == 0.0)            # exactly zero, not merely small
    rel = ig.TOL + (igm.LEVEL2_KERNEL_ERROR if precision == 2 else 0.0)      # the product rule on one pair, with the level term at level 2
    assert abs(lone[0][0] - 1.5 * f) <= rel * 1.5 * f and abs(lone[2][0] + 2.5 * f) <= rel * 2.5 * f
    if n > 1:   # the point at 10^3: the kernel values underflow; the range-clamped 2^x leaves at most its floor (the floor term of the tolerance alone)
        fu, fw = ig.FLOOR * f * np.abs(u).sum(), ig.FLOOR * f * np.abs(Wt[:, 1]).sum()
        assert abs(both[0][1]) <= fu and np.all(np.abs(both[1][1]) <= fu) and abs(both[2][1]) <= fw and np.all(np.abs(both[3][1]) <= fw)


@pytest.mark.parametrize("c", CELLS, ids=pgm.cell_id)
def test_product_matches_the_reference(c):
    _check_cell(c, c["precision"])


@pytest.mark.parametrize("x", pgm.PRECISION_CELLS, ids=lambda x: pgm.cell_id(CELLS[x]))
def test_product_at_precision_level_2(x):
    _check_cell(CELLS[x], 2)


# ---- 3. single kernel values ------------------------------------------------------------------------------------------------------------------------
VALUE_ROWS = [c for c in kv.case_table() if c.name in pgm.VALUE_SETS]
VALUE_CASES = [v for c in VALUE_ROWS for v in [c] + kv.axis_variants(c)]


@pytest.mark.parametrize("case", VALUE_CASES, ids=[kv.case_id(c) for c in VALUE_CASES])
def test_single_kernel_values(case):
    """weighted_grad_mid_kernel pair by pair, point set "train": u = e_m for every m (out_u / gout_u are column m) and Wt[m, i] = 1 where
    m == (i + shift) % N, shift = 0 .. N - 1, with ldw = n_new + 3 and NaN in the spare columns, both weights in one call; then each alone, bitwise
    the same.  Value and gradient under the bounds tests/test_gpu_kernel_values.py holds cross_grad_mid_kernel to, with its helpers."""
    import test_gpu_kernel_values as tkv
    prec = 1
    xnew = kv.new_points(case)
    ctx, _clamp, _bias = tkv._context(case, {"precision": prec, "input_grad_mid": 1, "wide_reg": 1})
    try:
        assert int(ctx.get_stat("predict_grad_native")) == 1
        N, n, D = ctx.N, xnew.shape[0], ctx.D
        u = torch.zeros(N, dtype=torch.float64, device=ctx.device)
        Wt = _nan(ctx, N, n + 3)
        cols = torch.arange(n, device=ctx.device)

        def run(which):
            Ku, Gu, Kw, Gw = np.full((n, N), np.nan), np.full((n, N, D), np.nan), np.full((n, N), np.nan), np.full((n, N, D), np.nan)
            for m in range(N):
                u[m] = 1.0
                Wt[:, :n] = 0.0
                tgt = (cols + m) % N
                Wt[tgt, cols] = 1.0
                kw = {}
                if which != "w":
                    kw.update(u=u, out_u=_nan(ctx, n), gout_u=_nan(ctx, n, D))
                if which != "u":
                    kw.update(Wt=Wt, out_w=_nan(ctx, n), gout_w=_nan(ctx, n, D))
                ou, gu, ow, gw = ctx.cross_grad_weighted(xnew, **kw)
                u[m] = 0.0
                if which != "w":
                    Ku[:, m], Gu[:, m] = ou.cpu().numpy(), gu.cpu().numpy()
                if which != "u":
                    t = tgt.cpu().numpy()
                    Kw[np.arange(n), t], Gw[np.arange(n), t] = ow.cpu().numpy(), gw.cpu().numpy()
            return Ku, Gu, Kw, Gw

        both, ua, wa = run("both"), run("u"), run("w")
    finally:
        ctx.close()
    assert np.array_equal(both[0], ua[0], equal_nan=True) and np.array_equal(both[1], ua[1], equal_nan=True)
    assert np.array_equal(both[2], wa[2], equal_nan=True) and np.array_equal(both[3], wa[3], equal_nan=True)
    worst = max(tkv._compare_grad(case, "cross_grad_weighted mid u", pgm.VALUE_ENTRY, prec, both[0], both[1], xnew),
                tkv._compare_grad(case, "cross_grad_weighted mid Wt", pgm.VALUE_ENTRY, prec, both[2], both[3], xnew))
    print(f"{kv.case_id(case)}: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0


# ---- 4. the predictors ----------------------------------------------------------------------------------------------------------------------------
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
    X, y, hyp, v = pgm.problem(case)
    xn = pgm.xnew(case)
    n, D = case.n_new, case.D
    ctx = _context(X, y, hyp.Z, case.kind, _hypers(hyp), jitter=hyp.jitter)
    try:
        for q in (0, 1):
            ctx.set_option("logdet_bound", q)      # quad_term 1 with the NM^2 bound: the SGPR class, as tests/test_gpu_predict_grad.py sets it
            ctx.set_option("quad_term", q)
            ctx.setup()
            vq = np.full(case.N, NAN) if q else v
            mean, var = pr.predict(ctx, vq, xn)
            outs = _np(ctx.predict_grad(vq, xn, f_mean=_nan(ctx, n), g_mean=_nan(ctx, n, D), f_var=_nan(ctx, n), g_var=_nan(ctx, n, D)))
            assert np.array_equal(outs[0], mean) and np.array_equal(outs[2], var)       # bitwise cglb_predict
            _check_grad(case, hyp, outs, pgm.cglb_reference(case, q), f"quad_term {q} autograd")
            _check_grad(case, hyp, outs, pgm.cglb_analytic(case, q), f"quad_term {q} analytic")
            m2, g2, v2, gv2 = _np(ctx.predict_grad(vq, xn, with_var=False, f_mean=_nan(ctx, n), g_mean=_nan(ctx, n, D)))
            assert v2 is None and gv2 is None and np.array_equal(m2, outs[0]) and np.array_equal(g2, outs[1])
    finally:
        ctx.close()


@pytest.mark.parametrize("case", pgm.CGLB_CASES, ids=lambda c: c.id)
def test_cglb_predict_grad(case):
    _run_cglb_case(case)


def test_cglb_predict_grad_beyond_one_launch():
    _run_cglb_case(pgm.LARGE_CASE)


@pytest.mark.parametrize("case", pgm.GPR_CASES, ids=lambda c: c.id)
def test_gpr_predict_grad(case):
    X, y, hyp, _ = pgm.problem(case)
    xn = pgm.xnew(case)
    n, D = case.n_new, case.D
    ctx = _context(X, y, X[:1].copy(), case.kind, _hypers(hyp))
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
    _check_grad(case, hyp, outs, pgm.gpr_reference(case), "gpr")


# ---- 5. the backend -------------------------------------------------------------------------------------------------------------------------
N_B, D_B, M_B = 160, 40, 16


def _model(name):
    from cglb_amd.backend import config
    from cglb_amd.backend import interface as backend
    from cglb_amd.data import synthetic_problem
    backend.set_default_float("fp64")
    backend.set_default_jitter(1e-6)
    X, y, _Z = synthetic_problem(N_B + 9, D_B, M_B, seed=5)
    kernel = config.Matern32Config()
    cfg = config.GPRConfig(kernel) if name == "gpr" else config.SGPR_CONFIGS[name](kernel=kernel, inducing_variable=config.InducingVariableConfig(M_B))
    return backend.create_model(cfg, (X[:N_B], y[:N_B])), torch.as_tensor(X[N_B:], dtype=torch.float64)


@pytest.mark.parametrize("name", ["cglb", "sgpr", "gpr"])
def test_backend_classes_wide(name):
    from cglb_amd.backend import models
    model, xs = _model(name)
    cls = {"cglb": models.PredictGradCG, "sgpr": models.PredictGradSGPR, "gpr": models.PredictGradGPR}[name]
    with pytest.raises(ValueError, match="no wide path yet"):      # without wide=True: as before
        cls(model)(xs)
    pred = cls(model, wide=True)
    assert model.hip.get_stat("predict_grad_native") == 1.0
    mean, dmean, var, dvar = pred(xs)
    assert mean.shape == (9, 1) and var.shape == (9, 1) and dmean.shape == (9, D_B) and dvar.shape == (9, D_B)
    for t in (mean, dmean, var, dvar):
        assert bool(torch.isfinite(t).all())
    x = xs.clone().requires_grad_(True)
    m, s2 = pred.mean_and_variance(x)
    assert torch.equal(m.detach(), mean) and torch.equal(s2.detach(), var)
    (m + 2.0 * torch.sqrt(s2)).sum().backward()
    hand = dmean.cpu() + dvar.cpu() / torch.sqrt(var.cpu())
    assert x.grad.shape == xs.shape
    assert float((x.grad - hand).abs().max()) <= 8 * 2.0 ** -53 * float(hand.abs().max() + dmean.abs().max().cpu() + (dvar.cpu() / torch.sqrt(var.cpu())).abs().max())


# ---- 6. neighbours ----------------------------------------------------------------------------------------------------------------------------------
def _plain_problem(N, D, M):
    X, y = gpr_ref.problem(N, D)
    return X, y, X[:M].copy(), dict(lengthscales=np.full(D, 0.9 * np.sqrt(D)), variance=1.1, noise=0.2, mean=0.1)


def test_neighbouring_scope():
    N, M = 65, 8

    def each(ctx, xs, match):
        for call in (lambda: ctx.cross_grad_weighted(xs, np.ones(N)), lambda: ctx.predict_grad(np.zeros(N), xs), lambda: ctx.time_predict_grad(3, True, 1)):
            with pytest.raises(ValueError, match=match):
                call()

    X, y, Z, h = _plain_problem(N, 97, M)
    ctx = _context(X, y, Z, "rbf", h)
    try:
        ctx.setup()
        ctx.gpr_set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"])
        assert ctx.get_stat("predict_grad_native") == 0.0
        each(ctx, X[:3], "no wide path yet")
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.gpr_predict_grad(X[:3])
    finally:
        ctx.close()
    X, y, Z, h = _plain_problem(N, 40, M)
    ctx = _context(X, y, Z, "rbf", h, options=(("wide_reg", 0),))
    try:
        ctx.setup()
        assert ctx.get_stat("predict_grad_native") == 0.0
        each(ctx, X[:3], "no wide path yet")
    finally:
        ctx.close()
    ctx = _context(X, y, Z, "rbf", h, dtype=torch.float32)
    try:
        ctx.setup()
        assert ctx.get_stat("predict_grad_native") == 0.0
        each(ctx, X[:3], "-t fp64")
    finally:
        ctx.close()
    ctx = _context(X, y, Z, "rbf", h)
    try:
        ctx.setup()
        ctx.set_targets(np.stack([y, -y], axis=1))
        assert ctx.get_stat("predict_grad_native") == 0.0
        each(ctx, X[:3], "one target column")
    finally:
        ctx.close()
    # a narrow context: the option changes nothing, bit for bit
    X, y, Z, h = _plain_problem(N, 20, M)
    got = {}
    for mid in (False, True):
        ctx = _context(X, y, Z, "matern52", h, mid=mid)
        try:
            ctx.setup()
            ctx.gpr_set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"])
            assert ctx.get_stat("predict_grad_native") == 1.0
            got[mid] = (_np(ctx.predict_grad(np.linspace(-1, 1, N), X[:5] + 0.1)) + _np(ctx.cross_grad_weighted(X[:5], np.ones(M), np.ones((M, 8)), "inducing"))
                        + _np(ctx.gpr_predict_grad(X[:5] + 0.1)))
        finally:
            ctx.close()
    for p, q in zip(got[False], got[True]):
        assert np.array_equal(p, q)


def test_the_new_calls_leave_the_neighbours_alone():
    N, D, M = 130, 40, 33
    X, y, Z, h = _plain_problem(N, D, M)
    xs = X[:17] + 0.25

    def run(with_new_calls):
        ctx = _context(X, y, Z, "matern32", h)
        out = []
        try:
            v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
            ctx.gpr_set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"])
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
        assert np.array_equal(np.asarray(got), np.asarray(want))


def test_set_hypers_refreshes_the_inducing_operand():
    N, D, M = 130, 77, 33
    X, y, Z, h = _plain_problem(N, D, M)
    h2 = dict(h, lengthscales=h["lengthscales"] * np.linspace(0.8, 1.3, D))
    xs = np.concatenate([X[:5], Z[:3], X[40:49] + 0.25])
    v = np.linspace(-0.1, 0.1, N)

    def answers(ctx):
        ctx.setup()
        return _np(ctx.predict_grad(v, xs)) + _np(ctx.cross_grad_weighted(xs, np.ones(M), np.ones((M, 24)), "inducing"))

    ctx = _context(X, y, Z, "matern52", h)
    try:
        first = answers(ctx)
        ctx.set_hypers(h2["lengthscales"], h2["variance"], h2["noise"], h2["mean"], Z, 1e-6)
        moved = answers(ctx)
    finally:
        ctx.close()
    fresh_ctx = _context(X, y, Z, "matern52", h2)
    try:
        fresh = answers(fresh_ctx)
    finally:
        fresh_ctx.close()
    assert not np.array_equal(first[1], moved[1])
    for a, b in zip(moved, fresh):
        assert np.array_equal(a, b)
