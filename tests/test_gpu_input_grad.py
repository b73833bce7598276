"""Input gradients of the iterative exact-GP class (cglb_cross_grad_matmat, cglb_feature_grad_matmat, cglb_itergp_predict_grad,
cglb_itergp_paths_solve / _eval, `PredictGradIterGPR`, `PathsIterGPR`) against the dense longdouble restatement tests/input_grad_ref.py.
Small shapes; every output is pre-filled with NaN.

1. The two products, every element: the covering table input_grad_ref.product_cells (padded-width classes D in 1, 3, 8, 9, 20, 32 with the
   rows per lane and group width the restated rule gives; n_new in 1, 2, B - 1, B, B + 1; N in 1, 65, 300; kff_jsplit forced to 1, 3, 7;
   S in 1, g, g + 1, 9; F in 1, 65; the three kinds).  New points: a training row first (its own pair adds exactly zero to the gradient), a point at
   10^3 second (kernel value and gradient underflow, the features stay finite), the rest random; one duplicated training row.
   Tolerances (input_grad_ref): 1e-11 of f sum_j |h delta_k / l_k V| per gradient element and of f sum_j |kappa V| per value - the figure
   tests/test_gpu_cross_matmat.py holds the same kernel values to (tests/kernel_value_cases.py holds the derivative factor of cglb_grad_kff_multi to its evaluator's
   level, <= 1e-13 relative, plus operand roundings: tighter than 1e-11 at these shapes, so 1e-11 stands) - plus that file's floor; the feature product's derived bound.  A second call is bitwise equal; with out NULL the gradient is
   bitwise the same.
2. cglb_itergp_predict_grad at sample_ref.SAMPLE_CASES[:4] with the rank-8 and rank-33 caches: mean and variance bitwise those of
   cglb_itergp_predict_cached; g_mean re-assembled from the library's own alpha to the product tolerance, and within
   sqrt(C f) / l_k sqrt(2 max_error) of the dense gradient at max_error 1e-12 and 1e-3; g_var against -2 sum B G of the restatement at
   love_ref's cache to 1e-10 f sqrt(C) / l_k; CGLB_ERR_STATE without a cache.
3. Paths: the solves and (without gradients) the values are bitwise those of cglb_itergp_sample; with gradients the values are within 1e-10
   of max(|f|, sqrt f) and the gradients within the sum of the two product tolerances at the library's U; evaluating runs no solve.
4. `PathsIterGPR`, `PredictGradIterGPR`; the refusals; the neighbours' state is left alone.
"""
import functools
import math

import numpy as np
import pytest
import torch

import gpr_ref as ref
import input_grad_ref as ig
import sample_ref as sr

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _context(X, y, kind, h, k=1, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)   # Z is a placeholder: the class selects its own
    return ctx


def _nan(ctx, *shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=ctx.device)


# ---- 1. the two products ----------------------------------------------------------------------------------------------------------------
CELLS = ig.product_cells()


def test_the_cells_reach_every_instance_class():
    reached = {(ig.rows_per_lane(c["D"]), ig.group_width(c["D"])) for c in CELLS}
    assert reached == set(ig.CLASSES) == {(2, 8), (1, 8), (1, 4), (1, 2)}
    for c in CELLS:
        assert c["n_new"] in ig.row_counts(c["D"]) or c["n_new"] == 2
        assert c["S"] in ig.s_values(c["D"])


@pytest.mark.parametrize("c", CELLS, ids=ig.cell_id)
def test_products_match_the_restatement(c):
    X, y, xnew, V, omega, b, W = ig.cell_problem(c)
    h = ig.cell_hypers(c["D"])
    ls, f, n, S, D = h["lengthscales"], h["variance"], c["n_new"], c["S"], c["D"]
    ctx = _context(X, y, c["kind"], h)
    try:
        ctx.set_option("kff_jsplit", c["jsplit"])
        out, g = ctx.cross_grad_matmat(xnew, V, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        out2, g2 = ctx.cross_grad_matmat(xnew, V, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        none, g3 = ctx.cross_grad_matmat(xnew, V, gout=_nan(ctx, n, S, D), with_value=False)
        fo, fg = ctx.feature_grad_matmat(xnew, omega, b, W, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        fo2, fg2 = ctx.feature_grad_matmat(xnew, omega, b, W, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        fnone, fg3 = ctx.feature_grad_matmat(xnew, omega, b, W, gout=_nan(ctx, n, S, D), with_value=False)
        value_kernel = ctx.cross_matmat(xnew, V).cpu().numpy()
        out, g, out2, g2, g3, fo, fg, fo2, fg2, fg3 = [t.cpu().numpy() for t in (out, g, out2, g2, g3, fo, fg, fo2, fg2, fg3)]
    finally:
        ctx.close()
    # the cross product
    want_o, want_g = ig.cross_grad(c["kind"], xnew, X, ls, f, V)
    tv, tg = ig.cross_tolerance(c["kind"], xnew, X, ls, f, V)
    eo, eg = np.abs(out - want_o) / tv, np.abs(g - want_g) / tg
    print(f"{ig.cell_id(c)}: cross value {float(eo.max()):.2e}, gradient {float(eg.max()):.2e} of the tolerance")
    assert out.shape == (n, S) and g.shape == (n, S, D) and np.all(np.isfinite(out)) and np.all(np.isfinite(g))
    assert float(eo.max()) <= 1.0 and float(eg.max()) <= 1.0
    assert np.array_equal(out, out2) and np.array_equal(g, g2) and np.array_equal(g, g3) and none is None
    assert np.all(np.abs(out - value_kernel) <= 2 * tv)                     # the Gram-chain kernel's values, each within the same tolerance
    floor = ig.FLOOR * f * np.abs(V).sum(axis=0)
    if c["N"] == 1:
        assert np.all(g[0] == 0.0)                                          # the coincident pair alone: exactly zero
    if n > 1:
        assert np.all(np.abs(out[1]) <= floor) and np.all(np.abs(g[1]) <= floor[:, None])   # the point at 10^3: everything underflows
    # the feature product
    cen = sr.centre(X)
    want_o, want_g = ig.feature_grad(xnew, cen, ls, f, omega, b, W)
    tv, tg = ig.feature_tolerance(xnew, cen, ls, f, omega, b, W)
    eo, eg = np.abs(fo - want_o) / tv, np.abs(fg - want_g) / tg
    print(f"{ig.cell_id(c)}: feature value {float(eo.max()):.2e}, gradient {float(eg.max()):.2e} of the tolerance")
    assert np.all(np.isfinite(fo)) and np.all(np.isfinite(fg))
    assert float(eo.max()) <= 1.0 and float(eg.max()) <= 1.0
    assert np.array_equal(fo, fo2) and np.array_equal(fg, fg2) and np.array_equal(fg, fg3) and fnone is None


def test_out_tensors_are_checked():
    X, y = ref.problem(65, 3)
    ctx = _context(X, y, "rbf", ig.cell_hypers(3))
    try:
        V = np.ones((65, 2))
        with pytest.raises(ValueError, match="gout"):
            ctx.cross_grad_matmat(X[:4], V, gout=torch.zeros((4, 3, 2), dtype=torch.float64, device=ctx.device))
        with pytest.raises(ValueError, match="out"):
            ctx.cross_grad_matmat(X[:4], V, out=torch.zeros((4, 2), dtype=torch.float32, device=ctx.device))
    finally:
        ctx.close()


# ---- 2. the predictive and its gradients -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_predict(case, rank):
    N, D, kind, _k = case
    X, y = ref.problem(N, D)
    xnew = sr.sample_new_points(X, ig.PREDICT_NEW)
    out = ig.predict_grad(kind, X, y, sr.sample_hypers(D), xnew, rank=rank)
    for a in out:
        a.setflags(write=False)
    return X, y, xnew, out


@pytest.mark.parametrize("rank", ig.PREDICT_RANKS)
@pytest.mark.parametrize("case", ig.PREDICT_CASES, ids=lambda c: "N%d_D%d_%s" % c[:3])
def test_predict_grad(case, rank):
    N, D, kind, k = case
    h = sr.sample_hypers(D)
    ls, f = np.asarray(h["lengthscales"], dtype=np.float64), h["variance"]
    X, y, xnew, (d_mean, d_gmean, d_var, d_gvar) = _dense_predict(case, rank)
    a, b = _context(X, y, kind, h, k), _context(X, y, kind, h, k)     # two contexts in the same state
    try:
        with pytest.raises(RuntimeError, match="call order"):
            b.itergp_predict_grad(xnew)                                 # no cache yet
        assert a.itergp_var_cache(rank) == b.itergp_var_cache(rank)
        res = {}
        for max_error in (1e-3, 1e-12):                                 # the second solve is warm-started at the first alpha in both contexts
            m_a, v_a = a.itergp_predict_cached(xnew, max_error=max_error)
            res[max_error] = [t.cpu().numpy() for t in b.itergp_predict_grad(xnew, max_error=max_error)] + [b.get_matrix("alpha").cpu().numpy()]
            assert np.array_equal(m_a.cpu().numpy(), res[max_error][0]) and np.array_equal(v_a.cpu().numpy(), res[max_error][2])
        mean_only = b.itergp_predict_grad(xnew, max_error=1e-12, with_var=False)
        assert mean_only[2] is None and mean_only[3] is None
        assert np.array_equal(mean_only[0].cpu().numpy(), res[1e-12][0]) and np.array_equal(mean_only[1].cpu().numpy(), res[1e-12][1])
        assert int(b.get_stat("itergp_cache_request")) == rank          # the cache is still valid
    finally:
        a.close()
        b.close()
    for max_error, (mean, gmean, var, gvar, alpha) in res.items():
        assert gmean.shape == (len(xnew), D) and gvar.shape == (len(xnew), D) and np.all(np.isfinite(gmean)) and np.all(np.isfinite(gvar))
        # re-assembled from the library's own alpha
        _o, want = ig.cross_grad(kind, xnew, X, ls, f, alpha.reshape(-1, 1))
        tol = ig.cross_tolerance(kind, xnew, X, ls, f, alpha.reshape(-1, 1))[1][:, 0, :]
        e1 = float((np.abs(gmean - want[:, 0, :]) / tol).max())
        # against the dense gradient: the solve bound
        bound = ig.solve_bound(kind, ls, f, max_error)[None, :] + tol
        e2 = float((np.abs(gmean - d_gmean) / bound).max())
        # the variance gradient at love_ref's cache
        tvar = ig.gvar_tolerance(kind, ls, f)[None, :]
        e3 = float((np.abs(gvar - d_gvar) / tvar).max())
        print(f"{kind} N={N} D={D} r={rank} max_error {max_error:.0e}: g_mean re-assembled {e1:.2e} of the product tolerance, against dense {e2:.2e} of the "
              f"solve bound; g_var {e3:.2e} of its tolerance ({float(np.abs(gvar - d_gvar).max()):.2e} absolute)")
        assert e1 <= 1.0 and e2 <= 1.0 and e3 <= 1.0


# ---- 3. sample paths solved once ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sr.SAMPLE_S)
@pytest.mark.parametrize("case", ig.PREDICT_CASES, ids=lambda c: "N%d_D%d_%s" % c[:3])
def test_paths(case, S):
    N, D, kind, k = case
    h = sr.sample_hypers(D)
    ls, f = np.asarray(h["lengthscales"], dtype=np.float64), h["variance"]
    X, y = ref.problem(N, D)
    xnew, other = sr.sample_new_points(X, 17), sr.sample_new_points(X, 5)
    omega, b, W, eps = sr.sample_draws(N, D, kind, S)
    a, c2 = _context(X, y, kind, h, k), _context(X, y, kind, h, k)
    try:
        sample = a.itergp_sample(xnew, omega, b, W, eps, max_error=1e-8, return_solves=True)
        c2.set_option("k1_profile", 1)
        solved = c2.itergp_paths_solve(omega, b, W, eps, max_error=1e-8)
        launches = c2.get_stat("k1_launches")
        f0, none = c2.itergp_paths_eval(xnew, omega, b, W, solved.solves)
        f1, g1 = c2.itergp_paths_eval(xnew, omega, b, W, solved.solves, with_grad=True)
        f2, g2 = c2.itergp_paths_eval(other, omega, b, W, solved.solves, with_grad=True)
        f3, _ = c2.itergp_paths_eval(other, omega, b, W, solved.solves)
        assert c2.get_stat("k1_launches") == launches                    # evaluating ran no K_ff mat-vec: no solve
        if S == 1:
            assert launches > 0                                          # ... which the one-column solve does run
        U = solved.solves.cpu().numpy()
        assert np.array_equal(U, sample.solves.cpu().numpy()) and (solved.steps, solved.residual_error) == (sample.steps, sample.residual_error)
        assert none is None and np.array_equal(f0.cpu().numpy(), sample.samples.cpu().numpy())
        assert np.array_equal(f3.cpu().numpy(), a.itergp_sample(other, omega, b, W, eps, max_error=1e-8).samples.cpu().numpy())
        f1, g1, f2, g2 = [t.cpu().numpy() for t in (f1, g1, f2, g2)]
    finally:
        a.close()
        c2.close()
    cen = sr.centre(X)
    for pts, fv, gv in ((xnew, f1, g1), (other, f2, g2)):
        want_f, want_g, _ = ig.paths(kind, X, y, h, pts, omega, b, W, eps, U=U)
        assert fv.shape == (S, len(pts)) and gv.shape == (S, len(pts), D) and np.all(np.isfinite(gv))
        ef = float((np.abs(fv - want_f) / np.maximum(np.abs(want_f), math.sqrt(f))).max())
        tol = ig.cross_tolerance(kind, pts, X, ls, f, U.T)[1] + ig.feature_tolerance(pts, cen, ls, f, omega, b, W)[1]
        eg = float((np.abs(np.swapaxes(gv, 0, 1) - np.swapaxes(want_g, 0, 1)) / tol).max())
        print(f"{kind} N={N} D={D} S={S} n={len(pts)}: values {ef:.2e} of max(|f|, sqrt f), gradients {eg:.2e} of the summed product tolerances")
        assert ef <= ig.TOL_SAMPLE and eg <= 1.0


# ---- 4. backend, refusals, neighbours ---------------------------------------------------------------------------------------------------
@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


def test_paths_itergpr(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import PathsIterGPR, SampleIterGPR
    X, y = ref.problem(300, 3)
    xnew = torch.as_tensor(sr.sample_new_points(X, 17))

    def model(seed):
        return backend.create_model(config.IterGPRConfig(config.Matern52Config(), prec_size=8, seed=seed), (X, y))

    want = SampleIterGPR(model(3))(xnew, 5)
    m = model(3)
    paths = PathsIterGPR(m, 5)
    got = paths(xnew)
    assert got.shape == (5, 17, 1) and torch.equal(got, want)               # the samples SampleIterGPR returns from the same seed, bitwise
    assert torch.equal(paths(xnew), got)                                    # the same paths at every call
    fv, gv = paths.value_and_grad(xnew)
    assert fv.shape == (5, 17, 1) and gv.shape == (5, 17, 3)
    assert float((fv - got).abs().max()) <= 1e-9
    x = xnew.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(paths(x).sum(), x)
    assert grad.shape == x.shape and torch.equal(grad.to(gv.device), gv.sum(dim=0))
    with pytest.raises(ValueError):
        PathsIterGPR(object(), 2)
    m.covar_module.base_kernel.lengthscale = torch.full((1, 3), 0.7, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="other hyper-parameters"):
        paths(xnew)
    # pushed to the library behind the model's back: the same refusal
    m2 = model(3)
    p2 = PathsIterGPR(m2, 2, num_features=65)
    ls = m2.covar_module.base_kernel.lengthscale.detach().cpu().numpy().reshape(-1)
    m2.hip.set_hypers(2.0 * ls, 1.0, 0.1, 0.0, X[:8].copy(), 1e-6)
    with pytest.raises(RuntimeError, match="other hyper-parameters"):
        p2.value_and_grad(xnew)


def test_predict_grad_itergpr(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import PredictGradIterGPR, PredictIterGPR
    X, y = ref.problem(300, 3)
    xnew = torch.as_tensor(sr.sample_new_points(X, 17))
    m = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), (X, y))
    mean, dmean, var, dvar = PredictGradIterGPR(m, var_rank=33)(xnew)
    assert mean.shape == (17, 1) and dmean.shape == (17, 3) and var.shape == (17, 1) and dvar.shape == (17, 3)
    assert int(m.hip.get_stat("itergp_cache_request")) == 33                 # built on demand
    m2 = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), (X, y))
    want_mean, want_var = PredictIterGPR(m2, var_rank=33)(xnew)
    assert torch.equal(mean, want_mean) and torch.equal(var, want_var)
    mean0, dmean0, var0, dvar0 = PredictGradIterGPR(m2)(xnew)                # the model's rank: 0
    assert var0 is None and dvar0 is None and dmean0.shape == (17, 3)
    with pytest.raises(ValueError):
        PredictGradIterGPR(object())


def _all_entries(ctx, X, xs, draws, U):
    """every new entry once; returns nothing"""
    omega, b, W, eps = draws
    ctx.cross_grad_matmat(xs, np.ones((len(X), 2)))
    ctx.feature_grad_matmat(xs, omega, b, W)
    ctx.itergp_predict_grad(xs, with_var=False)
    ctx.itergp_paths_solve(omega, b, W, eps)
    ctx.itergp_paths_eval(xs, omega, b, W, U, with_grad=True)
    ctx.time_cross_grad_matmat(3, 2, 1)


def test_refusals():
    N, D, k = 65, 3, 4
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    draws = sr.sample_draws(N, D, "rbf", 2)
    U = np.zeros((2, N))

    def each(ctx, xs, match, Xc=X, dr=draws):
        omega, b, W, eps = dr
        calls = (lambda: ctx.cross_grad_matmat(xs, np.ones((len(Xc), 2))), lambda: ctx.feature_grad_matmat(xs, omega, b, W),
                 lambda: ctx.itergp_predict_grad(xs, with_var=False), lambda: ctx.itergp_paths_solve(omega, b, W, eps),
                 lambda: ctx.itergp_paths_eval(xs, omega, b, W, np.zeros((2, len(Xc)))), lambda: ctx.time_cross_grad_matmat(3, 2, 1),
                 lambda: ctx.time_feature_grad_matmat(3, 5, 2, 1))
        for call in calls:
            with pytest.raises(ValueError, match=match):
                call()

    ctx = _context(X, y, "rbf", h, k, dtype=torch.float32)
    try:
        each(ctx, X[:3], "-t fp64")
    finally:
        ctx.close()
    Xw, yw = ref.problem(N, 33)
    ctx = _context(Xw, yw, "rbf", ref.hypers(33, True), k)
    try:
        each(ctx, Xw[:3], "no wide path yet", Xc=Xw, dr=sr.sample_draws(N, 33, "rbf", 2))
    finally:
        ctx.close()
    ctx = _context(X, y, "rbf", h, k)
    try:
        good = [t.cpu().numpy() for t in ctx.cross_grad_matmat(X[:3], np.ones((N, 2)))]
        ctx.set_targets(np.stack([y, -y], axis=1))
        each(ctx, X[:3], "logdet_bound 0|one target column")
        ctx.set_targets(y)
        ctx.set_option("logdet_bound", 1)
        each(ctx, X[:3], "logdet_bound 0")
        ctx.set_option("logdet_bound", 0)
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
        again = [t.cpu().numpy() for t in ctx.cross_grad_matmat(X[:3], np.ones((N, 2)))]
        assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])       # the context is still usable
        _all_entries(ctx, X, X[:3], draws, U)
    finally:
        ctx.close()


def test_the_new_calls_leave_the_predictive_state_alone():
    """the pattern of test_sampling_leaves_the_predictive_state_alone (tests/test_gpu_itergp_sample.py): the new entries between predictive calls
    move neither alpha, the preconditioner nor the variance cache"""
    N, D, kind, k = sr.SAMPLE_CASES[1]
    h = sr.sample_hypers(D)
    X, y = ref.problem(N, D)
    xnew = sr.sample_new_points(X, 17)
    draws = sr.sample_draws(N, D, kind, 9)

    def run(with_new_calls):
        ctx = _context(X, y, kind, h, k)
        out = []
        try:
            ctx.itergp_objective_and_grad(np.random.default_rng(0).standard_normal((2, k + N)), torch.zeros(N, dtype=torch.float64, device=ctx.device),
                                          with_grad=False)
            assert ctx.itergp_var_cache(12) >= 1
            for _ in range(3):
                out += [t.cpu().numpy() for t in ctx.itergp_predict(xnew, max_error=1e-6)]
                out += [t.cpu().numpy() for t in ctx.itergp_predict_cached(xnew, max_error=1e-6)]
                if with_new_calls:
                    omega, b, W, eps = draws
                    ctx.cross_grad_matmat(xnew, np.ones((N, 3)))
                    ctx.feature_grad_matmat(xnew, omega, b, W)
                    ctx.itergp_predict_grad(xnew, max_error=1e-6)
                    U = ctx.itergp_paths_solve(omega, b, W, eps, max_error=1e-6).solves
                    ctx.itergp_paths_eval(xnew, omega, b, W, U, with_grad=True)
                    ctx.itergp_paths_eval(xnew, omega, b, W, U)
                    assert int(ctx.get_stat("itergp_cache_request")) == 12
        finally:
            ctx.close()
        return out

    with_calls, plain = run(True), run(False)
    assert len(with_calls) == len(plain) == 12
    for got, want in zip(with_calls, plain):
        assert np.array_equal(got, want)
