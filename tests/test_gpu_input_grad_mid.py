"""Input gradients of the iterative exact-GP class at mid widths (33 - 96 input dimensions) behind the option "input_grad_mid"
(csrc/kernels_input_grad_mid.hip): cglb_cross_grad_matmat, cglb_feature_grad_matmat, their timers, cglb_itergp_predict_grad,
cglb_itergp_paths_solve / _eval, `PredictGradIterGPR(wide=True)`, `PathsIterGPR(wide=True)`, against the longdouble restatement
tests/input_grad_ref.py at the cells and tolerances of tests/input_grad_mid_ref.py.  Small shapes; every
output is pre-filled with NaN.

1. Option off: the D = 33 context refuses as before and "input_grad_native" is 0; with the option on it is 1 and the call returns.
2. Per cell of input_grad_mid_ref.product_cells (D in 33, 48, 49, 64, 65, 80, 81, 96; n_new in 1, 2, 63, 64, 65; N in 1, 65, 300; kff_jsplit 1, 3, 7;
   S in 1, G, G + 1, 9; F in 1, 65; the three kinds; precision levels 0 and 2 on one cell per kind), cross and feature product: every element
   within input_grad_ref.cross_tolerance / feature_tolerance and finite; a second call bitwise equal; with out NULL the gradient bitwise the
   same; the cross values within twice the tolerance of cglb_cross_matvec column by column; N = 1 gives exact zeros; the row at 10^3 is below
   the floor.
3. cglb_itergp_predict_grad at wide_cases.CACHE_CASES with the rank-8 and rank-33 caches: mean and variance bitwise those of
   cglb_itergp_predict_cached; g_mean re-assembled from the library's alpha to the product tolerance and within sqrt(C f) / l_k sqrt(2 max_error)
   of the dense gradient at max_error 1e-12 and 1e-3; g_var to input_grad_mid_ref.gvar_tolerance; CGLB_ERR_STATE without a cache.
4. Paths: the solves and (without gradients) the values are bitwise those of cglb_itergp_sample; with gradients the values are within 1e-10 of
   max(|f|, sqrt f) and the gradients within the sum of the two product tolerances at the library's U.  `PathsIterGPR(wide=True)`
   backpropagates; `PredictGradIterGPR(wide=True)` returns the four shapes.
5. Neighbouring scope: D = 97, wide_reg 0 and fp32 stay refused with the option on; a narrow context gives bitwise the same results with the option
   on and off.
"""
import functools
import math

import numpy as np
import pytest
import torch

import gpr_ref as ref
import input_grad_mid_ref as igm
import input_grad_ref as ig
import sample_ref as sr
import wide_cases as wc

pytestmark = pytest.mark.gpu
NAN = float("nan")
CELLS = igm.product_cells()


def _context(X, y, kind, h, k=1, dtype=torch.float64, mid=True):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)   # Z is a placeholder: the class selects its own
    if mid:
        ctx.set_option("input_grad_mid", 1)
    return ctx


def _nan(ctx, *shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=ctx.device)


# ---- 1. the option ------------------------------------------------------------------------------------------------------------------------------
def test_the_option_opens_the_mid_width_path():
    N, D = 65, 33
    X, y = ref.problem(N, D)
    ctx = _context(X, y, "rbf", ref.hypers(D, True), 4, mid=False)
    try:
        V = np.ones((N, 2))
        assert ctx.get_stat("input_grad_native") == 0.0
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.cross_grad_matmat(X[:3], V)
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.itergp_predict_grad(X[:3], with_var=False)
        ctx.set_option("input_grad_mid", 1)
        assert ctx.get_stat("input_grad_native") == 1.0
        out, g = ctx.cross_grad_matmat(X[:3], V, out=_nan(ctx, 3, 2), gout=_nan(ctx, 3, 2, D))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
        assert ctx.time_cross_grad_matmat(3, 2, 1) > 0.0
        ctx.set_option("input_grad_mid", 0)
        assert ctx.get_stat("input_grad_native") == 0.0
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.cross_grad_matmat(X[:3], V)
    finally:
        ctx.close()


# ---- 2. the cross product, cell by cell -----------------------------------------------------------------------------------------------------------
def _check_cell(c, precision):
    X, y, h, xnew, V, omega, b, W = igm.cell_problem(c)
    ls, f, n, S, D, kind = h["lengthscales"], h["variance"], c["n_new"], c["S"], c["D"], c["kind"]
    ctx = _context(X, y, kind, h)
    try:
        ctx.set_option("kff_jsplit", c["jsplit"])
        ctx.set_option("precision", precision)
        out, g = ctx.cross_grad_matmat(xnew, V, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        out2, g2 = ctx.cross_grad_matmat(xnew, V, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        none, g3 = ctx.cross_grad_matmat(xnew, V, gout=_nan(ctx, n, S, D), with_value=False)
        value_kernel = np.stack([ctx.cross_matvec(xnew, V[:, s].copy()).cpu().numpy() for s in range(S)], axis=1)
        fo, fg = ctx.feature_grad_matmat(xnew, omega, b, W, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        fo2, fg2 = ctx.feature_grad_matmat(xnew, omega, b, W, out=_nan(ctx, n, S), gout=_nan(ctx, n, S, D))
        fnone, fg3 = ctx.feature_grad_matmat(xnew, omega, b, W, gout=_nan(ctx, n, S, D), with_value=False)
        out, g, out2, g2, g3, fo, fg, fo2, fg2, fg3 = [t.cpu().numpy() for t in (out, g, out2, g2, g3, fo, fg, fo2, fg2, fg3)]
    finally:
        ctx.close()
    want_o, want_g = igm.cross_grad(kind, xnew, X, ls, f, V)
    tv, tg = igm.level_tolerance(kind, xnew, X, ls, f, V, precision)
    eo, eg = np.abs(out - want_o) / tv, np.abs(g - want_g) / tg
    print(f"{igm.cell_id(c)} precision {precision}: value {float(eo.max()):.2e}, gradient {float(eg.max()):.2e} of the tolerance; against cross_matvec "
          f"{float((np.abs(out - value_kernel) / tv).max()):.2e}")
    assert out.shape == (n, S) and g.shape == (n, S, D) and np.all(np.isfinite(out)) and np.all(np.isfinite(g))
    assert float(eo.max()) <= 1.0 and float(eg.max()) <= 1.0
    assert np.array_equal(out, out2) and np.array_equal(g, g2) and np.array_equal(g, g3) and none is None
    assert np.all(np.abs(out - value_kernel) <= 2 * tv)                     # the Gram-chain mat-vec's values, column by column
    floor = ig.FLOOR * f * np.abs(V).sum(axis=0)
    if c["N"] == 1:
        assert np.all(g[0] == 0.0)                                          # the coincident pair alone: exactly zero
    if n > 1:
        assert np.all(np.abs(out[1]) <= floor) and np.all(np.abs(g[1]) <= floor[:, None])   # the point at 10^3: everything underflows
    # the feature product
    cen = sr.centre(X)
    want_o, want_g = igm.feature_grad(xnew, cen, ls, f, omega, b, W)
    tv, tg = igm.feature_tolerance(xnew, cen, ls, f, omega, b, W)
    eo, eg = np.abs(fo - want_o) / tv, np.abs(fg - want_g) / tg
    print(f"{igm.cell_id(c)} precision {precision}: feature value {float(eo.max()):.2e}, gradient {float(eg.max()):.2e} of the tolerance")
    assert fo.shape == (n, S) and fg.shape == (n, S, D) and np.all(np.isfinite(fo)) and np.all(np.isfinite(fg))
    assert float(eo.max()) <= 1.0 and float(eg.max()) <= 1.0
    assert np.array_equal(fo, fo2) and np.array_equal(fg, fg2) and np.array_equal(fg, fg3) and fnone is None


@pytest.mark.parametrize("c", CELLS, ids=igm.cell_id)
def test_cross_product_matches_the_restatement(c):
    _check_cell(c, 1)


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("x", igm.PRECISION_CELLS, ids=lambda x: igm.cell_id(CELLS[x]))
def test_cross_product_at_the_other_precision_levels(x, precision):
    _check_cell(CELLS[x], precision)


# ---- 3. the predictive and its gradients ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_predict(N, D, kind, rank):
    X, y, h, xnew = wc.itergp_case(N, D)
    out = ig.predict_grad(kind, X, y, h, xnew, rank=rank)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("rank", igm.PREDICT_RANKS)
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("case", wc.CACHE_CASES, ids=lambda c: "N%d_D%d" % c)
def test_predict_grad(case, kind, rank):
    N, D = case
    X, y, h, xnew = wc.itergp_case(N, D)
    ls, f = np.asarray(h["lengthscales"], dtype=np.float64), h["variance"]
    d_mean, d_gmean, d_var, d_gvar = _dense_predict(N, D, kind, rank)
    a, b = _context(X, y, kind, h, 8), _context(X, y, kind, h, 8)       # two contexts in the same state
    try:
        with pytest.raises(RuntimeError, match="call order"):
            b.itergp_predict_grad(xnew)                                 # no cache yet
        assert a.itergp_var_cache(rank) == b.itergp_var_cache(rank) == rank
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
        _o, want = ig.cross_grad(kind, xnew, X, ls, f, alpha.reshape(-1, 1))        # re-assembled from the library's own alpha
        tol = ig.cross_tolerance(kind, xnew, X, ls, f, alpha.reshape(-1, 1))[1][:, 0, :]
        e1 = float((np.abs(gmean - want[:, 0, :]) / tol).max())
        bound = ig.solve_bound(kind, ls, f, max_error)[None, :] + tol                 # against the dense gradient: the solve bound
        e2 = float((np.abs(gmean - d_gmean) / bound).max())
        tvar = igm.gvar_tolerance(kind, ls, f)[None, :]                               # the variance gradient at love_ref's cache
        e3 = float((np.abs(gvar - d_gvar) / tvar).max())
        print(f"{kind} N={N} D={D} r={rank} max_error {max_error:.0e}: g_mean re-assembled {e1:.2e} of the product tolerance, against dense {e2:.2e} of the "
              f"solve bound; g_var {e3:.2e} of its tolerance ({float(np.abs(gvar - d_gvar).max()):.2e} absolute)")
        assert e1 <= 1.0 and e2 <= 1.0 and e3 <= 1.0


# ---- 4. sample paths solved once; the backend classes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("kind", wc.KINDS)
def test_paths(kind, S):
    N, D = wc.CACHE_CASES[1]
    X, y, h, xnew = wc.itergp_case(N, D)
    ls, f = np.asarray(h["lengthscales"], dtype=np.float64), h["variance"]
    other = ig.new_points(X, 5)
    omega, b, W, eps = sr.sample_draws(N, D, kind, S)
    a, c2 = _context(X, y, kind, h, 8, mid=False), _context(X, y, kind, h, 8)
    try:
        sample = a.itergp_sample(xnew, omega, b, W, eps, max_error=1e-8, return_solves=True)
        solved = c2.itergp_paths_solve(omega, b, W, eps, max_error=1e-8)
        f0, none = c2.itergp_paths_eval(xnew, omega, b, W, solved.solves)
        f1, g1 = c2.itergp_paths_eval(xnew, omega, b, W, solved.solves, with_grad=True)
        f2, g2 = c2.itergp_paths_eval(other, omega, b, W, solved.solves, with_grad=True)
        f3, _ = c2.itergp_paths_eval(other, omega, b, W, solved.solves)
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


@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


def test_predict_grad_itergpr_wide(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import PredictGradIterGPR, PredictIterGPR
    X, y, _h, xnew = wc.itergp_case(300, 40)
    xnew = torch.as_tensor(xnew)
    n = len(xnew)
    m = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), (X, y))
    with pytest.raises(ValueError, match="no wide path yet"):
        PredictGradIterGPR(m, var_rank=33)(xnew)
    mean, dmean, var, dvar = PredictGradIterGPR(m, var_rank=33, wide=True)(xnew)
    assert mean.shape == (n, 1) and dmean.shape == (n, 40) and var.shape == (n, 1) and dvar.shape == (n, 40)
    assert bool(torch.isfinite(dmean).all()) and bool(torch.isfinite(dvar).all())
    m2 = backend.create_model(config.IterGPRConfig(config.Matern32Config(), prec_size=8), (X, y))
    want_mean, want_var = PredictIterGPR(m2, var_rank=33)(xnew)
    assert torch.equal(mean, want_mean) and torch.equal(var, want_var)


def test_paths_itergpr_wide(backend):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import PathsIterGPR, SampleIterGPR
    X, y, _h, xnew = wc.itergp_case(300, 40)
    xnew = torch.as_tensor(xnew)
    n = len(xnew)

    def model(seed):
        return backend.create_model(config.IterGPRConfig(config.Matern52Config(), prec_size=8, seed=seed), (X, y))

    with pytest.raises(ValueError, match="no wide path yet"):
        PathsIterGPR(model(3), 5, num_features=65)
    want = SampleIterGPR(model(3), num_features=65)(xnew, 5)
    paths = PathsIterGPR(model(3), 5, num_features=65, wide=True)
    got = paths(xnew)
    assert got.shape == (5, n, 1) and torch.equal(paths(xnew), got)        # the same paths at every call
    assert torch.equal(got, want)                                           # the samples SampleIterGPR returns from the same seed, bitwise
    fv, gv = paths.value_and_grad(xnew)
    assert fv.shape == (5, n, 1) and gv.shape == (5, n, 40) and bool(torch.isfinite(gv).all())
    assert float((fv - got).abs().max()) <= 1e-9
    x = xnew.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(paths(x).sum(), x)
    assert grad.shape == x.shape and torch.equal(grad.to(gv.device), gv.sum(dim=0))


# ---- 5. the neighbouring scope --------------------------------------------------------------------------------------------------------------------
def test_neighbouring_scope():
    N = 65
    X, y = ref.problem(N, 97)
    ctx = _context(X, y, "rbf", ref.hypers(97, True), 4)
    try:
        assert ctx.get_stat("input_grad_native") == 0.0
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.cross_grad_matmat(X[:3], np.ones((N, 2)))
    finally:
        ctx.close()
    X, y = ref.problem(N, 40)
    ctx = _context(X, y, "rbf", ref.hypers(40, True), 4)
    try:
        ctx.set_option("wide_reg", 0)
        assert ctx.get_stat("input_grad_native") == 0.0
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.cross_grad_matmat(X[:3], np.ones((N, 2)))
        with pytest.raises(ValueError, match="no wide path yet"):
            ctx.itergp_predict_grad(X[:3], with_var=False)
    finally:
        ctx.close()
    ctx = _context(X, y, "rbf", ref.hypers(40, True), 4, dtype=torch.float32)
    try:
        assert ctx.get_stat("input_grad_native") == 0.0
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.cross_grad_matmat(X[:3], np.ones((N, 2)))
    finally:
        ctx.close()
    # a narrow context: the option changes nothing, bit for bit
    X, y = ref.problem(N, 20)
    h = ig.cell_hypers(20)
    V = np.random.default_rng(3).standard_normal((N, 3))
    got = {}
    for mid in (False, True):
        ctx = _context(X, y, "matern52", h, 4, mid=mid)
        try:
            assert ctx.get_stat("input_grad_native") == 1.0
            got[mid] = [t.cpu().numpy() for t in ctx.cross_grad_matmat(X[:5], V)] + [t.cpu().numpy() for t in ctx.itergp_predict_grad(X[:5], with_var=False)[:2]]
        finally:
            ctx.close()
    for p, q in zip(got[False], got[True]):
        assert np.array_equal(p, q)
