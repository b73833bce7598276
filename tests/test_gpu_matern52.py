"""The Matern-5/2 kernel through every pair kernel and model class on the GPU.

Reference: the closed form of tests/matern52_ref.py, handed to the unchanged oracle and helper modules for the duration of each test
(`oracle_with_matern52`).  The blocked C oracle has no Matern-5/2, so fp64 mat-vec references are numpy direct differences.  Shapes are
the smallest that reach each instance (tests/geometry_cases.py, tests/predict_ref.py).  tests/test_matern52_ref_host.py shows that a
kernel computing the Matern-3/2 profile or gradient factor instead would miss each tolerance used here by >= 100x.

Tolerances are those the existing tests hold Matern-3/2 to, named at each use.  Two are set here:
  * precision level 2 (degree-2 table polynomial, kernel values to 1.03e-10 relative): mat-vec to 1e-9 max|ref|, the bound
    tests/test_gpu_multi_output.py holds level 2 to - the polynomial's error on every term, with a factor 10 for sum|terms| / |sum|;
  * cross mat-vec rows: 2e-12 of the largest row sum of absolute terms (one output row alone has no max over rows to lean on).
"""
import functools
import os

import numpy as np
import pytest
import torch

import fp32_error_model as em
import geometry_cases as gc
import matern52_ref as m52
from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu

KIND = m52.KIND


@pytest.fixture(autouse=True)
def _oracle_knows_matern52():
    with m52.oracle_with_matern52():
        yield


def _ctx(X, y, hyp, dtype=torch.float64, M=None, row_range=None, **options):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, hyp.Z.shape[0] if M is None else M, KIND, dtype=dtype, row_range=row_range)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    return ctx


def _mv(ctx, p):
    return ctx.matvec(torch.from_numpy(p)).double().cpu().numpy()


def _close(out, ref, rel, what=""):
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"{what}: max |out - ref| / max |ref| = {err:.3g} (bound {rel})")
    assert err <= rel, what


# --------------------------------------------------------------------------- 1. symmetric mat-vec, every rows-per-lane class
@pytest.mark.parametrize("i", range(len(gc.CLASSES)), ids=[f"{c[0]}-D{c[1]}" for c in gc.CLASSES])
def test_symmetric_matvec_every_rows_per_lane_class(i):
    dtype, D, extra = gc.CLASSES[i]
    opt, order, prec = gc.CHUNKS[i % 7], i % 2, (i // 2) % 2
    for N in gc.sizes(dtype, D, opt):
        X, _, hyp, p = gc.problem(N, D)
        ctx = gc.make_ctx(KIND, dtype, X, hyp, dict(extra, sym_chunk=opt, sym_order=order, precision=prec))
        out = _mv(ctx, p)
        if dtype == "fp64":
            _close(out, m52.dense_matvec(X, hyp, p), gc.ATOL64, f"fp64 D={D} N={N} chunk={opt}")
        else:
            case = em.matvec_case(KIND, X, hyp, p, chunk=gc.eff_chunk(opt))
            gc.check(out, case.ref, case.s, gc.bound(dtype), f"fp32 D={D} N={N} chunk={opt}")
        assert ctx.get_stat("k1_pairs_per_launch") == gc.pairs_closed_form(N, gc.rbrows(dtype, D))
        assert np.array_equal(_mv(ctx, p), out), "a second call differs"
        ctx.close()


# --------------------------------------------------------------------------- 2. padded widths and precision levels
@pytest.mark.parametrize("D", [1, 6, 10, 14, 24, 27, 32])
def test_padded_widths_and_precision_levels(D):
    N = 1301
    X, _, hyp, p = gc.problem(N, D)
    ref = m52.dense_matvec(X, hyp, p)
    for prec, rel in ((0, gc.ATOL64), (1, gc.ATOL64), (2, 1e-9)):
        ctx = _ctx(X, np.zeros(N), hyp, precision=prec)
        _close(_mv(ctx, p), ref, rel, f"D={D} precision {prec}")
        ctx.close()


# --------------------------------------------------------------------------- 3. plain and rectangular kernels
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("jsplit", [1, 7])
def test_plain_matvec_kernel(jsplit, rows):
    for N, D in ((1301, 8), (700, 20)):
        X, _, hyp, p = gc.problem(N, D)
        ctx = _ctx(X, np.zeros(N), hyp, kff_variant=0, kff_jsplit=jsplit, kff_rows=rows)
        _close(_mv(ctx, p), m52.dense_matvec(X, hyp, p), gc.ATOL64, f"plain N={N} D={D} jsplit={jsplit} rows={rows}")
        ctx.close()


@pytest.mark.parametrize("n_new", [1, 257])
def test_cross_matvec(n_new):
    N, D = 1301, 8
    X, _, hyp, p = gc.problem(N, D)
    Xnew = np.concatenate([X[:n_new // 2], np.random.default_rng(n_new).standard_normal((n_new - n_new // 2, D))])
    ctx = _ctx(X, np.zeros(N), hyp)
    out = ctx.cross_matvec(Xnew, torch.from_numpy(p)).double().cpu().numpy()
    ctx.close()
    K = orc.kernel_matrix(KIND, Xnew, X, hyp.lengthscales, hyp.variance)
    assert np.abs(out - K @ p).max() <= gc.ATOL64 * (np.abs(K) @ np.abs(p)).max()


def test_implicit_preconditioner_rectangular_kernel():
    """precond_mode 1: K_uf r and K_fu t through kff_rect_generic, against the oracle's Nystrom preconditioner at the bound of
    tests/test_gpu_pair_geometry.py (1e-9 of the largest entry)."""
    N, D, M = 1301, 8, 24
    X, y, hyp, p = em.problem(N, D, M=M)
    ctx = _ctx(X, y, hyp, precond_mode=1)
    ctx.setup()
    z, rz = ctx.precond(torch.from_numpy(p))
    ctx.close()
    terms = orc.common_terms(KIND, X, hyp)
    zr, rzr = orc.nystrom_precond(terms.A, terms.LB, hyp.noise, p)
    _close(z.cpu().numpy(), zr, 1e-9, "implicit preconditioner")
    assert rz == pytest.approx(rzr, rel=1e-9)


def test_matrix_pipe_variant_is_refused():
    X, _, hyp, p = gc.problem(300, 8)
    ctx = _ctx(X, np.zeros(300), hyp, kff_variant=1)
    with pytest.raises(ValueError, match="kff_variant 1"):
        ctx.matvec(torch.from_numpy(p))
    ctx.set_option("kff_variant", 2)
    _close(_mv(ctx, p), m52.dense_matvec(X, hyp, p), gc.ATOL64, "after the refusal")
    ctx.close()


# --------------------------------------------------------------------------- 4. clamped exponent range and bias edge
def _box_problem(hw, ls, N=1500, D=2, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-hw, hw, size=(N, D))
    X[0], X[1], X[2] = hw, -hw, [hw, -hw]
    X[3] = X[0] * (1 - 1e-9)
    hyp = orc.Hypers(np.full(D, ls), 1.3, 0.2, 0.0, X[4:12].copy(), 1e-6)   # distinct inducing points (X[3] nearly repeats X[0])
    return X, rng.standard_normal(N), hyp, rng.standard_normal(N)


@pytest.mark.parametrize("hw,ls,why", [(3.0, 0.05, "range"), (10.0, 1.0, "bias"), (1.0, 1.0, "neither")])
def test_clamped_exponent_range_and_bias_cap(hw, ls, why):
    """cglb_set_hypers, Matern kinds, D = 2, box of half width hw: s2 = 2 (hw sqrt5 log2e / l)^2.  The unclamped kernels need
    2 s2 256^2 < 1e9, i.e. s2 < 7629: hw = 3, l = 0.05 gives s2 = 74 900 (clamped for the range).  hw = 10, l = 1 gives s2 = 2081 (in range)
    and a bias 1.5 u (5 D + 3) s2 128^2 = 7.4e-8 above the cap 2e-8 (clamped for the bias); hw = 1 gives 7.4e-10: the biased kernels run.
    Bound: 1e-10 max|ref|, as tests/test_gpu_kff_variants.py holds Matern-3/2 at the range limit (the Gram form loses |x|^2 u)."""
    X, y, hyp, p = _box_problem(hw, ls)
    ks2 = 5.0 * np.log2(np.e) ** 2
    s2 = (np.abs(X - X.mean(0)).max(0) ** 2 * ks2 / ls ** 2).sum()
    bias = 1.5 * 2.0 ** -53 * 13 * s2 * 128.0 ** 2
    assert {"range": s2 > 7629, "bias": s2 < 7629 and bias > 2e-8, "neither": s2 < 7629 and bias < 2e-8}[why]
    ref = m52.dense_matvec(X, hyp, p)
    for prec in (0, 1):
        ctx = _ctx(X, y, hyp, precision=prec)
        out = _mv(ctx, p)
        assert np.isfinite(out).all()
        _close(out, ref, 1e-10, f"{why} precision {prec}")
        v = torch.zeros(len(y), dtype=torch.float64, device=ctx.device)
        res = ctx.objective_and_grad(v, True, 1.0)
        ctx.close()
        at_v = orc.objective(KIND, X, y, hyp, v.cpu().numpy(), run_cg=False, with_grad=True)
        assert res.bound == pytest.approx(at_v.bound, rel=1e-9)
        g, rg = res.grad["lengthscales"], at_v.grad["lengthscales"]
        np.testing.assert_allclose(g, rg, rtol=1e-6, atol=1e-8 * max(1.0, np.abs(rg).max()))


def test_coincident_rows_and_inducing_points_on_data():
    """As test_duplicate_training_points_and_inducing_on_data (tests/test_gpu_edge_cases.py): distance exactly 0, h = 5 f / 3 finite there."""
    X, y, _ = orc.synthetic_problem(200, 2, 4, seed=3)
    X[10] = X[11] = X[12]
    Z = X[[10, 50, 90, 130]].copy()
    hyp = orc.Hypers(np.array([0.8, 1.2]), 1.0, 0.1, 0.0, Z, 1e-6)
    p = np.random.default_rng(0).standard_normal(200)
    for gram in (0, 1):
        ctx = _ctx(X, y, hyp, precision=1, grad_gram=gram)
        _close(_mv(ctx, p), m52.dense_matvec(X, hyp, p), gc.ATOL64, "coincident rows")
        v = torch.zeros(200, dtype=torch.float64, device=ctx.device)
        res = ctx.objective_and_grad(v, True, 1e-4)
        ctx.close()
        at_v = orc.objective(KIND, X, y, hyp, v.cpu().numpy(), run_cg=False, with_grad=True)
        assert res.bound == pytest.approx(at_v.bound, rel=1e-11)
        assert np.isfinite(res.grad["Z"]).all() and np.isfinite(res.grad["lengthscales"]).all()
        np.testing.assert_allclose(res.grad["Z"], at_v.grad["Z"], rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(res.grad["lengthscales"], at_v.grad["lengthscales"], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("N", [1, 2])
def test_one_and_two_points(N):
    X = np.array([[0.3, -0.2, 1.1], [0.9, 0.4, -0.5]])[:N]
    hyp = orc.Hypers(np.array([0.8, 1.2, 1.0]), 1.3, 0.2, 0.1, X[:1].copy(), 1e-6)
    p = np.array([0.7, -1.9])[:N]
    for dtype, rel in ((torch.float64, gc.ATOL64), (torch.float32, 1e-6)):
        ctx = _ctx(X, np.zeros(N), hyp, dtype=dtype)
        _close(_mv(ctx, p), m52.dense_matvec(X, hyp, p), rel, f"N={N} {dtype}")
        ctx.close()


# --------------------------------------------------------------------------- 5. objective, gradient and step count
OBJECTIVE_CASES = [(300, 3, 12, 1.0, 15), (640, 8, 32, 1.0, 17), (1301, 20, 24, 1.0, 9), (640, 8, 32, 1e-2, 24)]


@functools.lru_cache(maxsize=None)
def _objective_reference(N, D, M, max_error):
    """The patched oracle's solve from v = 0, once per case (callers run inside the patch and do not modify it)."""
    X, y, Z = orc.synthetic_problem(N, D, M, seed=11)
    hyp = orc.trained_like_hypers(D, Z)
    return X, y, hyp, orc.objective(KIND, X, y, hyp, np.zeros(N), True, max_error)


def _check_objective(res, v, X, y, hyp, ref):
    assert abs(res.bound - ref.bound) <= 1e-9 * abs(ref.bound), (res.bound, ref.bound)
    at_v = orc.objective(KIND, X, y, hyp, v, run_cg=False, with_grad=True)
    assert abs(res.bound - at_v.bound) <= 1e-11 * abs(at_v.bound), (res.bound, at_v.bound)
    assert abs(res.logdet - at_v.logdet) <= 1e-10 * abs(at_v.logdet), (res.logdet, at_v.logdet)
    for k in ("lengthscales", "variance", "noise", "mean", "Z"):   # smoke()'s tolerances
        np.testing.assert_allclose(np.asarray(res.grad[k]), at_v.grad[k], rtol=1e-7, atol=1e-8 * max(1.0, np.abs(at_v.grad[k]).max()), err_msg=k)


@pytest.mark.parametrize("N,D,M,max_error,steps", OBJECTIVE_CASES, ids=[f"N{c[0]}-D{c[1]}-M{c[2]}-e{c[3]}" for c in OBJECTIVE_CASES])
def test_objective_gradient_and_step_count(N, D, M, max_error, steps):
    X, y, hyp, ref = _objective_reference(N, D, M, max_error)
    assert ref.steps == steps, "fixture: the oracle's own step count moved"
    for gram, trsm in ((1, 1), (0, 2), (1, 2), (0, 1)):
        ctx = _ctx(X, y, hyp, grad_gram=gram, grad_trsm=trsm)
        v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
        res = ctx.objective_and_grad(v, True, max_error)
        ctx.close()
        print(f"grad_gram {gram} grad_trsm {trsm}: steps {res.steps} (oracle {ref.steps}), bound {res.bound!r} (oracle {ref.bound!r})")
        assert res.steps == ref.steps
        _check_objective(res, v.cpu().numpy(), X, y, hyp, ref)


@pytest.mark.parametrize("D,kw", [(12, {}), (24, {}), (8, dict(M=32, random_Z=True))], ids=["D12", "D24", "D8-M32-randomZ"])
def test_objective_and_gradient_at_fp32(D, kw):
    """The fp32 round-off model (tests/fp32_error_model.py: grad_case, bound_scale, TAU) through the case function of
    tests/test_gpu_fp32_parity.py, unchanged; its non-RBF envelope covers Matern-5/2 within 1.14 (host test), inside TAU's 4x margin."""
    import test_gpu_fp32_parity as fp
    ratios = fp.grad_case(KIND, D, **kw)
    print(ratios)
    bad = {q: r for q, r in ratios.items() if not r <= fp.tau_of(q)}
    assert not bad, bad


# --------------------------------------------------------------------------- 6. mid and wide inputs
@pytest.mark.parametrize("D,options", [(50, dict(wide_reg=0)), (50, dict(wide_reg=1)), (100, dict(wide_grad_sym=0)), (100, dict(wide_grad_sym=1))],
                         ids=["D50-gram", "D50-reg", "D100-nosym", "D100-sym"])
def test_mid_and_wide_inputs(D, options):
    """Tolerances of tests/test_gpu_wide.py for Matern-3/2: mat-vec 1e-11, bound at the same v 1e-10, gradient blocks 1e-7 of
    max(|block|, 1e-3 |bound|)."""
    N, M = 1100, 33
    X, y, hyp, p = em.problem(N, D, M=M)
    ctx = _ctx(X, y, hyp, **options)
    _close(_mv(ctx, p), m52.dense_matvec(X, hyp, p), 1e-11, f"D={D} {options}")
    v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
    res = ctx.objective_and_grad(v, True, 1.0)
    ctx.close()
    ref = orc.objective(KIND, X, y, hyp, np.zeros(N), True, 1.0)
    assert ref.steps <= 40 and res.steps == ref.steps
    at_v = orc.objective(KIND, X, y, hyp, v.cpu().numpy(), run_cg=False, with_grad=True)
    assert res.bound == pytest.approx(at_v.bound, rel=1e-10)
    for k in ("lengthscales", "variance", "noise", "Z"):
        b = np.asarray(at_v.grad[k])
        np.testing.assert_allclose(np.asarray(res.grad[k]), b, rtol=0, atol=1e-7 * max(np.abs(b).max(), 1e-3 * abs(at_v.bound)), err_msg=k)


# --------------------------------------------------------------------------- 7. prediction
@pytest.mark.parametrize("D,M", [(3, 33), (20, 24)])
def test_prediction_against_the_oracle_pieces(D, M):
    """cglb_predict at the GPU's own v against PredictCG.forward's pieces (quad_term 0) and the textbook SGPR predictive (quad_term 1), at
    tests/predict_ref.py's fp64 bound: 1e-8 of the largest entry.  New points: training rows, the inducing points, fresh points and one at
    1e3 in every coordinate (mean mu, variance f); outputs pre-filled with NaN."""
    import predict_ref as pr
    N = 700
    X, y, hyp, _ = em.problem(N, D, M=M)
    hyp.jitter = pr.JITTER
    Xnew = np.concatenate([X[:9], hyp.Z, np.random.default_rng(3).standard_normal((7, D)), np.full((1, D), pr.FAR)])
    ctx = _ctx(X, y, hyp)
    v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
    ctx.objective_and_grad(v, True, 1e-3, with_grad=False)
    mean, var = pr.predict(ctx, v, Xnew)
    vh = v.cpu().numpy()
    rm, rv = pr.cglb_predict(KIND, X, y, hyp, vh, Xnew)
    _close(mean, rm, 1e-8, "mean, quad_term 0")
    _close(var, rv, 1e-8, "variance, quad_term 0")
    assert mean[-1] == pytest.approx(hyp.mean, abs=1e-12) and var[-1] == pytest.approx(hyp.variance, rel=1e-12)
    ctx.set_option("logdet_bound", 1)   # the SGPR class, as tests/test_gpu_predict_geometry.py selects it
    ctx.set_option("quad_term", 1)
    ctx.setup()                         # the options invalidate the common terms
    mean1, var1 = pr.predict(ctx, np.full(N, np.nan), Xnew)
    ctx.close()
    sm, sv = pr.sgpr_predict(KIND, X, y, hyp, Xnew)
    _close(mean1, sm, 1e-8, "mean, quad_term 1")
    _close(var1, sv, 1e-8, "variance, quad_term 1")


# --------------------------------------------------------------------------- 8. other model classes
@pytest.mark.parametrize("cls", ["cglbnm2", "cglbn2m", "sgpr", "sgprn2m"])
def test_bound_variants_against_the_torch_restatement(cls):
    """logdet_bound 1 / 2 with quad_term 0 / 1, at the tolerances of tests/test_gpu_bound_variants.py (1e-10 on the bound, 1e-8 of the largest
    gradient entry)."""
    import test_gpu_bound_variants as tbv
    from cglb_amd.data import synthetic_problem
    N, M, D = 300, 16, 3
    X, y, Z = synthetic_problem(N, D, M, seed=N + D)
    h = tbv._hypers(D, True)
    ctx = tbv._context(X, y, M, KIND, cls)
    try:
        res, v = tbv._evaluate(ctx, h, Z, cls)
    finally:
        ctx.close()
    with m52.bound_variants_with_matern52() as bref:
        b, g = bref.bound_and_grad(cls, KIND, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Z,
                                   v=None if tbv.OPTIONS[cls][1] else v, device="cuda")
    assert abs(res.bound - b) <= 1e-10 * abs(b), (res.bound, b)
    tbv._assert_grad_close(res.grad, g, 1e-8)


def test_exact_gpr_value_gradient_and_predictive():
    """N = 300, gpr_block 64, at the tolerances of tests/test_gpu_gpr.py (1e-10 of the value scale, 1e-8 of the largest gradient entry; predictive
    1e-8 of the largest entry as tests/predict_ref.py)."""
    import gpr_ref as ref
    N, D = 300, 3
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    want = ref.evaluate(KIND, X, y, **h)
    Xnew = np.concatenate([X[:20], np.random.default_rng(5).standard_normal((21, D))])
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, 1, KIND)
    ctx.set_option("gpr_block", 64)
    ctx.gpr_set_hypers(**h)
    res = ctx.gpr_objective_and_grad()
    mean, var = ctx.gpr_predict(Xnew)
    ctx.close()
    scale = abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi)
    for name in ("lml", "quad", "logdet"):
        assert abs(getattr(res, name) - getattr(want, name)) <= 1e-10 * scale, name
    g, rg = ref.grad_vector(res.grad), ref.grad_vector(want.grad)
    assert np.abs(g - rg).max() <= 1e-8 * np.abs(rg).max(), (g, rg)
    rm, rv = ref.predict(KIND, X, want, h["lengthscales"], h["variance"], h["mean"], Xnew)
    _close(mean.cpu().numpy(), rm, 1e-8, "gpr mean")
    assert np.abs(var.cpu().numpy() - rv).max() <= 1e-8 * h["variance"]


@pytest.mark.parametrize("case", [(40, 3, 6), (67, 2, 9)], ids=lambda c: "N%d_D%d_k%d" % c)
def test_iterative_gp_in_the_exact_limit(case):
    """tests/test_gpu_itergp.py's exact limit: unit probes, N steps.  The restatement's own error for this kind is 2.9e-16 / 3.4e-14 at
    (40, 3, 6) and 6.4e-17 / 6.8e-14 at (67, 2, 9), so that file's floors 1e-10 / 1e-8 decide."""
    import gpr_ref as ref
    import itergp_ref as iref
    assert list(iref.EXACT_LIMIT_CASES) == [(40, 3, 6), (67, 2, 9)]
    N, D, k = case
    X, y = ref.problem(N, D)
    h = iref.exact_limit_hypers(D)
    want = ref.evaluate(KIND, X, y, **h)
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, KIND)
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
    res = ctx.itergp_objective_and_grad(iref.unit_probes(k, N), torch.zeros(N, dtype=torch.float64, device=ctx.device), max_error=1e-20,
                                        max_cg_iter=N, lanczos_iter=N)
    ctx.close()
    scale = abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi)
    for name in ("lml", "quad", "logdet"):
        assert abs(getattr(res, name) - getattr(want, name)) <= 1e-10 * scale, name
    g, rg = ref.grad_vector(res.grad), ref.grad_vector(want.grad)
    assert np.abs(g - rg).max() <= 1e-8 * np.abs(rg).max(), (g, rg)


@pytest.mark.parametrize("N,D,S", [(513, 8, 3), (257, 12, 9)])
def test_multi_pair_gradient_pass(N, D, S):
    """cglb_grad_kff_multi against itergp_ref.bilinear_forms at tests/test_gpu_grad_multi.py's 1e-11 of the sum of absolute terms."""
    import gpr_ref as ref
    import itergp_ref as iref
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    rng = np.random.default_rng(N + S)
    U, V = rng.standard_normal((N, S)), rng.standard_normal((N, S))
    want = iref.bilinear_forms(KIND, X, h["lengthscales"], h["variance"], U, V)
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, 1, KIND)
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:1].copy(), 1e-6)
    got, again = ctx.grad_kff_multi(U, V), ctx.grad_kff_multi(U, V)
    ctx.close()
    assert np.all(np.abs(got - np.concatenate([want["lengthscales"], [want["variance"]]])) <= 1e-11 * want["abs"]), (got, want)
    assert np.array_equal(got, again)


def test_multi_column_product_and_solve():
    """cglb_matmat / cglb_pcg_solve_multi with P = 3 against tests/multi_output_ref.py, at tests/test_gpu_multi_output.py's bounds."""
    import multi_output_ref as mref
    N, D, M, P = 400, 3, 24, 3
    X, Y, hyp = mref.problem(N, D, M, P, seed=11)
    cov, terms = orc.dense_cov(KIND, X, hyp), orc.common_terms(KIND, X, hyp)
    Vref, steps, half = mref.stable_steps(cov, Y - hyp.mean, np.zeros_like(Y), lambda r: orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r), 1.0)
    assert 0 < steps <= 40
    ctx = _ctx(X, Y, hyp, sym_chunk=16)
    ctx.setup()
    W = np.random.default_rng(1).standard_normal((N, P))
    out = ctx.matmat(torch.from_numpy(W)).cpu().numpy()
    for b in range(P):
        _close(out[:, b], cov @ W[:, b], gc.ATOL64, f"matmat column {b}")
    V, st, total, cols = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64))
    ctx.close()
    assert st == steps
    np.testing.assert_allclose(V.cpu().numpy(), Vref, rtol=0, atol=1e-8 * np.abs(Vref).max())
    np.testing.assert_allclose(cols, half, rtol=1e-5)


@pytest.mark.parametrize("N,D,M", [(700, 8, 64), (257, 16, 9)])
def test_inducing_point_selection(N, D, M):
    from cglb_amd.hip_context import HipContext
    rng = np.random.default_rng(N + D)
    X = rng.standard_normal((N, D))
    ls, var = 0.7 + rng.random(D), 1.7

    def fn(x1, x2=None, full_cov=False):
        x1 = np.asarray(x1, dtype=np.float64)
        return orc.kernel_matrix(KIND, x1, x1 if x2 is None else np.asarray(x2, dtype=np.float64), ls, var) if full_cov else np.full(len(x1), var)

    ctx = HipContext(X, np.zeros(N), M, KIND)
    idx, trace, Z = ctx.select_inducing(ls, var, return_Z=True)
    ctx.close()
    ref = orc.greedy_conditional_variance(X, M, fn)
    np.testing.assert_array_equal(X[idx], ref)
    np.testing.assert_array_equal(Z.cpu().numpy(), ref)


# --------------------------------------------------------------------------- 9. cyclic partials
@pytest.mark.parametrize("world", [2, 3])
def test_cyclic_partials_sum_to_the_full_matvec(world):
    N, D = 2999, 8
    X, _, hyp, p = gc.problem(N, D, seed=world)
    ctx = _ctx(X, np.zeros(N), hyp, sym_chunk=512)
    p_dev = ctx._dev(p, N)
    total = sum(gc.matvec_cyclic(ctx, p_dev, world, rank) for rank in range(world))
    ctx.close()
    _close(total, m52.dense_matvec(X, hyp, p), gc.ATOL64, f"world {world}")


# --------------------------------------------------------------------------- 10. headline geometry
def test_headline_geometry_sampled_rows():
    """N = 100 000, D = 8, M = 8, fp64, default options (chunk 1024, many slabs): 384 sampled rows of one mat-vec against numpy's
    direct-difference closed form (no N^2 reference)."""
    N, D = 100_000, 8
    X, y, Z = orc.synthetic_problem(N, D, 8, seed=1)
    hyp = orc.trained_like_hypers(D, Z)
    p = np.random.default_rng(2).standard_normal(N)
    ctx = _ctx(X, y, hyp)
    out = _mv(ctx, p)
    ctx.close()
    rows = np.random.default_rng(3).choice(N, 384, replace=False)
    rows[:3] = (0, N // 2, N - 1)
    K = m52.k52(orc.scaled_sqdist(X[rows], X, hyp.lengthscales), hyp.variance)
    ref = K @ p + hyp.noise * p[rows]
    _close(out[rows], ref, gc.ATOL64, "sampled rows")


# --------------------------------------------------------------------------- 11. product API
def _model(M=16):
    import test_gpu_backend as tb
    from cglb_amd.backend import BACKENDS, CGLBConfig, InducingVariableConfig, Matern52Config
    be = BACKENDS["hip"]
    be.configure_backend(logdir="/tmp/cglb_amd_test", keops=False)
    be.set_default_float("fp64")
    be.set_default_jitter("fp64")
    train, test = tb._data()
    return be, be.create_model(CGLBConfig(Matern52Config(), InducingVariableConfig(M)), train), (train, test), tb


def test_create_model_loss_and_autograd_equal_the_oracle():
    from cglb_amd.backend.models import LowerBoundCG
    be, model, (train, _), tb = _model()
    assert model.covar_module.base_kernel.base_kernel.kind == "matern52"
    loss = -LowerBoundCG(model)(None)
    hyp = tb._hyp_of(model)
    ref = orc.objective(KIND, train[0], train[1], hyp, np.zeros(len(train[1])), True, 1.0)
    assert model.cg_stats.steps == ref.steps
    assert float(loss) == pytest.approx(-ref.bound, rel=1e-10)
    grads = torch.autograd.grad(loss, list(model.parameters()))
    v = model.v_vec.cpu().numpy().reshape(-1)
    g = orc.objective(KIND, train[0], train[1], hyp, v, run_cg=False, with_grad=True).grad
    named = dict(model.named_parameters())
    got = {n: gr for (n, _), gr in zip(model.named_parameters(), grads)}
    sig = lambda raw: torch.sigmoid(raw).numpy()
    np.testing.assert_allclose(got["covar_module.inducing_points"].numpy(), -g["Z"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(got["covar_module.base_kernel.base_kernel._lengthscale.raw"].numpy().reshape(-1),
                               -g["lengthscales"] * sig(named["covar_module.base_kernel.base_kernel._lengthscale.raw"].detach()).reshape(-1), rtol=1e-7)
    np.testing.assert_allclose(got["covar_module.base_kernel._outputscale.raw"].numpy(),
                               -g["variance"] * sig(named["covar_module.base_kernel._outputscale.raw"].detach()), rtol=1e-7)
    np.testing.assert_allclose(got["likelihood.noise_covar._noise.raw"].numpy(), -g["noise"] * sig(named["likelihood.noise_covar._noise.raw"].detach()), rtol=1e-7)


def test_five_optimize_steps_decrease_the_loss(tmp_path):
    from cglb_amd.backend.callbacks import Logger
    from cglb_amd.backend.models import LowerBoundCG
    be, model, data, _ = _model()
    mfn = be.metrics_fn(model, data)
    logger = Logger(str(tmp_path), mfn, lambda: be.model_parameters(model), holdout_interval=5, include_feval_log=True, verbose=False)
    first = float(-LowerBoundCG(model)(None))
    be.optimize(model, data, 5, logger, "scipy")
    last = mfn()["loss"]
    print("loss", first, "->", last)
    assert np.isfinite(last) and last < first


@pytest.mark.parametrize("command,model_args", [("cglb", ["-m", "cglb", "-i", "cv", "-M", "16"]), ("gpr", ["-m", "gpr"])])
def test_cli_train_and_metric(tmp_path, command, model_args):
    from click.testing import CliRunner
    from cglb_amd.cli import main
    logdir = str(tmp_path / "run")
    r = CliRunner().invoke(main, ["-b", "hip", "-t", "fp64", "-l", logdir, "-s", "0", "train", "-d", "synthetic-300-3", "-n", "5", command, "-k", "Matern52"]
                           + model_args, catch_exceptions=False)
    assert r.exit_code == 0, r.output
    for f in ("model.json", "results.json", "logs.json"):
        assert os.path.exists(os.path.join(logdir, f)), f
    r2 = CliRunner().invoke(main, ["-b", "hip", "-t", "fp64", "-l", logdir, "metric", "-d", "synthetic-300-3", command, "-k", "mat52"] + model_args
                            + ["-p", os.path.join(logdir, "model.json")], catch_exceptions=False)
    assert r2.exit_code == 0, r2.output
    assert os.path.exists(os.path.join(logdir, "metric.npy"))
