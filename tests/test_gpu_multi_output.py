"""Multi-output targets on the GPU: the shared-kernel product K_ff V (kernels_kff_multi.hip), the batched PCG, the evaluation, the
prediction, the fallback paths and the refusals, against the truth composed from the single-output oracle (tests/multi_output_ref.py).

Tolerances: the mat-mat product is held to ATOL64 of tests/geometry_cases.py per column; the solve, the evaluation and the prediction to
the figures tests/test_gpu_parity_golden.py applies to their single-output forms."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import geometry_cases as gc
import multi_output_ref as mref
from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu

KINDS = ("rbf", "matern32")
COLUMNS = (1, 2, 3, 4, 5, 8, 9)


def make_ctx(kind, X, Y, hyp, dtype=torch.float64, **options):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, Y, hyp.Z.shape[0], kind, dtype=dtype)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    return ctx


@functools.lru_cache(maxsize=None)
def matmat_case(kind, N, D):
    X, _y, hyp, _p = gc.problem(N, D, seed=5)
    V = np.random.default_rng(N + D).standard_normal((N, 9))
    cov = orc.dense_cov(kind, X, hyp)
    ref = cov @ V
    for a in (X, V, ref):
        a.setflags(write=False)
    return X, hyp, V, ref


def check_columns(out, ref, what):
    for b in range(ref.shape[1]):
        err = np.abs(out[:, b] - ref[:, b]).max()
        assert err <= gc.ATOL64 * np.abs(ref[:, b]).max(), f"{what} column {b}: {err:.3g}"


# N: not a multiple of 16 | not a multiple of 64 R | more than four row blocks; sym_chunk 16 (the smallest): many chunks at every size
@pytest.mark.parametrize("D", [1, 3, 8, 32])
@pytest.mark.parametrize("N", [37, 300, 1333])
@pytest.mark.parametrize("kind", KINDS)
def test_matmat_against_dense(kind, N, D):
    X, hyp, V, ref = matmat_case(kind, N, D)
    ctx = make_ctx(kind, X, np.zeros(N), hyp, sym_chunk=16)
    for P in COLUMNS:
        out = ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy()
        assert out.shape == (N, P)
        check_columns(out, ref[:, :P], f"{kind} N={N} D={D} P={P}")
    ctx.close()


# a span of several LDS chunks (sym_chunk 1024 > 1024 / S_pad) and a span that is no multiple of the LDS chunk (320 at S_pad 8)
@pytest.mark.parametrize("chunk", [320, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_matmat_span_of_several_lds_chunks(kind, chunk):
    X, hyp, V, ref = matmat_case(kind, 1333, 3)
    ctx = make_ctx(kind, X, np.zeros(1333), hyp, sym_chunk=chunk)
    for P in (2, 4, 8):
        check_columns(ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy(), ref[:, :P], f"{kind} chunk={chunk} P={P}")
    for order in (0, 1):
        ctx.set_option("sym_order", order)
        check_columns(ctx.matmat(torch.from_numpy(V[:, :4].copy())).cpu().numpy(), ref[:, :4], f"{kind} order={order}")
    ctx.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_matmat_precision_levels(kind, precision):
    X, hyp, V, ref = matmat_case(kind, 300, 8)
    ctx = make_ctx(kind, X, np.zeros(300), hyp, sym_chunk=16, precision=precision)
    out = ctx.matmat(torch.from_numpy(V[:, :4].copy())).cpu().numpy()
    single = np.stack([ctx.matvec(torch.from_numpy(V[:, b].copy())).cpu().numpy() for b in range(4)], axis=1)
    if precision < 2:
        check_columns(out, ref[:, :4], f"precision {precision}")
    # level 2 trades kernel values of ~1e-10 for speed: held to that level, and every level to its own single mat-vec
    tol = {0: gc.ATOL64, 1: gc.ATOL64, 2: 1e-9}[precision]
    assert np.abs(out - ref[:, :4]).max() <= tol * np.abs(ref[:, :4]).max()
    assert np.abs(out - single).max() <= gc.ATOL64 * np.abs(ref[:, :4]).max() * (1 if precision < 2 else 1e3)
    ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_matmat_zero_equal_and_permuted_columns(kind):
    X, hyp, V, ref = matmat_case(kind, 1333, 8)
    ctx = make_ctx(kind, X, np.zeros(1333), hyp, sym_chunk=16)
    W = V[:, :4].copy()
    W[:, 2] = 0.0
    out = ctx.matmat(torch.from_numpy(W)).cpu().numpy()
    assert not out[:, 2].any()
    check_columns(out[:, [0, 1, 3]], ref[:, [0, 1, 3]], "beside a zero column")
    same = ctx.matmat(torch.from_numpy(np.repeat(V[:, :1], 3, axis=1))).cpu().numpy()
    assert same[:, 0].tobytes() == same[:, 1].tobytes() == same[:, 2].tobytes()
    # run to run, and under a permutation of the columns inside one S_pad group: bitwise
    for P in (2, 4, 7):
        base = ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy()
        assert base.tobytes() == ctx.matmat(torch.from_numpy(V[:, :P].copy())).cpu().numpy().tobytes()
        perm = np.random.default_rng(P).permutation(P)
        out = ctx.matmat(torch.from_numpy(V[:, perm].copy())).cpu().numpy()
        assert out.tobytes() == np.ascontiguousarray(base[:, perm]).tobytes()
    ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_alternating_matvec_and_matmat_keep_their_work_lists_apart(kind):
    """One context, N = 2500, D = 3 (five 512-row blocks in two groups for the single kernel, 256- and 128-row blocks for the multi
    kernel), mat-vec and mat-mat calls in turn under a shuffled sequence of sym_chunk and sym_order: each kernel caches its own work
    list, keyed by what it was built for.  A wrong or shared key would serve a stale list: every result is held to the dense oracle and
    every repeat of a configuration to the bits of its first occurrence."""
    N = 2500
    X, hyp, V, ref = matmat_case(kind, N, 3)
    ctx = make_ctx(kind, X, np.zeros(N), hyp)
    settings = [(chunk, order) for chunk in (128, 256, 1024) for order in (0, 1)]
    rng = np.random.default_rng(17)
    vec = [(c, o, 1) for c, o in settings] * 6            # 36 mat-vecs and 36 mat-mats: every configuration returns
    mat = [(c, o, S) for c, o in settings for S in (2, 3, 8)] * 2
    rng.shuffle(vec)
    rng.shuffle(mat)
    first = {}
    for step, (chunk, order, S) in enumerate(x for pair in zip(vec, mat) for x in pair):
        ctx.set_option("sym_chunk", chunk)
        ctx.set_option("sym_order", order)
        if S == 1:
            out = ctx.matvec(torch.from_numpy(V[:, 0].copy())).cpu().numpy()[:, None]
        else:
            out = ctx.matmat(torch.from_numpy(V[:, :S].copy())).cpu().numpy()
        what = f"{kind} step {step}: chunk {chunk} order {order} S {S}"
        check_columns(out, ref[:, :S], what)
        assert first.setdefault((chunk, order, S), out.tobytes()) == out.tobytes(), what + " differs from its first occurrence"
    assert len(first) == 24
    ctx.close()


@functools.lru_cache(maxsize=None)
def solve_case(kind, P, noise=None, max_error=1.0):
    N, D, M = 400, 3, 24
    X, Y, hyp = mref.problem(N, D, M, P, seed=11)
    if noise is not None:
        hyp.noise = noise
    cov, terms = orc.dense_cov(kind, X, hyp), orc.common_terms(kind, X, hyp)
    pre = lambda r: orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r)
    V, steps, half = mref.stable_steps(cov, Y - hyp.mean, np.zeros_like(Y), pre, max_error)
    return X, Y, hyp, cov, V, steps, half


@pytest.mark.parametrize("kind", KINDS)
def test_p1_multi_entry_points_equal_single_bitwise(kind):
    X, Y, hyp, cov, Vref, steps, half = solve_case(kind, 1)
    y = Y[:, 0]
    ctx = make_ctx(kind, X, y, hyp, sym_chunk=16)
    ctx.setup()
    p = torch.from_numpy(Vref[:, 0].copy())
    assert ctx.matmat(p).reshape(-1).cpu().numpy().tobytes() == ctx.matvec(p).cpu().numpy().tobytes()
    b, v0 = torch.from_numpy(y - hyp.mean), torch.zeros(len(y), dtype=torch.float64)
    v1, s1, h1 = ctx.pcg(b, v0)
    vm, sm, hm, cols = ctx.pcg_multi(b, v0)
    assert (s1, h1) == (sm, hm) and cols[0] == h1 and vm.reshape(-1).cpu().numpy().tobytes() == v1.cpu().numpy().tobytes()
    Xn = X[:17] + 0.1
    m1, var1 = ctx.predict(v1, Xn)
    mm, varm = ctx.predict_multi(v1, Xn)
    assert mm.reshape(-1).cpu().numpy().tobytes() == m1.cpu().numpy().tobytes() and varm.cpu().numpy().tobytes() == var1.cpu().numpy().tobytes()
    # the evaluation: cglb_objective_and_grad_multi on a p = 1 context against cglb_objective_and_grad
    from cglb_amd.hip_context import grad_len
    va, vb = v0.to(ctx.device).clone(), v0.to(ctx.device).clone()
    r1 = ctx.objective_and_grad(va, True)
    out4, g = (ctypes.c_double * 4)(), np.empty(grad_len(ctx.D, ctx.M))
    st, hf = ctypes.c_int(), ctypes.c_double()
    rc = ctx.lib.cglb_objective_and_grad_multi(ctx._ctx, ctypes.c_void_p(vb.data_ptr()), 1, 1.0, 100, 40, out4,
                                               g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(st), ctypes.byref(hf))
    assert rc == 0 and tuple(out4) == (r1.bound, r1.lower, r1.upper, r1.logdet) and st.value == r1.steps
    assert va.cpu().numpy().tobytes() == vb.cpu().numpy().tobytes()
    assert g.tobytes() == np.concatenate([r1.grad["lengthscales"], [r1.grad["variance"], r1.grad["noise"], r1.grad["mean"]], r1.grad["Z"].reshape(-1)]).tobytes()
    ctx.close()


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_pcg_multi_against_lockstep_loop(kind, P):
    X, Y, hyp, cov, Vref, steps, half = solve_case(kind, P)
    assert 0 < steps <= 40
    ctx = make_ctx(kind, X, Y, hyp, sym_chunk=16)
    ctx.setup()
    V, st, total, cols = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64))
    print(f"steps {st} (ref {steps}); 1/2 r^T P r {cols} (ref {half})")
    assert st == steps
    np.testing.assert_allclose(V.cpu().numpy(), Vref, rtol=0, atol=1e-8 * np.abs(Vref).max())
    np.testing.assert_allclose(cols, half, rtol=1e-5)
    assert total == pytest.approx(half.sum(), rel=1e-5) and total <= 1.0
    ctx.close()


def test_pcg_multi_restart_branch():
    """Small noise and a tolerance of 1e-9: more than 40 steps, so the restart step (exact residuals of all columns) runs."""
    X, Y, hyp, cov, Vref, steps, half = solve_case("rbf", 2, noise=1e-3, max_error=1e-9)
    assert steps > 40
    ctx = make_ctx("rbf", X, Y, hyp, sym_chunk=16)
    ctx.setup()
    V, st, total, cols = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64), max_error=1e-9)
    print(f"steps {st} (ref {steps}); total {total}")
    assert abs(st - steps) <= 1          # the golden tests' allowance beyond 40 steps
    if st == steps:
        np.testing.assert_allclose(V.cpu().numpy(), Vref, rtol=0, atol=1e-4 * np.abs(Vref).max())
    assert total <= 1e-9 or st == 100
    ctx.close()


def test_pcg_multi_column_equal_to_the_mean():
    X, Y, hyp, cov, Vref, steps, half = solve_case("matern32", 3)
    Y4 = np.concatenate([Y[:, :1], np.full((len(Y), 1), hyp.mean), Y[:, 1:]], axis=1)   # same S_pad group as the 3 columns
    ctx = make_ctx("matern32", X, Y, hyp, sym_chunk=16)
    ctx.setup()
    V3, s3, t3, c3 = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64))
    V4, s4, t4, c4 = ctx.pcg_multi(torch.from_numpy(Y4 - hyp.mean), torch.zeros(Y4.shape, dtype=torch.float64))
    V3, V4 = V3.cpu().numpy(), V4.cpu().numpy()
    assert np.isfinite(V4).all() and np.isfinite(c4).all() and not V4[:, 1].any() and c4[1] == 0.0
    assert s4 == s3 and V4[:, [0, 2, 3]].tobytes() == V3.tobytes()
    ctx.close()


def test_single_and_multi_solves_share_one_context():
    """pcg, pcg_multi (P = 3), pcg again, then a one-column evaluation on ONE context: the one loop keeps the scalar slots, the host mirror
    and the weighted-operand state of each column count apart, so the third call repeats the first and the evaluation that of a fresh context."""
    X, Y, hyp, cov, Vref, steps, half = solve_case("rbf", 3)
    y = np.ascontiguousarray(Y[:, 0])
    b1, z1 = torch.from_numpy(y - hyp.mean), torch.zeros(len(y), dtype=torch.float64)

    def evaluate(ctx):
        v = torch.zeros(len(y), dtype=torch.float64, device=ctx.device)
        res = ctx.objective_and_grad(v, True)
        return (v.cpu().numpy().tobytes(), res.steps, res.residual_error, res.bound, res.lower, res.upper, res.logdet) + \
            tuple(np.asarray(res.grad[k]).tobytes() for k in mref.GRAD_KEYS)

    ctx = make_ctx("rbf", X, y, hyp, sym_chunk=16)
    ctx.setup()
    v1, s1, h1 = ctx.pcg(b1, z1, 1e-3)
    assert s1 > 0
    V, sm, total, cols = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64))
    assert sm == steps
    v3, s3, h3 = ctx.pcg(b1, z1, 1e-3)
    assert (s3, h3) == (s1, h1) and v3.cpu().numpy().tobytes() == v1.cpu().numpy().tobytes()
    shared = evaluate(ctx)
    ctx.close()
    fresh_ctx = make_ctx("rbf", X, y, hyp, sym_chunk=16)
    fresh = evaluate(fresh_ctx)
    fresh_ctx.close()
    assert shared == fresh


def test_pcg_multi_lookahead_is_bitwise_neutral():
    """The multi-column twin of test_lookahead_stop_test_does_not_change_results (tests/test_gpu_edge_cases.py): a speculative mat-mat product
    only writes Ap and the p.Ap slots, so V, the steps and the per-column statistics do not depend on the look-ahead rule."""
    X, Y, hyp, cov, Vref, steps, half = solve_case("rbf", 2)
    outs = []
    for la in (0, 1, 2, 8):
        ctx = make_ctx("rbf", X, Y, hyp, sym_chunk=16, pcg_lookahead=la)
        ctx.setup()
        V, st, total, cols = ctx.pcg_multi(torch.from_numpy(Y - hyp.mean), torch.zeros(Y.shape, dtype=torch.float64), max_error=1e-6)
        outs.append((V.cpu().numpy().tobytes(), st, total, cols.tobytes()))
        ctx.close()
    print("steps", outs[0][1], "total", outs[0][2])
    assert outs[0][1] > steps >= 1          # tighter than the default tolerance: several steps
    for other in outs[1:]:
        assert other == outs[0]


def test_eval_profile_counts_multi_column_evaluations():
    """eval_profile counts and times the evaluations of P > 1 columns like the one-column ones, and one that fails after its first mark
    leaves no marks behind (tests/test_gpu_edge_cases.py has the one-column form).  The failing evaluation: a context that holds two
    columns refuses set_option("logdet_bound", 1) itself (asserted below), so require_multi_ok's refusal cannot be reached through the
    options; a singular K_uu without jitter makes cglb_setup fail inside the evaluation instead, after the first mark."""
    X, Y, hyp, cov, Vref, steps, half = solve_case("rbf", 2)
    ctx = make_ctx("rbf", X, Y, hyp, sym_chunk=16)
    ctx.set_option("eval_profile", 1)
    stats = ("eval_setup_ms", "eval_pcg_ms", "eval_final_ms", "eval_grad_ms")
    for _ in range(2):
        res = ctx.objective_and_grad(torch.zeros(Y.shape, dtype=torch.float64, device=ctx.device), True)
        assert np.isfinite(res.bound)
    ms = [ctx.get_stat(k) for k in stats]
    print("eval_count", ctx.get_stat("eval_count"), "eval_*_ms", ms)
    assert ctx.get_stat("eval_count") == 2
    assert all(np.isfinite(t) and t >= 0.0 for t in ms)
    with pytest.raises(ValueError, match="more than one target column"):
        ctx.set_option("logdet_bound", 1)
    Zdup = hyp.Z.copy()
    Zdup[1] = Zdup[0]
    ctx.set_hypers(np.ones(3), 1.0, 0.1, 0.0, Zdup, 0.0)     # k(z, z) = 1 exactly: the second pivot is an exact zero (as in test_error_mapping)
    with pytest.raises(RuntimeError, match="[Cc]holesky"):
        ctx.objective_and_grad(torch.zeros(Y.shape, dtype=torch.float64, device=ctx.device), True)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    res = ctx.objective_and_grad(torch.zeros(Y.shape, dtype=torch.float64, device=ctx.device), True)
    assert np.isfinite(res.bound)
    ms = [ctx.get_stat(k) for k in stats]
    assert ctx.get_stat("eval_count") == 3
    assert all(np.isfinite(t) and t >= 0.0 for t in ms)
    ctx.close()


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_evaluation_at_given_v_and_after_solve(kind, P):
    X, Y, hyp, cov, Vref, steps, half = solve_case(kind, P)
    ctx = make_ctx(kind, X, Y, hyp, sym_chunk=16)
    tot, grad = mref.composed_objective(kind, X, Y, hyp, Vref, cov=cov)
    v = torch.from_numpy(Vref.copy()).to(ctx.device)
    res = ctx.objective_and_grad(v, run_cg=False)
    assert res.bound == pytest.approx(tot["bound"], rel=1e-11)
    assert res.lower == pytest.approx(tot["lower"], rel=1e-9) and res.upper == pytest.approx(tot["upper"], rel=1e-9)
    assert res.logdet == pytest.approx(tot["logdet"], rel=1e-11)
    for key in mref.GRAD_KEYS:
        tol = 1e-8 * max(1.0, np.abs(grad[key]).max())
        if key == "mean":
            tol = 1e-11 * np.abs(Vref).sum()
        np.testing.assert_allclose(np.asarray(res.grad[key]), grad[key], rtol=1e-7, atol=tol, err_msg=key)
    v0 = torch.zeros(Y.shape, dtype=torch.float64, device=ctx.device)
    solved = ctx.objective_and_grad(v0, True)
    assert solved.steps == steps
    assert solved.bound == pytest.approx(tot["bound"], rel=1e-6)          # north-star tolerance of the golden tests
    np.testing.assert_allclose(v0.cpu().numpy(), Vref, rtol=0, atol=1e-8 * np.abs(Vref).max())
    at_v = ctx.objective_and_grad(v0.clone(), run_cg=False)
    for key in mref.GRAD_KEYS:
        np.testing.assert_allclose(np.asarray(solved.grad[key]), at_v.grad[key], rtol=0, atol=1e-6 * np.abs(at_v.grad[key]).max(), err_msg=key)
    ctx.close()


def test_predict_multi_and_predictcg():
    """Reference: the numpy lockstep loop at PredictCG's tolerance (1e-3 on the SUMMED statistic, stop step checked stable), then the
    single-output oracle's prediction per column started AT that V: every column's 1/2 r^T P r is at most the sum, so the oracle's own
    solve takes no step and predicts at exactly the lockstep V.  Tolerances: 1e-8 of the largest entry, as the predict goldens."""
    from cglb_amd.backend.models import CGLB, BaseKernel, GaussianLikelihood, InducingPointKernel, PredictCG, ScaleKernel
    kind = "rbf"
    X, Y, hyp = mref.problem(300, 2, 16, 3, seed=4)
    Xn = np.random.default_rng(9).standard_normal((41, 2))
    cov, terms = orc.dense_cov(kind, X, hyp), orc.common_terms(kind, X, hyp)
    pre = lambda r: orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r)
    Vref, steps, half = mref.stable_steps(cov, Y - hyp.mean, np.zeros_like(Y), pre, 1e-3)
    assert steps > 0
    refs = [orc.predict(kind, X, Y[:, b], hyp, Vref[:, b], Xn) for b in range(3)]
    for b in range(3):
        assert refs[b][3].steps == 0 and refs[b][2].tobytes() == Vref[:, b].tobytes()
    ctx = make_ctx(kind, X, Y, hyp, sym_chunk=16)
    ctx.setup()
    f_mean, f_var = ctx.predict_multi(torch.from_numpy(Vref), Xn)
    for b in range(3):
        np.testing.assert_allclose(f_mean[:, b].cpu().numpy(), refs[b][0], rtol=0, atol=1e-8 * np.abs(refs[b][0]).max())
    np.testing.assert_allclose(f_var.cpu().numpy(), refs[0][1], rtol=0, atol=1e-8 * np.abs(refs[0][1]).max())
    ctx.close()
    kernel = InducingPointKernel(ScaleKernel(BaseKernel(kind, 2)), hyp.Z)
    kernel.base_kernel.base_kernel.lengthscale = hyp.lengthscales.reshape(1, -1)
    kernel.base_kernel.outputscale = hyp.variance
    lik = GaussianLikelihood()
    lik.noise = hyp.noise
    model = CGLB((X, Y), lik, kernel)
    with torch.no_grad():
        model.mean_module.constant.fill_(hyp.mean)
    pred = PredictCG(model)
    pm, pv = pred(torch.from_numpy(Xn))
    assert tuple(pm.shape) == (41, 3) and tuple(pv.shape) == (41, 3) and tuple(pred.v_vec.shape) == (300, 3)
    np.testing.assert_allclose(pred.v_vec.cpu().numpy(), Vref, rtol=0, atol=1e-8 * np.abs(Vref).max())
    for b in range(3):
        np.testing.assert_allclose(pm[:, b].cpu().numpy(), refs[b][0], rtol=0, atol=1e-8 * np.abs(refs[b][0]).max())
        np.testing.assert_allclose(pv[:, b].cpu().numpy(), refs[0][1], rtol=0, atol=1e-8 * np.abs(refs[0][1]).max())
    model.hip.close()


def test_fallback_paths_give_the_same_answers():
    # D = 40 (wide inputs, fp64): S single mat-vecs; held to the product's own tolerance
    X, _y, hyp, _p = gc.problem(300, 40, seed=2)
    V = np.random.default_rng(1).standard_normal((300, 3))
    ref = orc.dense_cov("rbf", X, hyp) @ V
    ctx = make_ctx("rbf", X, np.zeros(300), hyp)
    check_columns(ctx.matmat(torch.from_numpy(V)).cpu().numpy(), ref, "D=40")
    ctx.close()
    # a forced non-symmetric variant: the same
    X, hyp, V, ref = matmat_case("rbf", 300, 8)
    ctx = make_ctx("rbf", X, np.zeros(300), hyp, kff_variant=0)
    check_columns(ctx.matmat(torch.from_numpy(V[:, :3].copy())).cpu().numpy(), ref[:, :3], "kff_variant 0")
    ctx.close()
    # fp32 context: every column to the fp32 round-off model of the single mat-vec (tests/geometry_cases.py, tests/test_gpu_fp32_parity.py)
    X, _y, hyp, p = gc.problem(300, 3, seed=3)
    W = np.stack([p, p[::-1].copy(), np.roll(p, 7)], axis=1)
    ctx = make_ctx("rbf", X, np.zeros(300), hyp, dtype=torch.float32, sym_chunk=16)
    out = ctx.matmat(torch.from_numpy(W)).cpu().numpy().astype(np.float64)
    for b in range(3):
        ref_b, s, bound = gc.reference("rbf", "fp32", X, hyp, W[:, b].copy(), 16)
        gc.check(out[:, b], ref_b, s, bound, f"fp32 column {b}")
    # and the batched solve / evaluation run there too
    Y = np.stack([np.sin(X[:, 0]), np.cos(X[:, 1]), X[:, 2]], axis=1)
    ctx.set_targets(torch.from_numpy(Y))
    res = ctx.objective_and_grad(torch.zeros((300, 3), dtype=torch.float32, device=ctx.device), True)
    tot, _ = mref.composed_objective("rbf", X, Y, hyp, np.zeros_like(Y), with_grad=False)
    assert np.isfinite(res.bound) and res.bound >= tot["bound"] - 1.0   # the solve closes the gap left at v = 0 to within max_error
    ctx.close()


def test_refusals_leave_the_context_usable():
    from cglb_amd import _lib
    X, hyp, V, ref = matmat_case("rbf", 300, 3)
    Y2 = torch.from_numpy(V[:, :2].copy()).t().contiguous().cuda()
    ptr = ctypes.c_void_p(Y2.data_ptr())
    ctx = make_ctx("rbf", X, np.zeros(300), hyp)
    lib = ctx.lib
    assert lib.cglb_set_parallel(ctx._ctx, 2, 0) == _lib.OK
    assert lib.cglb_set_targets(ctx._ctx, ptr, 2) == _lib.ERR_BAD_ARG
    assert lib.cglb_set_parallel(ctx._ctx, 1, 0) == _lib.OK
    ctx.set_option("logdet_bound", 1)
    assert lib.cglb_set_targets(ctx._ctx, ptr, 2) == _lib.ERR_BAD_ARG
    ctx.set_option("logdet_bound", 0)
    assert lib.cglb_set_targets(ctx._ctx, ptr, 2) == _lib.OK
    assert lib.cglb_set_parallel(ctx._ctx, 2, 0) == _lib.ERR_BAD_ARG
    assert lib.cglb_set_option(ctx._ctx, b"logdet_bound", 1) == _lib.ERR_BAD_ARG
    assert lib.cglb_set_option(ctx._ctx, b"quad_term", 1) == _lib.ERR_BAD_ARG
    check_columns(ctx.matmat(torch.from_numpy(V[:, :2].copy())).cpu().numpy(), ref[:, :2], "after the refusals")
    ctx.close()


def test_backend_optimize_and_cli_round_trip(tmp_path):
    from cglb_amd.backend.models import CGLB, BaseKernel, GaussianLikelihood, InducingPointKernel, LowerBoundCG, ScaleKernel
    from cglb_amd.cli import get_dataset
    data = get_dataset("synthetic-400-3-2")
    X, Y = np.asarray(data.train[0]), np.asarray(data.train[1])
    assert Y.shape[1] == 2
    Z = X[:16].copy()
    hyp = orc.reference_init_hypers(3, Z)
    kernel = InducingPointKernel(ScaleKernel(BaseKernel("rbf", 3)), Z)
    kernel.base_kernel.base_kernel.lengthscale = hyp.lengthscales.reshape(1, -1)
    kernel.base_kernel.outputscale = hyp.variance
    lik = GaussianLikelihood()
    lik.noise = hyp.noise
    model = CGLB((X, Y), lik, kernel)
    bound = LowerBoundCG(model)
    params = [p for p in model.parameters()]
    loss0 = -bound(None)
    g0 = torch.autograd.grad(loss0, params, allow_unused=True)
    V = model.v_vec.detach().cpu().numpy()
    tot, grad = mref.composed_objective("rbf", X, Y, hyp, V)
    assert float(loss0) == pytest.approx(-tot["bound"], rel=1e-9)
    # gradient of the loss wrt the raw parameters = -(constrained gradient of the bound) x d value / d raw; value = softplus(raw) + bound
    # for lengthscales, variance and noise (d/d raw = sigmoid(raw)), the mean and Z are their own raw parameters
    named = dict(zip([n for n, _ in model.named_parameters()], g0))
    assert len(named) == 5

    def raw(suffix):
        (key,) = [k for k in named if k.endswith(suffix)]
        return dict(model.named_parameters())[key].detach(), named[key].numpy()
    got = {}
    for key, suffix in (("lengthscales", "base_kernel.base_kernel._lengthscale.raw"), ("variance", "_outputscale.raw"), ("noise", "_noise.raw")):
        p, g = raw(suffix)
        got[key] = (-g / torch.sigmoid(p).numpy()).reshape(np.shape(grad[key]))
    got["mean"] = -raw("mean_module.constant")[1]
    got["Z"] = -raw("inducing_points")[1]
    for key in mref.GRAD_KEYS:   # the tolerances of the golden evaluation test; the shared mean's entry is the sum over the columns
        tol = 1e-8 * max(1.0, np.abs(grad[key]).max())
        if key == "mean":
            tol = 1e-11 * max(1.0, np.abs(V).sum())
        np.testing.assert_allclose(got[key], grad[key], rtol=1e-7, atol=tol, err_msg=key)
    model.hip.close()
    # a short optimize run through the command tree (a few L-BFGS steps) decreases the loss; metric then round-trips with the same name
    from click.testing import CliRunner
    from cglb_amd.backend import jsonio
    from cglb_amd.cli import main
    logdir = str(tmp_path / "run")
    model_args = ["cglb", "-k", "SquaredExponential", "-m", "cglb", "-i", "cv", "-M", "16"]
    r = CliRunner().invoke(main, ["-b", "hip", "-t", "fp64", "-l", logdir, "-s", "0", "train", "-d", "synthetic-400-3-2", "-n", "8"] + model_args,
                           catch_exceptions=False)
    assert r.exit_code == 0, r.output
    logs = jsonio.load(os.path.join(logdir, "logs.json"))
    results = jsonio.load(os.path.join(logdir, "results.json"))
    # the logger evaluates the metrics at every 20th accepted iterate: with 8 steps the log holds the loss after the first one, and
    # results.json the loss of the model the run ends with
    first, last = float(np.asarray(logs["loss"], dtype=np.float64).reshape(-1)[0]), float(results["loss"])
    print("loss after the first step", first, "after the last", last)
    assert last < first and np.isfinite(results["test/rmse"]) and np.isfinite(results["test/nlpd"])
    r2 = CliRunner().invoke(main, ["-b", "hip", "-t", "fp64", "-l", logdir, "metric", "-d", "synthetic-400-3-2"] + model_args +
                            ["-p", os.path.join(logdir, "model.json")], catch_exceptions=False)
    assert r2.exit_code == 0, r2.output
    assert os.path.exists(os.path.join(logdir, "metric.npy"))
