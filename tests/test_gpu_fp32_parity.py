"""fp32 kernels at fp32 round-off: every case builds an fp32 context on inputs rounded through float32 and compares each output entry
with the fp64 reference on the same values, |out - ref| <= TAU[q] * s (tests/fp32_error_model.py).

Every case is a function returning {quantity: max_i |err_i| / s_i}; the tests assert each ratio against its tau and
tools/fp32_error_ratios.py runs the same functions to record the ratios (profiles/fp32_error_ratios.json)."""
import math
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import fp32_error_model as em
from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu

KINDS = em.KINDS
MATVEC_D = em.MATVEC_D
_problem = em.problem


def _ctx(kind, X32, y32, hyp, row_range=None, **opts):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X32, y32, hyp.Z.shape[0], kind, dtype=torch.float32, row_range=row_range)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    return ctx


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _f(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


# --------------------------------------------------------------------------- K_ff mat-vec
def matvec_sweep_case(D, N, kind, variants=(0, 2), chunk=0):
    X32, y32, hyp, p32 = _problem(N, D)
    opts = {"sym_chunk": chunk} if chunk else {}
    ctx = _ctx(kind, X32, y32, hyp, **opts)
    case = em.matvec_case(kind, X32, hyp, p32, chunk=chunk or None)
    out = {}
    for var in variants:
        ctx.set_option("kff_variant", var)
        out[f"matvec_v{var}"] = em.ratio(_np(ctx.matvec(_f(p32))), case.ref, case.s)
    ctx.close()
    return out


def _matvec_cases():
    return [(f"matvec-{kind}-D{D}-N{N}" + (f"-c{chunk}" if chunk else ""), matvec_sweep_case, dict(D=D, N=N, kind=kind, chunk=chunk))
            for kind, D, N, chunk in em.matvec_shapes()]


# --------------------------------------------------------------------------- row shards, cyclic partials
def shard_case(D, kind, r0, r1):
    N = 2999
    X32, y32, hyp, p32 = _problem(N, D, seed=7)
    ctx = _ctx(kind, X32, y32, hyp, row_range=(r0, r1))
    case = em.matvec_case(kind, X32, hyp, p32, r0=r0, r1=r1)
    out = {}
    for var in (0, 2):
        ctx.set_option("kff_variant", var)
        out[f"matvec_v{var}"] = em.ratio(_np(ctx.matvec(_f(p32))), case.ref, case.s)
    ctx.close()
    return out


def cyclic_case(D, kind, world):
    from cglb_amd import _lib
    N = 2999
    X32, y32, hyp, p32 = _problem(N, D, seed=8)
    ctx = _ctx(kind, X32, y32, hyp)
    case = em.matvec_case(kind, X32, hyp, p32, chunk=em.sym_chunk(N, D, world))
    p = _f(p32).to(ctx.device)
    total = np.zeros(N)
    s_parts = np.zeros(N)
    for rank in range(world):
        _lib.check(ctx.lib.cglb_set_parallel(ctx._ctx, world, rank), ctx._ctx)
        part = torch.empty(N, dtype=torch.float32, device=ctx.device)
        _lib.check(ctx.lib.cglb_matvec_cyclic(ctx._ctx, c_void_p(p.data_ptr()), c_void_p(part.data_ptr())), ctx._ctx)
        part = _np(part)
        total += part
        s_parts += em.U * np.abs(part)  # the sum of the partials (in fp64 here, in fp32 by the caller's all-reduce)
    ctx.close()
    return {"matvec": em.ratio(total, case.ref, case.s + s_parts)}


# --------------------------------------------------------------------------- exponent range, near-duplicates, offset data
def edge_case(kind, hw=None, ls=1.0, offset=0.0, dup=False):
    X32, y32, hyp, p32 = em.edge_problem(hw, ls, offset, dup)
    ctx = _ctx(kind, X32, y32, hyp)
    case = em.matvec_case(kind, X32, hyp, p32)
    out = {}
    for var in (0, 2):
        ctx.set_option("kff_variant", var)
        o = _np(ctx.matvec(_f(p32)))
        assert np.isfinite(o).all()
        out[f"matvec_v{var}"] = em.ratio(o, case.ref, case.s)
    ctx.close()
    return out


# --------------------------------------------------------------------------- cross mat-vec, setup panels, preconditioner
def panels_case(kind, D, N=1500, M=8):
    X32, y32, hyp, v32 = _problem(N, D, M=M, seed=3)
    ctx = _ctx(kind, X32, y32, hyp)
    ctx.setup()
    out = {}
    for n_new in (1, 77, 1000):
        Xn = em.f32(np.random.default_rng(n_new).standard_normal((n_new, D)))
        ref, s = em.cross_case(kind, X32, hyp, Xn, v32)
        out[f"cross_n{n_new}"] = em.ratio(_np(ctx.cross_matvec(_f(Xn), _f(v32))), ref, s)
    terms, sA, sL = em.setup_case(kind, X32, hyp)
    A, L, LB = _np(ctx.get_matrix("A")), _np(ctx.get_matrix("L")), _np(ctx.get_matrix("LB"))
    out["A"] = em.ratio(A, terms.A, sA)
    out["L"] = em.ratio(np.tril(L), terms.L, sL)
    r32 = em.f32(np.random.default_rng(5).standard_normal(N))
    z_ref, s_z = em.precond_case(A, np.tril(LB), hyp.noise, r32)  # the apply alone: on the context's own A and LB
    z, _ = ctx.precond(_f(r32))
    out["precond"] = em.ratio(_np(z), z_ref, s_z)
    ctx.close()
    return out


# --------------------------------------------------------------------------- gradient and bound at a fixed v
def _well_separated_Z(X32, M):
    """M points of X spread out (greedy farthest point): cond(K_uu) = O(1)."""
    idx = [0]
    d = np.sum((X32 - X32[0]) ** 2, axis=1)
    for _ in range(M - 1):
        idx.append(int(np.argmax(d)))
        d = np.minimum(d, np.sum((X32 - X32[idx[-1]]) ** 2, axis=1))
    return X32[idx].copy()


def grad_case(kind, D, N=1500, M=6, random_Z=False):
    """random_Z: the inputs of test_gpu_fp32.py (M = 32 data points as Z, trained-like hypers, noise 0.5, fp32 jitter): cond(K_uu)
    is large there and the small-M algebra dominates the Z block - the same taus hold those checks, so they are calibrated here too."""
    if random_Z:
        X, y, Z = orc.synthetic_problem(N, D, M, seed=21)
        hyp = em.round_hypers(orc.trained_like_hypers(D, Z))
        hyp.noise, hyp.jitter = 0.5, 1e-5
        X32, y32 = em.f32(X), em.f32(y)
    else:
        X32, y32, hyp, _ = _problem(N, D, M=M, seed=4)
        hyp.Z = _well_separated_Z(X32, M)
    v64 = orc.objective(kind, X32, y32, hyp, np.zeros(N), True, 1.0 if random_Z else 1e-3).v
    v32 = em.f32(v64)
    g, sg, w = em.grad_case(kind, X32, y32, hyp, v32)
    bref = orc.objective(kind, X32, y32, hyp, v32, run_cg=False)
    s_b = em.bound_scale(kind, X32, y32, hyp, v32, w)
    ctx = _ctx(kind, X32, y32, hyp)
    v = _f(v32).to(ctx.device)
    res = ctx.objective_and_grad(v, run_cg=False, with_grad=True)
    ctx.close()
    return {"grad_ls": em.ratio(res.grad["lengthscales"], g["lengthscales"], sg["lengthscales"]),
            "grad_Z": em.ratio(res.grad["Z"], g["Z"], sg["Z"]),
            "bound": abs(res.bound - bref.bound) / s_b}


def predict_case(kind, D=5, N=1500, M=6):
    X32, y32, hyp, _ = _problem(N, D, M=M, seed=6)
    hyp.Z = _well_separated_Z(X32, M)
    v32 = em.f32(orc.objective(kind, X32, y32, hyp, np.zeros(N), True, 1e-3).v)
    Xn = em.f32(np.random.default_rng(9).standard_normal((333, D)))
    fm, fv, sm, sv = em.predict_case(kind, X32, y32, hyp, v32, Xn)
    ctx = _ctx(kind, X32, y32, hyp)
    ctx.setup()
    m, var = ctx.predict(_f(v32), _f(Xn))
    ctx.close()
    return {"f_mean": em.ratio(_np(m), fm, sm), "f_var": em.ratio(_np(var), fv, sv)}


def _cases():
    cases = _matvec_cases()
    for D in (8, 24):
        for kind in KINDS:
            for r0, r1 in em.SHARDS:
                cases.append((f"shard-{kind}-D{D}-{r0}-{r1}", shard_case, dict(D=D, kind=kind, r0=r0, r1=r1)))
    for world in (2, 3):
        for kind in KINDS:
            cases.append((f"cyclic-{kind}-w{world}", cyclic_case, dict(D=8, kind=kind, world=world)))
    for kind in KINDS:
        for label, kw in em.EDGE_CASES:
            cases.append((f"edge-{kind}-{label}", edge_case, dict(kind=kind, **kw)))
        for D in (3, 12, 24):
            cases.append((f"panels-{kind}-D{D}", panels_case, dict(kind=kind, D=D)))
        for D in (12, 24):  # the gradient pass's R = 2 (DP <= 16, packed) and R = 1 (DP > 16) instances
            cases.append((f"grad-{kind}-D{D}", grad_case, dict(kind=kind, D=D)))
        for D in (3, 8, 12, 16, 24):
            cases.append((f"grad-{kind}-D{D}-M32-randomZ", grad_case, dict(kind=kind, D=D, M=32, random_Z=True)))
        cases.append((f"predict-{kind}", predict_case, dict(kind=kind)))
    return cases


CASES = _cases()


def tau_of(q):
    return em.TAU[em.quantity(q)]


@pytest.mark.parametrize("name,fn,kw", CASES, ids=[c[0] for c in CASES])
def test_fp32_within_round_off(name, fn, kw):
    ratios = fn(**kw)
    bad = {q: r for q, r in ratios.items() if not r <= tau_of(q)}
    assert not bad, f"{name}: max |err| / s above tau: {bad} (tau {em.TAU})"


# --------------------------------------------------------------------------- precision levels and final_matvec
def test_precision_option_is_a_no_op_in_fp32():
    """CGLB_DISPATCH_PREC forces the exact level for float: precision 0 / 1 / 2 give bitwise-identical results."""
    kind, N, D = "matern32", 2000, 5
    X32, y32, hyp, p32 = _problem(N, D, seed=2)
    ctx = _ctx(kind, X32, y32, hyp)
    v = _f(em.f32(0.1 * p32)).to(ctx.device)
    got = []
    for prec in (0, 1, 2):
        ctx.set_option("precision", prec)
        mv = _np(ctx.matvec(_f(p32)))
        res = ctx.objective_and_grad(v.clone(), run_cg=False, with_grad=True)
        got.append((mv, res.bound, res.grad["lengthscales"], res.grad["Z"]))
    ctx.close()
    for g in got[1:]:
        assert np.array_equal(g[0], got[0][0])
        assert g[1] == got[0][1]
        assert np.array_equal(g[2], got[0][2]) and np.array_equal(g[3], got[0][3])


FINAL_MATVEC_PROBLEMS = {"rbf": (1000, 3, 32), "matern32": (1000, 2, 32)}  # (N, D, M): 59 / 48 fp64 PCG steps at noise 0.02


def final_matvec_case(kind):
    """A solve that crosses the restart (step 40) and ends before step 80; the bound with K v from the recurrence residual
    (final_matvec 0, the default) against the recomputed one (1), both against the fp64 oracle at the upcast fp32 v."""
    N, D, M = FINAL_MATVEC_PROBLEMS[kind]
    X, y, Z = orc.synthetic_problem(N, D, M, seed=5)
    X32, y32 = em.f32(X), em.f32(y)
    hyp = orc.Hypers(np.ones(D), 1.0, 0.02, 0.0, em.f32(Z), 1e-5)
    out = {}
    for fm in (0, 1):
        ctx = _ctx(kind, X32, y32, hyp, final_matvec=fm)
        v = torch.zeros(N, dtype=torch.float32, device=ctx.device)
        res = ctx.objective_and_grad(v, run_cg=True, max_error=1e-3, with_grad=False)
        v32 = _np(v)
        ctx.close()
        ref = orc.objective(kind, X32, y32, hyp, v32, run_cg=False)
        w = orc.nystrom_precond(*(lambda t: (t.A, t.LB))(orc.common_terms(kind, X32, hyp)), hyp.noise,
                                (y32 - hyp.mean) - orc.dense_cov(kind, X32, hyp) @ v32)[0]
        out[fm] = dict(steps=res.steps, floor=em.bound_scale(kind, X32, y32, hyp, v32, w),
                       bound=abs(res.bound - ref.bound), lower=abs(res.lower - ref.lower), upper=abs(res.upper - ref.upper))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_final_matvec_default_in_fp32(kind):
    out = final_matvec_case(kind)
    for fm in (0, 1):
        assert 41 <= out[fm]["steps"] <= 79, out
    for q in ("bound", "lower", "upper"):
        # the default form is no farther from the oracle than a small multiple of the recomputed form plus the model's floor
        assert out[0][q] <= 4.0 * out[1][q] + em.TAU["bound"] * out[0]["floor"], (q, out)
        assert out[1][q] <= em.TAU["bound"] * out[1]["floor"], (q, out)
