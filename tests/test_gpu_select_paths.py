"""cglb_select_inducing against the path-following longdouble reference of tests/select_cases.py: for every case, kind and dtype of the table the
library's own picks are followed in np.longdouble and held to the instance's tolerance (regret at every step, trace), next to what is exact
on the device (gather, tie rule, first pick, sign and zero of the trace, equality across row ranges and after stale hyper-parameters)."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import select_cases as sc

pytestmark = pytest.mark.gpu


def _torch_dtype(inst):
    return torch.float64 if inst.dtype == "f64" else torch.float32


def _ctx(inst, p, **kw):
    from cglb_amd.hip_context import HipContext
    return HipContext(p.X, np.zeros(p.N), p.M, inst.kind, dtype=_torch_dtype(inst), **kw)


def _select(inst, p, **kw):
    ctx = _ctx(inst, p, **kw)
    try:
        idx, trace, Z = ctx.select_inducing(p.ls, p.var, jitter=p.jitter, return_Z=True)
        return idx, trace, Z.cpu().numpy()
    finally:
        ctx.close()


def _check(inst, p, idx, trace, label=""):
    """Regret at every step, uniqueness, trace and the exact properties of one result; prints the figures first."""
    assert len(idx) == p.picks and ((0 <= idx) & (idx < p.N)).all() and np.isfinite(trace)
    v = sc.judge(inst, p, idx, trace)
    print(f"{inst.id}{label}: largest regret {v.worst_regret:.3g} tol (step {v.worst_step}), trace error {v.trace_err:.3g} N tol, "
          f"{v.multi} multi-candidate steps of {len(idx)}")
    assert v.worst_regret <= 1.0, f"step {v.worst_step}: regret {v.worst_regret:.3g} tol"
    assert v.unique_ok
    assert v.trace_err <= 1.0
    assert sc.exact_violations(p, idx, trace) == []
    return v


@pytest.mark.parametrize("inst", sc.INSTANCES, ids=[i.id for i in sc.INSTANCES])
def test_library_path_is_admissible(inst):
    p = sc.problem(inst)
    sc.check_geometry(inst, p)
    idx, trace, Z = _select(inst, p)
    assert Z.dtype == inst.np_dtype and Z.shape == (p.picks, p.X.shape[1])
    np.testing.assert_array_equal(Z, p.X[idx].astype(inst.np_dtype))       # the gather, bitwise in the context's type
    _check(inst, p, idx, trace)
    if inst.case == "O1":   # M = N + 5: min(M, N) picks, all distinct, nothing left
        assert len(idx) == p.N and len(np.unique(idx)) == p.N and 0.0 <= trace <= p.N * sc.tol(inst, p.var)


@pytest.mark.parametrize("ident", ["G2-matern52-f32", "W2-matern32-f64"])
def test_null_outputs(ident):
    """Z_out = NULL and, through the raw entry, trace_out = NULL: the same indices as with both outputs."""
    inst = sc.by_id(ident)
    p = sc.problem(inst)
    idx_ref, trace_ref, _ = _select(inst, p)
    ctx = _ctx(inst, p)
    try:
        idx, trace = ctx.select_inducing(p.ls, p.var, jitter=p.jitter)        # Z_out = NULL
        np.testing.assert_array_equal(idx, idx_ref)
        assert trace == trace_ref
        raw = np.full(p.picks, -1, dtype=np.int64)
        ls = np.ascontiguousarray(p.ls, dtype=np.float64)
        rc = ctx.lib.cglb_select_inducing(ctx._ctx, ls.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(p.var), float(p.jitter),
                                          raw.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None, None)
        assert rc == 0
        np.testing.assert_array_equal(raw, idx_ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("ident", ["G4-matern32-f64", "G1-rbf-f32", "G5s-rbf-f32"])
def test_row_range_does_not_change_the_answer(ident):
    """S1: contexts over (0, N), (37, N), (N / 2, N) and an empty range give bitwise equal indices, Z and trace."""
    inst = sc.by_id(ident)
    p = sc.problem(inst)
    ref = _select(inst, p, row_range=(0, p.N))
    _check(inst, p, ref[0], ref[1])
    for rr in ((37, p.N), (p.N // 2, p.N), (p.N, p.N)):
        idx, trace, Z = _select(inst, p, row_range=rr)
        np.testing.assert_array_equal(idx, ref[0], err_msg=str(rr))
        np.testing.assert_array_equal(Z, ref[2], err_msg=str(rr))
        assert trace == ref[1], rr


@pytest.mark.parametrize("ident", ["G3-matern52-f64", "G2-matern32-f32", "W1-rbf-f64"])
def test_stale_hypers_do_not_leak(ident):
    """H1: after set_hypers with ten times the lengthscales and another variance the selection under the case's own values equals the one on a
    fresh context bitwise; setup() is then refused until set_hypers is called again, after which the common terms equal a fresh context's."""
    inst = sc.by_id(ident)
    p = sc.problem(inst)
    fresh = _select(inst, p)
    _check(inst, p, fresh[0], fresh[1])
    Z0, noise = p.X[:p.picks].copy(), 0.3
    used, clean = _ctx(inst, p), _ctx(inst, p)
    try:
        used.set_hypers(10.0 * p.ls, 0.37 * p.var, noise, 0.0, Z0, 1e-6)
        used.setup()
        idx, trace, Z = used.select_inducing(p.ls, p.var, jitter=p.jitter, return_Z=True)
        np.testing.assert_array_equal(idx, fresh[0])
        np.testing.assert_array_equal(Z.cpu().numpy(), fresh[2])
        assert trace == fresh[1]
        with pytest.raises(RuntimeError, match="call order"):
            used.setup()
        for c in (used, clean):
            c.set_hypers(p.ls, p.var, noise, 0.0, p.X[idx], 1e-6)
            c.setup()
        for which in ("L", "LB", "A"):
            np.testing.assert_array_equal(used.get_matrix(which).cpu().numpy(), clean.get_matrix(which).cpu().numpy(), err_msg=which)
    finally:
        used.close()
        clean.close()


def test_iterative_class_reselects_under_the_current_hypers():
    """The iterative exact-GP class (N 257, D 3, k 9, jitter 1e-6): every evaluation re-selects Z under the current hyper-parameters.  The library
    exposes no Z, so the evaluation's L is compared with chol(K_uu + jitter I) of the picks cglb_select_inducing makes under the same values,
    which pass the regret check.  Bound on L: first-order perturbation of a Cholesky factor, |dL| <~ cond(K_uu) |dK| / |K| |L| with the stated
    kernel-value error 1e-13 and k eps for the factorisation, times k for entries against norms; a wrong pick moves L by O(sqrt(variance))."""
    from cglb_amd.hip_context import HipContext
    insts = [sc.by_id("I1a-rbf-f64"), sc.by_id("I1b-rbf-f64")]
    probs = [sc.problem(i) for i in insts]
    N, k = probs[0].N, probs[0].M
    np.testing.assert_array_equal(probs[0].X, probs[1].X)
    y = np.sin(probs[0].X.sum(axis=1))
    eps = np.random.default_rng(0).standard_normal((2, k + N))
    picks = []
    ctx = HipContext(probs[0].X, y, k, "rbf")
    try:
        for inst, p in zip(insts, probs):
            idx, trace, _ = _select(inst, p)
            _check(inst, p, idx, trace)
            picks.append(idx)
            ctx.set_hypers(p.ls, p.var, 0.2, 0.0, p.X[:k].copy(), p.jitter)     # Z is a placeholder: the class selects its own
            v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
            ctx.itergp_objective_and_grad(eps, v, max_error=1e-6, with_grad=False)
            L = ctx.get_matrix("L").cpu().numpy()
            Kuu = sc.kernel_fn(inst.kind, p.ls, p.var)(p.X[idx], p.X[idx], full_cov=True) + p.jitter * np.eye(k)
            Lref = sla.cholesky(Kuu, lower=True)
            bound = k * np.linalg.cond(Kuu) * (sc.KV64 + k * np.finfo(np.float64).eps) * np.abs(Lref).max()
            err = np.abs(np.tril(L) - Lref).max()
            print(f"{inst.id}: |L - chol(K_uu)| {err:.3g}, bound {bound:.3g}")
            assert err <= bound
        assert not np.array_equal(picks[0], picks[1])     # the two evaluations had different preconditioner points to find
    finally:
        ctx.close()
