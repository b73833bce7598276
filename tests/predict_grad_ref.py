"""References, tolerances, case tables and planted defects of the input gradients of the CGLB / SGPR / exact-GP predictive (test helper, not a
test module; runs on any CPU).  Shared by tests/test_predict_grad_ref_host.py and tests/test_gpu_predict_grad.py.

    weighted_product     out_u, gout_u, out_w, gout_w of cglb_cross_grad_weighted in np.longdouble on input_grad_ref.cross_terms
    cglb_predict_grad    (mean, g_mean, var, g_var) of cglb_predict_grad, twice: `analytic` in the library's algebra
                           q = L^-T LB^-T c,  C^T = L^-T (tmp1 - LB^-T tmp2),  g_mean = grad(K_*f v) + sum_m q_m dk,  g_var = -2 sum_m C^T[m, i] dk
                         and `autograd`: torch.autograd in fp64 through the textbook form of predict_ref.sgpr_predict extended by K_*f v and res
    gpr_predict_grad     the same pair for cglb_gpr_predict_grad: alpha and C = K^-1 K_f* / autograd through the dense solve

dk(x*, p)/dx*_k = -f h delta_k / l_k, delta_k = (x*_k - p_k) / l_k, h the factor of input_grad_ref.profiles.  The kernels are restated here for the
three kinds (the oracle has no Matern-5/2); problems and new points are predict_ref.problem / predict_ref.xnew (JITTER 1e-4; new points on training
rows, on inducing points, the far point).

Tolerances.
* product: input_grad_ref.cross_tolerance's rule with the pair's own weight in the place of |V_js|: 1e-11 f sum_m |w_mi| |h delta_k / l_k| per gradient
  element, 1e-11 f sum_m |w kappa| per value, each plus the clamp floor times f sum |w| - the same kernel-value accuracy, the same direct differences.
* predictors: 1e-8 max(max |reference array|, G_k) - the 1e-8 of the largest reference entry predict_ref and tests/test_gpu_gpr.py hold these
  predictors to - with G_k = sqrt(C f) / l_k for g_mean and f sqrt(C) / l_k for g_var (input_grad_ref.solve_bound / gvar_tolerance, C_KIND), so that
  an all-zero reference does not demand exact zeros of the K_*f v term.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import scipy.linalg as sla
import torch

import input_grad_ref as ig
import predict_ref as pr
import slab_rules

LD = np.longdouble
TOL_PREDICT = 1e-8
ROW_CHUNK = 256      # new points per block of the dense [n, n_pts, d] terms


# ---- kernels, numpy and torch ------------------------------------------------------------------------------------------------------------------
def kernel(kind, A, B, ls, f):
    """f kappa(A, B) [len(A), len(B)], float64, direct differences."""
    diff = (np.asarray(A, dtype=np.float64)[:, None, :] - np.asarray(B, dtype=np.float64)[None, :, :]) / np.asarray(ls, dtype=np.float64)
    return f * ig.profiles(kind, (diff * diff).sum(axis=2))[0].astype(np.float64)


def _torch_kernel(kind, A, B, ls, f):
    diff = (A[:, None, :] - B[None, :, :]) / ls
    d2 = (diff * diff).sum(dim=2)
    if kind == "rbf":
        return f * torch.exp(-0.5 * d2)
    r = torch.sqrt(torch.clamp(d2, min=1e-300))   # a coincident pair: r ~ 0 and no gradient through the clamp
    if kind == "matern32":
        s = math.sqrt(3.0) * r
        return f * (1 + s) * torch.exp(-s)
    if kind == "matern52":
        s = math.sqrt(5.0) * r
        return f * (1 + s + s * s / 3) * torch.exp(-s)
    raise ValueError(kind)


def _rows(n):
    return [(a, min(a + ROW_CHUNK, n)) for a in range(0, n, ROW_CHUNK)]


# ---- launch geometry (csrc/kernels_predict_grad.hip) ----------------------------------------------------------------------------------------------
ROWS = 4096


def rows_per_lane(d: int) -> int:
    dp = ig.pad_dim(d)
    return 4 if dp <= 4 else (2 if dp <= 8 else 1)


def rows_per_block(d: int) -> int:
    return 256 * rows_per_lane(d)


def weighted_split(n_rows: int, n_pts: int, d: int, forced: int = 0):
    """(chunks, chunk length) of one launch (n_rows <= ROWS): the kff_jsplit rule without the even rounding, capped by the slab of the two-weight
    instance."""
    bx = (n_rows + rows_per_block(d) - 1) // rows_per_block(d)
    return slab_rules.pair_split(forced, bx, n_pts, slab_rules.slot_cap(n_rows, 2 * (ig.pad_dim(d) + 1)), even=False)


# ---- the product ------------------------------------------------------------------------------------------------------------------------------
PRODUCT_DEFECTS = ("sign", "inv_l", "m32_for_m52", "coincident_nonzero", "drop_chunk_last", "swap_uw", "ld_wrong", "lost_rows")


def _pair_terms(kind, xnew, P, ls, defect=None, chunk=None):
    """(kappa [n, n_pts], w [n, n_pts, d]) of input_grad_ref.cross_terms, with the pair-level defects of input_grad_ref.cross_grad."""
    lsd = np.asarray(ls, dtype=LD).reshape(-1)
    kap, w = ig.cross_terms("matern32" if (defect == "m32_for_m52" and kind == "matern52") else kind, xnew, P, ls)
    diff = np.asarray(xnew, dtype=LD)[:, None, :] - np.asarray(P, dtype=LD)[None, :, :]
    if defect == "m32_for_m52" and kind == "matern52":   # the factor 3 e^(-s) at Matern-5/2's own s = sqrt5 r
        s = np.sqrt(LD(5) * ((diff / lsd) ** 2).sum(axis=2))
        w = (3 * np.exp(-s))[:, :, None] * diff / lsd / lsd
        kap = ig.profiles(kind, ((diff / lsd) ** 2).sum(axis=2))[0]
    if defect == "inv_l":
        w = w * lsd
    if defect == "coincident_nonzero":   # delta / r taken as 1 at r = 0
        hit = (diff == 0).all(axis=2)
        w = w + np.where(hit, ig.profiles(kind, np.zeros(hit.shape))[1], 0)[:, :, None] / lsd
    if defect == "drop_chunk_last":
        w, kap = w.copy(), kap.copy()
        j = min(chunk, len(P)) - 1
        w[:, j, :] = 0
        kap[:, j] = 0
    if defect == "lost_rows":            # the points m >= 32 floor((n_pts - 1) / 32)
        w, kap = w.copy(), kap.copy()
        m0 = 32 * ((len(P) - 1) // 32)
        w[:, m0:, :] = 0
        kap[:, m0:] = 0
    return kap, w


def weighted_product(kind, xnew, P, ls, variance, u=None, Wt=None, defect=None, chunk=None):
    """(out_u [n], gout_u [n, d], out_w [n], gout_w [n, d]) in np.longdouble (None for an absent weight).  Wt [n_pts, ldw >= n]: the columns from n on
    are not read - except by the defect "ld_wrong", which reads the flat array with the leading dimension n."""
    xnew = np.asarray(xnew, dtype=np.float64)
    n, f = len(xnew), LD(variance)
    if Wt is not None:
        Wt = np.asarray(Wt, dtype=LD)
        W = Wt.reshape(-1)[:len(P) * n].reshape(len(P), n) if defect == "ld_wrong" else Wt[:, :n]
    res = [None if u is None else np.zeros(n, dtype=LD), None if u is None else np.zeros((n, xnew.shape[1]), dtype=LD),
           None if Wt is None else np.zeros(n, dtype=LD), None if Wt is None else np.zeros((n, xnew.shape[1]), dtype=LD)]
    for a, b in _rows(n):
        kap, w = _pair_terms(kind, xnew[a:b], P, ls, defect, chunk)
        if u is not None:
            ul = np.asarray(u, dtype=LD).reshape(-1)
            res[0][a:b] = f * (kap @ ul)
            res[1][a:b] = -f * np.einsum("imk,m->ik", w, ul)
        if Wt is not None:
            res[2][a:b] = f * (kap * W[:, a:b].T).sum(axis=1)
            res[3][a:b] = -f * np.einsum("imk,mi->ik", w, W[:, a:b])
    if defect == "sign":
        res[1], res[3] = (None if res[1] is None else -res[1]), (None if res[3] is None else -res[3])
    if defect == "swap_uw" and u is not None and Wt is not None:
        res = [res[2], res[3], res[0], res[1]]
    return tuple(res)


def weighted_tolerance(kind, xnew, P, ls, variance, u=None, Wt=None):
    """Per-element tolerances (tv_u [n], tg_u [n, d], tv_w [n], tg_w [n, d]) of the product, None for an absent weight."""
    xnew = np.asarray(xnew, dtype=np.float64)
    n, d = xnew.shape
    out = [None] * 4
    ua = None if u is None else np.abs(np.asarray(u, dtype=np.float64).reshape(-1))
    Wa = None if Wt is None else np.abs(np.asarray(Wt, dtype=np.float64)[:, :n])
    if ua is not None:
        out[0], out[1] = np.zeros(n), np.zeros((n, d))
    if Wa is not None:
        out[2], out[3] = np.zeros(n), np.zeros((n, d))
    for a, b in _rows(n):
        kap, w = ig.cross_terms(kind, xnew[a:b], P, ls)
        kap, w = np.abs(kap).astype(np.float64), np.abs(w).astype(np.float64)
        if ua is not None:
            floor = ig.FLOOR * variance * ua.sum()
            out[0][a:b] = ig.TOL * variance * (kap @ ua) + floor
            out[1][a:b] = ig.TOL * variance * np.einsum("imk,m->ik", w, ua) + floor
        if Wa is not None:
            floor = ig.FLOOR * variance * Wa[:, a:b].sum(axis=0)
            out[2][a:b] = ig.TOL * variance * (kap * Wa[:, a:b].T).sum(axis=1) + floor
            out[3][a:b] = ig.TOL * variance * np.einsum("imk,mi->ik", w, Wa[:, a:b]) + floor[:, None]
    return tuple(out)


# ---- cells of the product test (tests/test_gpu_predict_grad.py) ----------------------------------------------------------------------------------
DIMS = (1, 3, 8, 9, 20, 32)
N_PTS = (1, 65, 300)
JSPLITS = (1, 3, 7)
#: rows per lane -> the D of DIMS that reach it
CLASSES = {4: (1, 3), 2: (8,), 1: (9, 20, 32)}


def row_counts(d: int):
    B = rows_per_block(d)
    return (1, B - 1, B, B + 1, 4097)


def product_cells():
    """dicts (D, n_new, n_pts, set, jsplit, kind, precision, ldw_extra): every D with its five row counts (30 cells); the point count, the set, the forced
    kff_jsplit, the kind, the precision level and the padding of Wt are dealt cyclically with strides that make every value meet every D."""
    cells, x = [], 0
    for a, d in enumerate(DIMS):
        for q, n in enumerate(row_counts(d)):
            cells.append(dict(D=d, n_new=n, n_pts=N_PTS[(x + a) % 3], set=("train", "inducing")[(x + q // 3) % 2], jsplit=JSPLITS[(x // 3 + a) % 3],
                              kind=ig.KINDS[(q + a) % 3], precision=(x // 2) % 2, ldw_extra=(0, 3, 8)[(x + 1) % 3] if n > 1 else 5))
            x += 1
    return cells


def cell_id(c) -> str:
    return "D%d_n%d_P%d_%s_j%d_%s_p%d_ld%d" % (c["D"], c["n_new"], c["n_pts"], c["set"], c["jsplit"], c["kind"], c["precision"], c["ldw_extra"])


def cell_problem(c):
    """(X, y, Z, xnew, u [n_pts], Wt [n_pts, ldw] with NaN in the columns from n_new on) of a cell.  The point set the cell multiplies against has
    n_pts rows (the other one 7); new point 0 sits on point min(3, n_pts - 1) of that set and new point 1 (if any) at 10^3."""
    import gpr_ref
    N, M = (c["n_pts"], 7) if c["set"] == "train" else (70, c["n_pts"])
    X, y = gpr_ref.problem(N, c["D"])
    rng = np.random.default_rng(1000 * c["D"] + 7 * c["n_new"] + c["n_pts"])
    Z = X[:M].copy() if M <= N else rng.standard_normal((M, c["D"]))
    P = X if c["set"] == "train" else Z
    xnew = ig.new_points(P, c["n_new"])
    u = rng.standard_normal(len(P))
    Wt = np.full((len(P), c["n_new"] + c["ldw_extra"]), np.nan)
    Wt[:, :c["n_new"]] = rng.standard_normal((len(P), c["n_new"]))
    return X, y, Z, xnew, u, Wt


# ---- the predictors ------------------------------------------------------------------------------------------------------------------------------
PREDICT_DEFECTS = ("sign", "gvar_factor", "q_without_LinvT", "kv_term_dropped", "ct_without_tmp2", "ld_wrong", "lost_rows", "drop_chunk_last",
                   "coincident_nonzero", "swap_uw", "inv_l", "m32_for_m52")
_PAIR = {"inv_l", "m32_for_m52", "coincident_nonzero", "drop_chunk_last", "lost_rows", "ld_wrong", "swap_uw"}


@dataclasses.dataclass
class Grad:
    mean: np.ndarray    # [n]
    g_mean: np.ndarray  # [n, d]
    var: np.ndarray
    g_var: np.ndarray


def _panel(Ct, n):
    """C^T [M, n] as the library stores it: [M][ld], ld = (n + 7) & ~7, zeros in the padding."""
    out = np.zeros((Ct.shape[0], (n + 7) & ~7))
    out[:, :n] = Ct
    return out


def cglb_predict_grad_analytic(kind, X, y, hyp, v, Xnew, quad_term, defect=None) -> Grad:
    """The library's algebra in float64 (the pair sums in np.longdouble).  `defect`: one of PREDICT_DEFECTS."""
    ls, f, s = hyp.lengthscales, hyp.variance, hyp.noise
    M, n = hyp.Z.shape[0], len(Xnew)
    v = np.zeros(len(X)) if quad_term else np.asarray(v, dtype=np.float64)
    L = np.linalg.cholesky(kernel(kind, hyp.Z, hyp.Z, ls, f) + hyp.jitter * np.eye(M))
    Kuf = kernel(kind, hyp.Z, X, ls, f)
    A = sla.solve_triangular(L, Kuf, lower=True) / math.sqrt(s)
    LB = np.linalg.cholesky(A @ A.T + np.eye(M))
    res = (y - hyp.mean) - (kernel(kind, X, X, ls, f) @ v + s * v)
    c = sla.solve_triangular(LB, A @ res, lower=True) / math.sqrt(s)
    Kus = kernel(kind, hyp.Z, Xnew, ls, f)
    tmp1 = sla.solve_triangular(L, Kus, lower=True)
    tmp2 = sla.solve_triangular(LB, tmp1, lower=True)
    q = sla.solve_triangular(LB, c, lower=True, trans="T")
    if defect != "q_without_LinvT":
        q = sla.solve_triangular(L, q, lower=True, trans="T")
    inner = tmp1 if defect == "ct_without_tmp2" else tmp1 - sla.solve_triangular(LB, tmp2, lower=True, trans="T")
    Ct = sla.solve_triangular(L, inner, lower=True, trans="T")
    pair = defect if defect in _PAIR else None
    chunk = weighted_split(min(n, ROWS), M, X.shape[1])[1]
    _, gq, _, gc = weighted_product(kind, Xnew, hyp.Z, ls, f, q, _panel(Ct, n), pair, chunk)
    mean = hyp.mean + (0 if quad_term else kernel(kind, Xnew, X, ls, f) @ v) + tmp2.T @ c
    var = f + (tmp2 ** 2).sum(0) - (tmp1 ** 2).sum(0)
    g_mean = gq.astype(np.float64)
    if not quad_term and defect != "kv_term_dropped":
        g_mean = g_mean + weighted_product(kind, Xnew, X, ls, f, v)[1].astype(np.float64)
    g_var = (-1.0 if defect == "gvar_factor" else -2.0) * gc.astype(np.float64)
    if defect == "sign":
        g_mean, g_var = -g_mean, -g_var
    return Grad(mean, g_mean, var, g_var)


def _autograd(fn, Xnew):
    x = torch.tensor(np.asarray(Xnew, dtype=np.float64), requires_grad=True)
    mean, var = fn(x)
    gm, = torch.autograd.grad(mean.sum(), x, retain_graph=True)   # the new points are independent: row i of the gradient is that of output i
    gv, = torch.autograd.grad(var.sum(), x)
    return Grad(mean.detach().numpy(), gm.numpy(), var.detach().numpy(), gv.numpy())


def cglb_predict_grad_autograd(kind, X, y, hyp, v, Xnew, quad_term) -> Grad:
    """torch.autograd in fp64 through the textbook form: Sigma = K_uu + jitter I + K_uf K_fu / s, mean = mu + K_*f v + K_*u Sigma^-1 K_uf res / s,
    var = f - K_*u (K_uu + jitter I)^-1 K_u* + K_*u Sigma^-1 K_u*, res = (y - mu) - (K_ff + s I) v."""
    ls, f, s = hyp.lengthscales, hyp.variance, hyp.noise
    M = hyp.Z.shape[0]
    v = np.zeros(len(X)) if quad_term else np.asarray(v, dtype=np.float64)
    Kuu = kernel(kind, hyp.Z, hyp.Z, ls, f) + hyp.jitter * np.eye(M)
    Kuf = kernel(kind, hyp.Z, X, ls, f)
    res = (y - hyp.mean) - (kernel(kind, X, X, ls, f) @ v + s * v)
    Ls, Lu = torch.tensor(np.linalg.cholesky(Kuu + Kuf @ Kuf.T / s)), torch.tensor(np.linalg.cholesky(Kuu))
    a = torch.tensor(sla.cho_solve((Ls.numpy(), True), Kuf @ res) / s)
    Xt, Zt, lt, vt = torch.tensor(np.asarray(X, dtype=np.float64)), torch.tensor(np.asarray(hyp.Z, dtype=np.float64)), torch.tensor(np.asarray(ls, dtype=np.float64)), torch.tensor(v)

    def fn(x):
        Ksu = _torch_kernel(kind, x, Zt, lt, f)
        mean = hyp.mean + Ksu @ a
        if not quad_term:
            mean = mean + _torch_kernel(kind, x, Xt, lt, f) @ vt
        var = f - (Ksu * torch.cholesky_solve(Ksu.T, Lu).T).sum(dim=1) + (Ksu * torch.cholesky_solve(Ksu.T, Ls).T).sum(dim=1)
        return mean, var
    return _autograd(fn, Xnew)


def gpr_predict_grad_analytic(kind, X, y, hyp, Xnew, defect=None) -> Grad:
    ls, f, s = hyp.lengthscales, hyp.variance, hyp.noise
    n = len(Xnew)
    Lk = np.linalg.cholesky(kernel(kind, X, X, ls, f) + s * np.eye(len(X)))
    alpha = sla.cho_solve((Lk, True), y - hyp.mean)
    Kfs = kernel(kind, X, Xnew, ls, f)
    V = sla.solve_triangular(Lk, Kfs, lower=True)
    C = sla.solve_triangular(Lk, V, lower=True, trans="T")
    pair = defect if defect in _PAIR else None
    chunk = weighted_split(min(n, ROWS), len(X), X.shape[1])[1]
    _, ga, _, gc = weighted_product(kind, Xnew, X, ls, f, alpha, _panel(C, n), pair, chunk)
    g_mean, g_var = ga.astype(np.float64), (-1.0 if defect == "gvar_factor" else -2.0) * gc.astype(np.float64)
    if defect == "sign":
        g_mean, g_var = -g_mean, -g_var
    return Grad(hyp.mean + Kfs.T @ alpha, g_mean, f - (V * V).sum(0), g_var)


def gpr_predict_grad_autograd(kind, X, y, hyp, Xnew) -> Grad:
    ls, f, s = hyp.lengthscales, hyp.variance, hyp.noise
    Lk = np.linalg.cholesky(kernel(kind, X, X, ls, f) + s * np.eye(len(X)))
    alpha = torch.tensor(sla.cho_solve((Lk, True), y - hyp.mean))
    Lt, Xt, lt = torch.tensor(Lk), torch.tensor(np.asarray(X, dtype=np.float64)), torch.tensor(np.asarray(ls, dtype=np.float64))

    def fn(x):
        Ksf = _torch_kernel(kind, x, Xt, lt, f)
        return hyp.mean + Ksf @ alpha, f - (Ksf * torch.cholesky_solve(Ksf.T, Lt).T).sum(dim=1)
    return _autograd(fn, Xnew)


def predictor_tolerance(kind, hyp, ref: Grad):
    """{"mean", "var": scalars; "g_mean", "g_var": [d]} absolute tolerances of a predictor's outputs at the reference `ref`."""
    ls = np.asarray(hyp.lengthscales, dtype=np.float64).reshape(-1)
    C = ig.C_KIND[kind]
    return {"mean": TOL_PREDICT * np.abs(ref.mean).max(), "var": TOL_PREDICT * np.abs(ref.var).max(),
            "g_mean": TOL_PREDICT * np.maximum(np.abs(ref.g_mean).max(), math.sqrt(C * hyp.variance) / ls),
            "g_var": TOL_PREDICT * np.maximum(np.abs(ref.g_var).max(), hyp.variance * math.sqrt(C) / ls)}


def grad_miss(out: Grad, ref: Grad, tol) -> float:
    """max over the two gradient arrays of |out - ref| / tolerance; inf for an entry that is not finite."""
    if not (np.all(np.isfinite(out.g_mean)) and np.all(np.isfinite(out.g_var))):
        return math.inf
    return max(float((np.abs(out.g_mean - ref.g_mean) / tol["g_mean"]).max()), float((np.abs(out.g_var - ref.g_var) / tol["g_var"]).max()))


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------
#: cglb_predict_grad: the fp64 cells of group B of predict_ref.CASES, one Matern-5/2 cell, one cell with more new points than a launch takes
M52_CASE = pr.Case("B", "fp64", 3, 130, 33, 9, "matern52", True, 1)
LARGE_CASE = pr.Case("B", "fp64", 8, 130, 33, 4097, "matern32", True, 0)
CGLB_CASES = tuple(c for c in pr.cases("B") if c.dtype == "fp64") + (M52_CASE,)
#: cglb_gpr_predict_grad: group D up to n_new = 4097
GPR_CASES = tuple(c for c in pr.cases("D") if c.n_new <= 4097)


@functools.lru_cache(maxsize=None)
def cglb_reference(case, quad_term) -> Grad:
    X, y, hyp, v = pr.problem(case)
    return cglb_predict_grad_autograd(case.kind, X, y, hyp, v, pr.xnew(case), quad_term)


@functools.lru_cache(maxsize=None)
def gpr_reference(case) -> Grad:
    X, y, hyp, _ = pr.problem(case)
    return gpr_predict_grad_autograd(case.kind, X, y, hyp, pr.xnew(case))


def defect_applies(case, defect: str, quad_term: int, n_pts: int, P) -> bool:
    """Whether a planted defect changes the outputs of a cell at all (the reasons are structural):
    * kv_term_dropped: only where the term exists (quad_term 0);
    * q_without_LinvT / ct_without_tmp2: always (L is never the identity: jitter and f);
    * ld_wrong: n_new % 8 != 0, more than one point, more than one new point (row 0 of the panel is read alike);
    * drop_chunk_last, lost_rows: always (with one point everything is lost);
    * coincident_nonzero: a new point sits on a point of the set and its weight is not zero;
    * m32_for_m52: the Matern-5/2 cell;
    * the far point alone would hide everything, but n_new = 1 keeps a training row (predict_ref.xnew)."""
    n = case.n_new
    if defect == "kv_term_dropped":
        return quad_term == 0
    if defect == "ld_wrong":
        return n % 8 != 0 and n_pts > 1 and n > 1
    if defect == "coincident_nonzero":
        xn = pr.xnew(case)
        return bool((np.abs(xn[:, None, :] - np.asarray(P)[None, :, :]).max(axis=2) == 0).any())
    if defect == "m32_for_m52":
        return case.kind == "matern52"
    return True
