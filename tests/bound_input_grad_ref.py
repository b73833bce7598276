"""Restatement of the gradient of the CGLB / SGPR bounds with respect to the TRAINING inputs (test helper, not a test module; runs on any CPU).

    gx[n, k] = sum_m (Guf[m, n] + c_m w_n) d k(z_m, x_n) / d x_nk                    K_uf part (cglb_grad_x_kuf)
             + sum_j (u_n v_j + v_n u_j) d k(x_n, x_j) / d x_nk,  u = w + v / 2       K_ff part (cglb_grad_x_kff_pair), CG quadratic term only
    d k(z, x) / d x_k = +h delta_k / l_k,   delta_k = (z_k - x_k) / l_k,   h: the radial factor with the variance (train_input_grad_ref.grad_factor)

* `bound_and_grad_x`: the reference of the evaluation - torch autograd of bound_variants_ref.bound (v detached) in X, Matern-5/2 supplied by
  matern52_ref.
* `adjoints`: Guf, c, w, u of one evaluation in float64 numpy, as csrc/cglb_api.hip (obj_phase3_impl) forms them.
* `kuf_grad_x`, `kff_pair_grad_x`: the two products in np.longdouble with their per-element sums of absolute terms; `defect` plants one of DEFECTS.
* the mirrors of the launcher's rules (csrc/row_slab.h: grad_x_kuf_rows_per_lane, row_slab_panel_split, train_input_grad_pair_rows_per_lane;
  csrc/kernels_train_input_grad.hip: the rows of a launch of the single-pair pass) and the covering tables of tests/test_gpu_bound_input_grad.py.
"""
from __future__ import annotations

import numpy as np

import matern52_ref as m5
import slab_rules
import train_input_grad_ref as tr

LD = np.longdouble
KINDS = tr.KINDS
OPTIONS = {"cglb": (0, 0), "cglbnm2": (1, 0), "sgpr": (1, 1)}   # class -> (logdet_bound, quad_term)
CLASSES = tuple(OPTIONS)
TOL = 1e-11   # of the per-element sum of absolute terms: the figure every value-and-gradient product is held to
DEFECTS = ("no_rank_one", "no_transposed_term", "drop_chunk_last", "sign", "G_transposed")


# ---- the reference of the evaluation ---------------------------------------------------------------------------------------------------------
def bound_and_grad_x(cls, kind, X, y, h, Z, v=None, jitter=1e-6, device="cpu", x_map=None):
    """(bound, d bound / d X [N, D], hyper-parameter gradient dict) by torch autograd of the dense fp64 restatement, v held constant.
    x_map: (raw, A) - the inputs are raw @ A and the gradient returned in place of d / d X is d / d A."""
    import torch
    f64 = dict(dtype=torch.float64, device=device)
    params = [torch.tensor(np.asarray(h["lengthscales"], dtype=np.float64).reshape(-1), **f64), torch.tensor(float(h["variance"]), **f64),
              torch.tensor(float(h["noise"]), **f64), torch.tensor(float(h["mean"]), **f64), torch.tensor(np.asarray(Z, dtype=np.float64), **f64)]
    for p in params:
        p.requires_grad_(True)
    if x_map is None:
        leaf = torch.tensor(np.asarray(X, dtype=np.float64), **f64).requires_grad_(True)
        x = leaf
    else:
        leaf = torch.tensor(np.asarray(x_map[1], dtype=np.float64), **f64).requires_grad_(True)
        x = torch.tensor(np.asarray(x_map[0], dtype=np.float64), **f64) @ leaf
    vt = None if v is None else torch.as_tensor(np.asarray(v, dtype=np.float64), **f64).reshape(-1)
    with m5.bound_variants_with_matern52() as bref:
        b = bref.bound(cls, kind, x, torch.as_tensor(np.asarray(y, dtype=np.float64), **f64).reshape(-1), *params, jitter=jitter, v=vt)
        g = torch.autograd.grad(b, [leaf] + params)
    keys = ("lengthscales", "variance", "noise", "mean", "Z")
    return float(b.detach()), g[0].detach().cpu().numpy(), {k: gi.detach().cpu().numpy() for k, gi in zip(keys, g[1:])}


# ---- the adjoints of one evaluation (csrc/cglb_api.hip: obj_phase2, obj_phase3_impl), float64 -------------------------------------------------
def kernel(kind, X1, X2, ls, variance):
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (X1.shape[1],))
    a, b = X1 / ls, X2 / ls
    d2 = sum((a[:, k, None] - b[None, :, k]) ** 2 for k in range(X1.shape[1]))
    if kind == "rbf":
        return variance * np.exp(-0.5 * d2)
    return m5.k32(d2, variance) if kind == "matern32" else m5.k52(d2, variance)


def adjoints(cls, kind, X, y, h, Z, v=None, jitter=1e-6):
    """dict Guf [M, N], c [M], w [N], u [N] or None, v [N] or None: bound adjoint of K_uf = Guf + c w^T, of K_ff = u v^T (both orientations)"""
    import scipy.linalg as sl
    ld, qt = OPTIONS[cls]
    N, M = X.shape[0], Z.shape[0]
    f, s, sigma = float(h["variance"]), float(h["noise"]), float(np.sqrt(h["noise"]))
    Kuf = kernel(kind, Z, X, h["lengthscales"], f)
    L = np.linalg.cholesky(kernel(kind, Z, Z, h["lengthscales"], f) + jitter * np.eye(M))
    A = sl.solve_triangular(L, Kuf, lower=True) / sigma
    AAt = A @ A.T
    B = np.eye(M) + AAt
    Binv = np.linalg.inv(B)
    tau = 1.0 if ld == 1 else 1.0 + (N * f / s - np.trace(AAt)) / N
    e = np.asarray(y, dtype=np.float64).reshape(-1) - float(h["mean"])
    if qt == 1:
        r, vv = e, None
    else:
        vv = np.zeros(N) if v is None else np.asarray(v, dtype=np.float64).reshape(-1)
        r = e - (kernel(kind, X, X, h["lengthscales"], f) @ vv + s * vv)
    w = (r - A.T @ (Binv @ (A @ r))) / s                                   # w = P r
    c = sigma * sl.solve_triangular(L, A @ w, lower=True, trans="T")       # K_uu^-1 K_uf w
    Guf = sl.solve_triangular(L, (np.eye(M) / tau - Binv) @ A, lower=True, trans="T") / sigma
    return dict(Guf=Guf, c=c, w=w, u=None if qt == 1 else w + 0.5 * vv, v=vv)


# ---- the two products, np.longdouble -----------------------------------------------------------------------------------------------------------
def kuf_grad_x(kind, X, Z, ls, variance, G, cvec=None, wvec=None, defect=None, chunk=None):
    """(gx [N, D], scale [N, D]): gx[n, k] = sum_m (G[m, n] + c_m w_n) h_mn delta_mnk / l_k, scale the same sum of absolute values.  G: [M, >= N]
    (the columns from N on are ignored).  defect: no_rank_one | drop_chunk_last (`chunk`: the launcher's chunk length over m) | sign |
    G_transposed (M == N)."""
    X = np.asarray(X, dtype=LD).reshape(len(X), -1)
    Z = np.asarray(Z, dtype=LD).reshape(len(Z), -1)
    N, D, M = X.shape[0], X.shape[1], Z.shape[0]
    lsd = np.broadcast_to(np.asarray(ls, dtype=LD).reshape(-1), (D,))
    g = np.asarray(G, dtype=LD)[:, :N]
    if defect == "G_transposed":
        g = g.T.copy()
    if cvec is not None and defect != "no_rank_one":
        g = g + np.outer(np.asarray(cvec, dtype=LD), np.asarray(wvec, dtype=LD))
    delta = [(Z[:, k][:, None] - X[None, :, k]) / lsd[k] for k in range(D)]   # [M, N]
    hfac = tr.grad_factor(kind, sum(dk * dk for dk in delta), variance)
    if defect == "drop_chunk_last":
        last = ((M - 1) // chunk) * chunk
        g = g.copy()
        g[last:] = 0
    gx, scale = np.zeros((N, D), dtype=LD), np.zeros((N, D), dtype=LD)
    for k, dk in enumerate(delta):
        T = hfac * dk / lsd[k]
        if defect == "sign":
            T = -T
        gx[:, k] = (g * T).sum(axis=0)
        scale[:, k] = (np.abs(g) * np.abs(T)).sum(axis=0)
    return gx, scale


def kff_pair_grad_x(kind, X, ls, variance, u, v, defect=None):
    """(gx, scale) of the single pair (u, v): train_input_grad_ref.grad_x at S = 1"""
    return tr.grad_x(kind, X, ls, variance, np.asarray(u).reshape(-1, 1), np.asarray(v).reshape(-1, 1), defect=defect)


def kff_pair_grad_x_rows(kind, X, ls, variance, u, v, rows):
    """(gx, scale, sum_j |w_ij|) of the single pair for the given rows only, each [len(rows), ...]: the reference of a cell whose N makes the full
    square too slow for a test (one row past a launch block)"""
    X = np.asarray(X, dtype=LD).reshape(len(X), -1)
    u, v = np.asarray(u, dtype=LD).reshape(-1), np.asarray(v, dtype=LD).reshape(-1)
    lsd = np.broadcast_to(np.asarray(ls, dtype=LD).reshape(-1), (X.shape[1],))
    delta = [(X[rows, k][:, None] - X[None, :, k]) / lsd[k] for k in range(X.shape[1])]
    hfac = tr.grad_factor(kind, sum(dk * dk for dk in delta), variance)
    w = np.outer(u[rows], v) + np.outer(v[rows], u)
    gx, scale = np.zeros((len(rows), X.shape[1]), dtype=LD), np.zeros((len(rows), X.shape[1]), dtype=LD)
    for k, dk in enumerate(delta):
        T = -hfac * dk / lsd[k]
        gx[:, k] = (w * T).sum(axis=1)
        scale[:, k] = (np.abs(w) * np.abs(T)).sum(axis=1)
    return gx, scale, np.abs(w).sum(axis=1)


def bound_grad_x(cls, kind, X, y, h, Z, v=None, jitter=1e-6, defect=None, chunk=None):
    """(gx, scale) of the evaluation: the K_uf product of the adjoints plus, for the CG classes, the K_ff pair product"""
    a = adjoints(cls, kind, X, y, h, Z, v, jitter)
    kuf_defect = defect if defect in ("no_rank_one", "drop_chunk_last", "sign", "G_transposed") else None
    gx, scale = kuf_grad_x(kind, X, Z, h["lengthscales"], h["variance"], a["Guf"], a["c"], a["w"], defect=kuf_defect, chunk=chunk)
    if a["u"] is not None:
        g2, s2 = kff_pair_grad_x(kind, X, h["lengthscales"], h["variance"], a["u"], a["v"],
                                 defect=defect if defect in ("no_transposed_term", "sign") else None)
        gx, scale = gx + g2, scale + s2
    return gx, scale


# ---- launch geometry (csrc/row_slab.h, csrc/kernels_train_input_grad.hip) ---------------------------------------------------------------------
KUF_TARGET_WG, KUF_MIN_CHUNK = 2048, 16   # GRAD_X_KUF_TARGET_WG, GRAD_X_KUF_MIN_CHUNK


def kuf_rows_per_lane(d: int) -> int:
    return 2 if tr.pad_dim(d) <= 8 else 1


def panel_split(forced: int, row_blocks: int, M: int, slot_cap: int):
    """row_slab_panel_split: (chunks, chunk length) over the inducing points"""
    min_chunk = 1 if forced > 0 else KUF_MIN_CHUNK
    ms = forced if forced > 0 else -(-KUF_TARGET_WG // row_blocks)
    ms = max(1, min(ms, slot_cap, -(-M // min_chunk)))
    chunk = -(-M // ms)
    return -(-M // chunk), chunk


def kuf_split(N: int, M: int, d: int, forced: int = 0):
    bx = -(-N // (256 * kuf_rows_per_lane(d)))
    return panel_split(forced, bx, M, slab_rules.slot_cap(N, tr.pad_dim(d)))


def pair_rows_per_lane(d: int) -> int:
    dp = tr.pad_dim(d)
    return 4 if dp <= 8 else (2 if dp <= 16 else 1)


def pair_launch_rows(d: int) -> int:
    return tr.ROWS * (2 if pair_rows_per_lane(d) > 2 else 1)


#: one input dimension of every rows-per-lane class
KUF_CLASSES = {2: 8, 1: 12}
PAIR_CLASSES = {4: 8, 2: 12, 1: 20}


def kuf_cells():
    """dicts (N, M, D, msplit, ldg_pad, rank_one, kind, trained) of the every-element test of the panel pass: every R class at one row past its row
    block; N one past 4096; M in 1, 16, 130; forced splits 0, 1, 3, 7; ldg > N; cvec / wvec NULL; the three kinds at both hyper-parameter sets."""
    cells, i = [], 0
    for R, D in KUF_CLASSES.items():
        for M, ms in ((1, 1), (16, 3), (130, 7), (130, 0)):
            cells.append(dict(N=256 * R + 1, M=M, D=D, msplit=ms, pad=(0, 5, 32, 1)[i % 4], rank_one=i % 3 != 2, kind=KINDS[i % 3], trained=bool(i % 2)))
            i += 1
    for N, M, D, ms in ((1, 1, 1, 0), (2, 16, 3, 3), (63, 130, 3, 7), (4097, 16, 1, 3), (4097, 130, 20, 7), (300, 130, 32, 1), (1100, 16, 6, 0)):
        cells.append(dict(N=N, M=M, D=D, msplit=ms, pad=(0, 5, 32, 1)[i % 4], rank_one=i % 3 != 2, kind=KINDS[i % 3], trained=bool(i % 2)))
        i += 1
    return cells


def pair_cells():
    """(N, D, forced jsplit, kind, trained): every rows-per-lane class of the single-pair pass at one row past its row block with forced splits 1, 3,
    7 and the rule; one row past a launch block"""
    cells, i = [], 0
    for R, D in PAIR_CLASSES.items():
        for js in (1, 3, 7, 0):
            cells.append((256 * R + 1, D, js, KINDS[i % 3], bool(i % 2)))
            i += 1
    # one row past a launch block at one input dimension (the np.longdouble reference costs N^2 D); N = 1
    cells += [(pair_launch_rows(1) + 1, 1, 0, "matern32", True), (1, 1, 0, "matern52", True)]
    return cells
