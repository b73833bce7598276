"""Dense np.longdouble restatement of the gradients with respect to the TRAINING inputs (test helper, not a test module; runs on any CPU).

    d k(x_i, x_j) / d x_ik = -h_ij delta_ijk / l_k,   delta_ijk = (x_ik - x_jk) / l_k,   h: oracle.kernel_grad_factor (variance included)
    gx[i, k] = sum_j w_ij d k(x_i, x_j) / d x_ik
        pairs:  w_ij = sum_b (u_bi v_bj + v_bi u_bj)          (cglb_grad_x_kff_multi, the input gradient of cglb_itergp_objective_and_grad_x)
        dense:  w_ij = alpha_i alpha_j - K^-1_ij              (cglb_gpr_objective_and_grad_x)
    scale[i, k] = sum_j |w_ij| h_ij |delta_ijk| / l_k          the per-element sum of absolute terms every tolerance is a fraction of

Two identities hold to round-off for any U, V, with G_l[k] = sum_b u_b^T (dK / dl_k) v_b (cglb_grad_kff_multi):
    scaling       sum_i x_ik gx[i, k] = -l_k G_l[k]
    translation   sum_i gx[i, k] = 0

Built on oracle/cglb_oracle.py (`kernel_grad_factor`) and matern52_ref (`h52`), imported and not modified.  Also here: the mirrors of the launcher's
rules (csrc/row_slab.h: train_input_grad_rows_per_lane, train_input_grad_group_width; csrc/kernels_train_input_grad.hip), the covering table of
tests/test_gpu_train_input_grad.py, the planted defects of tests/test_train_input_grad_ref_host.py, and a torch (CPU, fp64) dense log marginal
likelihood that autograd differentiates in the inputs.
"""
from __future__ import annotations

import math

import numpy as np

import matern52_ref as m5
import slab_rules
from oracle import cglb_oracle as orc

LD = np.longdouble
EPS = 2.0 ** -53
KINDS = ("rbf", "matern32", "matern52")
#: the tolerance the pair evaluator is held to (tests/test_gpu_input_grad.py, tests/test_gpu_grad_multi.py) and the floor of the range-clamped 2^x
#: (input_grad_ref.FLOOR: 2^-1000 times a bound of the gradient's factor), per unit of f sum_j |w_ij|
TOL, FLOOR = 1e-11, 2.0 ** -1000 * 1e8
DEFECTS = ("no_transposed_term", "drop_chunk_last", "drop_groups_after_first", "sign")


def pad_dim(d: int) -> int:
    """the padded width the context runs an input dimension at (csrc/dispatch.h: CGLB_DISPATCH_DP)"""
    for dp in (1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32):
        if d <= dp:
            return dp
    raise ValueError(d)


def grad_factor(kind, d2, variance):
    """h_ij (np.longdouble) at the scaled squared distances d2"""
    d2 = np.asarray(d2, dtype=LD)
    if kind == "matern52":
        return m5.h52(d2, LD(variance))
    return orc.kernel_grad_factor(kind, d2, LD(variance))


def _blocks(kind, X, ls, variance, rows=512):
    """(row slice, h [rows, N], delta [d][rows, N]) block by block of rows, np.longdouble: delta_k = (x_ik - x_jk) / l_k; memory stays O(rows N)"""
    X = np.asarray(X, dtype=LD).reshape(len(X), -1)
    lsd = np.broadcast_to(np.asarray(ls, dtype=LD).reshape(-1), (X.shape[1],))
    for i0 in range(0, len(X), rows):
        sl = slice(i0, min(i0 + rows, len(X)))
        delta = [(X[sl, k][:, None] - X[None, :, k]) / lsd[k] for k in range(X.shape[1])]
        yield sl, grad_factor(kind, sum(dk * dk for dk in delta), variance), delta, lsd


def pair_weights(U, V, defect=None, group=8, rows=slice(None)):
    """w [rows, N] = sum_b (u_bi v_bj + v_bi u_bj) for U, V [N, S], np.longdouble"""
    U = np.asarray(U, dtype=LD).reshape(len(U), -1)
    V = np.asarray(V, dtype=LD).reshape(len(V), -1)
    if defect == "drop_groups_after_first":
        U, V = U[:, :group], V[:, :group]
    w = U[rows] @ V.T
    return w if defect == "no_transposed_term" else w + V[rows] @ U.T


def grad_x(kind, X, ls, variance, U=None, V=None, w=None, defect=None, chunk=None, group=8):
    """(gx [N, d], scale [N, d]) in np.longdouble from the vector pairs U, V [N, S] or from a dense weight w [N, N]: gx[i, k] = sum_j w_ij T_ijk with
    T_ijk = -h_ij delta_ijk / l_k = d k(x_i, x_j) / d x_ik, scale the same sum of absolute values.  `defect`: one of DEFECTS (`chunk`, `group`: the
    launcher's chunk length and group width)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    gx, scale = np.zeros(X.shape, dtype=LD), np.zeros(X.shape, dtype=LD)
    for sl, h, delta, lsd in _blocks(kind, X, ls, variance):
        wb = pair_weights(U, V, defect, group, sl) if w is None else np.asarray(w[sl], dtype=LD)
        for k, dk in enumerate(delta):
            T = -h * dk / lsd[k]
            if defect == "sign":   # delta taken as x_j - x_i
                T = -T
            if defect == "drop_chunk_last":
                T[:, min(chunk, len(X)) - 1] = 0
            gx[sl, k] = (wb * T).sum(axis=1)
            scale[sl, k] = (np.abs(wb) * np.abs(T)).sum(axis=1)
    return gx, scale


def tolerance(scale, w_abs_rowsum, variance):
    """per-element tolerance of the pair pass: TOL of the sum of absolute terms plus the floor where that sum underflows"""
    return TOL * np.asarray(scale, dtype=np.float64) + FLOOR * variance * np.asarray(w_abs_rowsum, dtype=np.float64)[:, None]


def lengthscale_forms(kind, X, ls, variance, U, V):
    """(G_l [d], sums of absolute terms [d]): G_l[k] = sum_b u_b^T (dK / dl_k) v_b = sum_ij (U V^T)_ij h_ij delta_ijk^2 / l_k, np.longdouble"""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    U = np.asarray(U, dtype=LD).reshape(len(X), -1)
    V = np.asarray(V, dtype=LD).reshape(len(X), -1)
    G, Gabs = np.zeros(X.shape[1], dtype=LD), np.zeros(X.shape[1], dtype=LD)
    for sl, h, delta, lsd in _blocks(kind, X, ls, variance):
        uv = U[sl] @ V.T
        for k, dk in enumerate(delta):
            t = h * dk * dk / lsd[k]
            G[k] += (uv * t).sum()
            Gabs[k] += (np.abs(uv) * np.abs(t)).sum()
    return G, Gabs


def gpr_weight(kind, X, y, hypers):
    """(w [N, N], alpha [N]) of the exact class: w = alpha alpha^T - K^-1 from the float64 Cholesky factor of gpr_ref.evaluate"""
    import scipy.linalg

    import gpr_ref
    with m5.oracle_with_matern52():
        ref = gpr_ref.evaluate(kind, X, y, hypers["lengthscales"], hypers["variance"], hypers["noise"], hypers["mean"], with_grad=False)
    Kinv = scipy.linalg.cho_solve((ref.L, True), np.eye(len(ref.alpha)))
    return np.outer(ref.alpha, ref.alpha) - 0.5 * (Kinv + Kinv.T), ref.alpha


# ---- launch geometry (csrc/row_slab.h, csrc/kernels_train_input_grad.hip) ------------------------------------------------------------------------
ROWS = 4096   # rows per launch


def rows_per_lane(d: int) -> int:
    return 2 if pad_dim(d) <= 8 else 1


def group_width(d: int) -> int:
    return 8 if pad_dim(d) <= 16 else 4


def rows_per_block(d: int) -> int:
    return 256 * rows_per_lane(d)


def split(N: int, d: int, forced: int = 0, row0: int = 0):
    """(jsplit, jchunk) of the launch for the rows [row0, min(row0 + ROWS, N)): the kff_jsplit rule over the N training points, capped by the slab
    of pad_dim(d) doubles per row, chunks of even length"""
    nrows = min(ROWS, N - row0)
    bx = -(-nrows // rows_per_block(d))
    return slab_rules.pair_split(forced, bx, N, slab_rules.slot_cap(nrows, pad_dim(d)), True)


#: the (R, G) classes the rule yields and one input dimension of each
CLASSES = {(2, 8): 8, (1, 8): 12, (1, 4): 20}


def covering_table():
    """Cells (N, D, S, forced jsplit, kind, trained) of the every-element test: every (R, G) class at one row past its row block, at S in
    {1, G, G + 1, 9, 11} and with one forced split each; N in 1, 2, 63, 1100 and one row past a launch block; D in 1, 3, 8, 12, 20, 32; the
    three kinds at both hyper-parameter sets."""
    cells = []
    for (R, G), D in CLASSES.items():
        for i, S in enumerate(sorted({1, G, G + 1, 9, 11})):
            cells.append((256 * R + 1, D, S, (0, 1, 3, 7, 0)[i], KINDS[i % 3], bool(i % 2)))
    cells += [(1, 1, 1, 0, "rbf", False), (2, 3, 2, 0, "matern32", True), (63, 3, 9, 3, "matern52", False), (63, 1, 11, 7, "rbf", True),
              (1100, 8, 11, 7, "matern32", False), (1100, 20, 9, 3, "matern52", True), (1100, 32, 5, 1, "rbf", True), (300, 32, 4, 0, "matern52", False),
              (300, 12, 9, 1, "matern32", True), (ROWS + 1, 1, 1, 0, "matern32", True)]
    return cells


# ---- torch (CPU, fp64): the dense log marginal likelihood, differentiable by autograd in x and the hyper-parameters -----------------------------
def torch_kernel(kind, x, ls, variance):
    import torch
    z = x / ls
    diff = z[:, None, :] - z[None, :, :]
    d2 = (diff * diff).sum(dim=2)
    if kind == "rbf":
        return variance * torch.exp(-0.5 * d2)
    # the root has no derivative at 0: the diagonal (and any coincident pair) is kept away from it; kappa is flat to first order there
    r = torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))) * (d2 > 0)
    if kind == "matern32":
        s = math.sqrt(3.0) * r
        return variance * (1.0 + s) * torch.exp(-s)
    if kind == "matern52":
        s = math.sqrt(5.0) * r
        return variance * (1.0 + s + s * s / 3.0) * torch.exp(-s)
    raise ValueError(kind)


def torch_lml(kind, x, y, ls, variance, noise, mean):
    """lml = -1/2 e^T K^-1 e - sum log L_ii - N/2 log 2 pi of K = f kappa(x, x) + s I (torch tensors, fp64, CPU)"""
    import torch
    K = torch_kernel(kind, x, ls, variance) + noise * torch.eye(x.shape[0], dtype=x.dtype)
    L = torch.linalg.cholesky(K)
    e = (y - mean).reshape(-1, 1)
    a = torch.cholesky_solve(e, L)
    return -0.5 * (e * a).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * x.shape[0] * math.log(2.0 * math.pi)
