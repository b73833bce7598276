"""Dense fp64 torch restatement of the five bounds of SGPR_CONFIGS (test helper, not a test module).

Each class is a log-det term and a quadratic term (reference paths relative to the reference repo root):

    cglb     Jensen log-det (cglb/backend/pytorch/models.py:215-244)               CG quadratic term at v (models.py:246-286)
    cglbnm2  NM^2 log-det   (cglb/backend/tensorflow/models.py:271-308)            CG quadratic term at v
    cglbn2m  N^2M log-det   (cglb/backend/tensorflow/models.py:311-350)            CG quadratic term at v
    sgpr     NM^2 log-det   (the SGPR bound, tensorflow/models.py:353-413 / gpflow)  exact term (tensorflow/models.py:393-402)
    sgprn2m  N^2M log-det   (tensorflow/models.py:353-413)                          exact term

The kernels and common terms are those of oracle/cglb_oracle.py (`kernel_matrix`, `common_terms`), written in torch so that
`torch.autograd.grad` gives the gradient with v detached, as cglb/backend/pytorch/optimizer.py:95-98 does.
"""
from __future__ import annotations

import math

import torch

from oracle import cglb_oracle as orc

CLASSES = {  # class -> (log-det term, quadratic term)
    "cglb": ("jensen", "cg"),
    "cglbnm2": ("nm2", "cg"),
    "cglbn2m": ("n2m", "cg"),
    "sgpr": ("nm2", "exact"),
    "sgprn2m": ("n2m", "exact"),
}

SQRT3 = math.sqrt(3.0)


def kernel_matrix(kind, X1, X2, ls, var):
    """oracle.cglb_oracle.kernel_matrix in torch: squared scaled differences summed one dimension at a time (never the matrix-product
    shortcut), then the closed form (RBF / Matern-3/2)."""
    a, b = X1 / ls, X2 / ls
    d2 = torch.zeros((X1.shape[0], X2.shape[0]), dtype=X1.dtype, device=X1.device)
    for d in range(X1.shape[1]):
        d2 = d2 + (a[:, d, None] - b[None, :, d]) ** 2
    if orc.kind_id(kind) == orc.RBF:
        return var * torch.exp(-0.5 * d2)
    r = torch.sqrt(d2.clamp_min(1e-300))  # flat at r = 0 (dk/dr = 0 there): the clamp keeps d r / d x finite and zero
    return var * (1.0 + SQRT3 * r) * torch.exp(-SQRT3 * r)


def common_terms(kind, X, ls, var, noise, Z, jitter):
    """oracle.cglb_oracle.common_terms (models.py:176-213): A = L^-1 K_uf / sigma, B = I + A A^T = LB LB^T."""
    M = Z.shape[0]
    kuf = kernel_matrix(kind, Z, X, ls, var)
    kuu = kernel_matrix(kind, Z, Z, ls, var) + jitter * torch.eye(M, dtype=X.dtype, device=X.device)
    L = torch.linalg.cholesky(kuu)
    A = torch.linalg.solve_triangular(L, kuf, upper=False) / torch.sqrt(noise)
    AAt = A @ A.T
    LB = torch.linalg.cholesky(AAt + torch.eye(M, dtype=X.dtype, device=X.device))
    return A, AAt, LB


def logdet_term(which, kind, X, ls, var, noise, A, AAt, LB):
    """Upper bound on -1/2 log|K_ff + s I| (returned with the sign the bound uses)."""
    N = X.shape[0]
    sum_log = torch.log(torch.diagonal(LB)).sum()
    t = N * var / noise - torch.trace(AAt)                                          # tr(K_ff - Q_ff) / s
    if which == "jensen":                                                           # models.py:236-243
        return -sum_log - 0.5 * N * torch.log(noise) - 0.5 * N * torch.log(1.0 + t / N)
    if which == "nm2":                                                              # tensorflow/models.py:295-308
        return -sum_log - 0.5 * N * torch.log(noise) - 0.5 * t
    if which == "n2m":                                                              # tensorflow/models.py:332-350
        Kt = kernel_matrix(kind, X, X, ls, var) + noise * torch.eye(N, dtype=X.dtype, device=X.device)
        C = torch.linalg.solve_triangular(LB, A, upper=False)
        tau = torch.trace(Kt) - torch.trace(C @ Kt @ C.T)
        # -(sum log + N/2 log s + N/2 (log tau - log N - log s)): the N/2 log s terms cancel
        return -sum_log - 0.5 * N * torch.log(tau / N)
    raise ValueError(which)


def quad_term(which, kind, X, y, ls, var, noise, mean, A, LB, v=None):
    """Upper bound on 1/2 e^T (K_ff + s I)^-1 e: the CG form at a detached v (models.py:246-286) or the exact SGPR term at v = 0."""
    e = y - mean
    if which == "exact":                                                            # tensorflow/models.py:393-402
        c = torch.linalg.solve_triangular(LB, (A @ e).reshape(-1, 1), upper=False).reshape(-1) / torch.sqrt(noise)
        return 0.5 * (e * e).sum() / noise - 0.5 * (c * c).sum()
    N = X.shape[0]
    v = torch.zeros_like(e) if v is None else v.detach().to(e)
    cov = kernel_matrix(kind, X, X, ls, var) + noise * torch.eye(N, dtype=X.dtype, device=X.device)
    cov_v = cov @ v                                                                 # :280
    r = e - cov_v                                                                   # :281
    t = torch.cholesky_solve((A @ r).reshape(-1, 1), LB).reshape(-1)                # conjugate_gradient.py:105-107
    w = (r - A.T @ t) / noise                                                       # :110-113
    lower = (v * (r + 0.5 * cov_v)).sum()                                           # :283
    return lower + 0.5 * (w * r).sum()                                              # :284


def bound(cls, kind, X, y, ls, var, noise, mean, Z, jitter=1e-6, v=None):
    """bound = -upper + logdet - N/2 log 2 pi for model class `cls` (all arguments torch tensors except kind, cls, jitter)."""
    ld, qt = CLASSES[cls]
    A, AAt, LB = common_terms(kind, X, ls, var, noise, Z, jitter)
    N = X.shape[0]
    return -quad_term(qt, kind, X, y, ls, var, noise, mean, A, LB, v) + logdet_term(ld, kind, X, ls, var, noise, A, AAt, LB) \
        - 0.5 * N * math.log(2.0 * math.pi)


def bound_and_grad(cls, kind, X, y, lengthscales, variance, noise, mean, Z, jitter=1e-6, v=None, device="cpu"):
    """(bound, gradient dict with the keys of HipContext.unpack_grad) from numpy / float inputs; v is held constant."""
    f64 = dict(dtype=torch.float64, device=device)
    X, y = torch.as_tensor(X, **f64), torch.as_tensor(y, **f64).reshape(-1)
    params = [torch.tensor(lengthscales, **f64).reshape(-1), torch.tensor(float(variance), **f64), torch.tensor(float(noise), **f64),
              torch.tensor(float(mean), **f64), torch.tensor(Z, **f64)]
    for p in params:
        p.requires_grad_(True)
    vt = None if v is None else torch.as_tensor(v, **f64).reshape(-1)
    b = bound(cls, kind, X, y, *params, jitter=jitter, v=vt)
    g = torch.autograd.grad(b, params)
    keys = ("lengthscales", "variance", "noise", "mean", "Z")
    return float(b.detach()), {k: gi.detach().cpu().numpy() for k, gi in zip(keys, g)}


def exact_half_logdet(kind, X, ls, var, noise):
    """1/2 log|K_ff + s I| by a dense Cholesky factorisation."""
    N = X.shape[0]
    Kt = kernel_matrix(kind, X, X, ls, var) + noise * torch.eye(N, dtype=X.dtype, device=X.device)
    return torch.log(torch.diagonal(torch.linalg.cholesky(Kt))).sum()


def exact_log_marginal(kind, X, y, ls, var, noise, mean):
    """log N(y | mean, K_ff + s I)."""
    N = X.shape[0]
    Kt = kernel_matrix(kind, X, X, ls, var) + noise * torch.eye(N, dtype=X.dtype, device=X.device)
    Lk = torch.linalg.cholesky(Kt)
    e = (y - mean).reshape(-1, 1)
    a = torch.linalg.solve_triangular(Lk, e, upper=False)
    return -0.5 * (a * a).sum() - torch.log(torch.diagonal(Lk)).sum() - 0.5 * N * math.log(2.0 * math.pi)
