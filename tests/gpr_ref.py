"""Dense numpy / scipy restatement of the exact GP regression objective (test helper, not a test module).

    K = f kappa(X, X) + s I = L L^T,  e = y - c,  alpha = K^-1 e
    lml = -1/2 e^T alpha - sum log L_ii - N/2 log 2 pi          (gpflow GPR.log_marginal_likelihood; the quantity behind
                                                                  ExactMarginalLogLikelihood times n, cglb/backend/pytorch/interface.py:568-569)
    W = alpha alpha^T - K^-1
    d lml / d l_d = 1/2 sum_ij W_ij h_ij delta_ijd^2 / l_d      h: oracle.kernel_grad_factor, delta_ijd = (x_id - x_jd) / l_d
    d lml / d f   = 1/2 sum_ij W_ij kappa_ij
    d lml / d s   = 1/2 tr W
    d lml / d c   = sum_i alpha_i
    predict_f:  mean = c + K_*f alpha,  var = f - |L^-1 K_f*|^2 column-wise;  the log density adds s to the variance.

Built on oracle/cglb_oracle.py (`scaled_sqdist`, `kernel_from_sqdist`, `kernel_grad_factor`), imported and not modified.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import scipy.linalg

from oracle import cglb_oracle as orc


@dataclass
class GPRRef:
    lml: float
    quad: float     # -1/2 e^T alpha
    logdet: float   # -sum log L_ii
    grad: Optional[Dict[str, np.ndarray]]
    L: np.ndarray
    alpha: np.ndarray


def hypers(D: int, trained: bool) -> dict:
    """The two hyper-parameter sets of the tests: the reference's initial values, and a trained-like set."""
    if trained:
        return dict(lengthscales=np.full(D, 1.5 if D < 8 else 2.5), variance=1.0, noise=0.05, mean=0.1)
    return dict(lengthscales=np.ones(D), variance=1.0, noise=1.0, mean=0.0)


def evaluate(kind, X, y, lengthscales, variance, noise, mean, with_grad: bool = True) -> GPRRef:
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ls = np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (X.shape[1],))
    N = X.shape[0]
    d2 = orc.scaled_sqdist(X, X, ls)
    K = orc.kernel_from_sqdist(kind, d2, variance)
    K[np.diag_indices_from(K)] += noise
    L = np.linalg.cholesky(K)
    e = y - mean
    alpha = scipy.linalg.cho_solve((L, True), e)
    quad = -0.5 * float(e @ alpha)
    logdet = -float(np.log(np.diagonal(L)).sum())
    lml = quad + logdet - 0.5 * N * math.log(2.0 * math.pi)
    grad = None
    if with_grad:
        Kinv, info = scipy.linalg.lapack.dpotri(L, lower=1)
        assert info == 0
        Kinv = np.tril(Kinv) + np.tril(Kinv, -1).T
        W = np.outer(alpha, alpha) - Kinv
        K[np.diag_indices_from(K)] -= noise
        g_var = 0.5 * float((W * K).sum()) / variance
        Wh = W * orc.kernel_grad_factor(kind, d2, variance)
        Xs = X / ls
        g_ls = np.empty(X.shape[1])
        for d in range(X.shape[1]):
            diff = Xs[:, d][:, None] - Xs[:, d][None, :]
            g_ls[d] = 0.5 * float((Wh * diff * diff).sum()) / ls[d]
        grad = {"lengthscales": g_ls, "variance": g_var, "noise": 0.5 * float(np.trace(W)), "mean": float(alpha.sum())}
    return GPRRef(lml, quad, logdet, grad, L, alpha)


def lml_only(kind, X, y, lengthscales, variance, noise, mean) -> float:
    return evaluate(kind, X, y, lengthscales, variance, noise, mean, with_grad=False).lml


def predict(kind, X, ref: GPRRef, lengthscales, variance, mean, Xnew):
    """(f_mean, f_var) at Xnew from the factor and alpha of `ref`."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    Xnew = np.asarray(Xnew, dtype=np.float64).reshape(len(Xnew), -1)
    ls = np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (X.shape[1],))
    Kfs = orc.kernel_from_sqdist(kind, orc.scaled_sqdist(X, Xnew, ls), variance)
    V = scipy.linalg.solve_triangular(ref.L, Kfs, lower=True)
    return mean + Kfs.T @ ref.alpha, variance - (V * V).sum(axis=0)


def grad_vector(g: dict) -> np.ndarray:
    return np.concatenate([np.asarray(g["lengthscales"], dtype=np.float64).reshape(-1), [g["variance"], g["noise"], g["mean"]]])


#: (N, D, gpr_block; None = the default) of the GPU tests: N = 1, N = 2, one short / one full / one full and a one-row block, two full
#: outer blocks and a one-row third, wide inputs with a ragged last block, a dozen outer blocks, and a size that crosses the default edge
SHAPES = [(1, 1, None), (2, 3, None), (63, 3, 64), (64, 3, 64), (65, 3, 64), (257, 1, 128), (300, 40, 128), (1500, 8, 128), (2999, 3, None)]


def problem(N: int, D: int):
    """The synthetic training set of a shape (cglb_amd.data.synthetic_problem, seed N + D)."""
    from cglb_amd.data import synthetic_problem
    if N == 1:  # the generator standardises y by its own deviation, which one point does not have: the first of two points
        X, y, _ = synthetic_problem(2, D, 1, seed=N + D)
        return X[:1].copy(), y[:1].copy()
    X, y, _ = synthetic_problem(N, D, 1, seed=N + D)
    return X, y
