"""Numpy restatement of the Lanczos variance cache of the iterative exact-GP class (test helper, not a test module), as the library's
cglb_itergp_var_cache / cglb_itergp_predict_cached define it (include/cglb_hip.h).

    K = f kappa(X, X) + s I,  e = y - c
    Lanczos with full reorthogonalisation, q_0 = e / |e|:  w = K q_j,  alpha_j = q_j^T w,  two passes w <- w - Q (Q^T w) over all columns so far,
        beta_j = |w|;  J = j + 1 columns when j + 1 = r or beta_j <= 1e-10 alpha_0, else q_{j+1} = w / beta_j
    T = tridiag(alpha, beta) = L L^T, L lower bidiagonal (d, l);  R_j = (Q_j - l_{j-1} R_{j-1}) / d_j, so that K^-1 ~ R R^T
    f_var(x*) = f - sum_s (sum_j f kappa(x*, x_j) R[j, s])^2       (the mean is that of the exact predictive)

A Galerkin projection of K^-1: f_var is never below the exact variance, does not increase with r and is exact at J = N.

Built on oracle/cglb_oracle.py and tests/gpr_ref.py, imported and not modified.  `wobble`: relative size of a symmetric random perturbation of
every kernel value (the round-off model of itergp_ref.bilinear_forms); the `defect_*` arguments plant the mistakes a kernel could make, to
show that the GPU tolerances see them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from oracle import cglb_oracle as orc

import gpr_ref

#: (N, D) of the cases the GPU tests of the cache use, with the hyper-parameters of itergp_ref.exact_limit_hypers
CASES = [(40, 3), (67, 2), (300, 3)]
#: ranks of the GPU comparison against this restatement
RANKS = [1, 8, 9, 33]
STOP = 1e-10


def hypers(D: int) -> dict:
    from itergp_ref import exact_limit_hypers
    return exact_limit_hypers(D)


def new_points(N: int, D: int, n_new: int = 9) -> np.ndarray:
    """New points of a case: standard normal like the training inputs, the first one ON training row 0 and the last one far outside."""
    X, _ = gpr_ref.problem(N, D)
    Xn = np.random.default_rng(1000 + N + D).standard_normal((n_new, D))
    Xn[0] = X[0]
    if n_new > 2:
        Xn[-1] = 4.0
    return Xn


@dataclass
class LoveRef:
    J: int
    alpha: np.ndarray    # [J]
    beta: np.ndarray     # [J]; beta[J - 1] is the norm the run stopped on
    R: np.ndarray        # [N, r_pad], r_pad = J rounded up to 8, zero padded
    Q: np.ndarray        # [N, J]


def kernel_matrices(kind, X, Xnew, lengthscales, variance, wobble: float = 0.0, seed: int = 0):
    """(f kappa(X, X), f kappa(Xnew, X)), every value moved by a relative `wobble` (symmetric on the square one)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    ls = np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (X.shape[1],))
    Kff = orc.kernel_from_sqdist(kind, orc.scaled_sqdist(X, X, ls), variance)
    Ksf = None
    if Xnew is not None:
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(len(Xnew), -1)
        Ksf = orc.kernel_from_sqdist(kind, orc.scaled_sqdist(Xnew, X, ls), variance)
    if wobble:
        rng = np.random.default_rng(seed)
        Rm = rng.uniform(-1.0, 1.0, Kff.shape)
        Kff = Kff * (1.0 + wobble * (np.triu(Rm) + np.triu(Rm, 1).T))
        if Ksf is not None:
            Ksf = Ksf * (1.0 + wobble * rng.uniform(-1.0, 1.0, Ksf.shape))
    return Kff, Ksf


def bidiagonal_factor(alpha, beta):
    """(d, l) of T = L L^T; ValueError at a pivot that is not positive (csrc/lanczos_host.h)."""
    J = len(alpha)
    d, l = np.zeros(J), np.zeros(J)
    lprev = 0.0
    for j in range(J):
        pivot = alpha[j] - lprev * lprev
        if not pivot > 0.0 or not math.isfinite(pivot):
            raise ValueError(f"pivot {j} is not positive")
        d[j] = math.sqrt(pivot)
        if j + 1 < J:
            l[j] = beta[j] / d[j]
            lprev = l[j]
    return d, l


def build(K: np.ndarray, e: np.ndarray, r: int, passes: int = 2) -> LoveRef:
    """The cache of rank r for K (noise included) and the start vector e."""
    N = K.shape[0]
    assert 1 <= r <= min(N, 1024)
    nrm = float(np.linalg.norm(e))
    if nrm == 0.0:
        raise ValueError("e = 0")
    Q = np.zeros((N, r))
    Q[:, 0] = e / nrm
    alpha, beta = [], []
    for j in range(r):
        w = K @ Q[:, j]
        alpha.append(float(Q[:, j] @ w))
        for _ in range(passes):
            w = w - Q[:, :j + 1] @ (Q[:, :j + 1].T @ w)
        beta.append(float(np.linalg.norm(w)))
        if j + 1 == r or beta[j] <= STOP * alpha[0]:
            break
        Q[:, j + 1] = w / beta[j]
    J = len(alpha)
    alpha, beta = np.array(alpha), np.array(beta)
    d, l = bidiagonal_factor(alpha, beta)
    r_pad = (J + 7) // 8 * 8
    R = np.zeros((N, r_pad))
    for j in range(J):
        R[:, j] = (Q[:, j] - (l[j - 1] * R[:, j - 1] if j else 0.0)) / d[j]
    return LoveRef(J, alpha, beta, R, Q[:, :J].copy())


def variance_from_cache(Ksf: np.ndarray, R: np.ndarray, variance: float, defect_drop_group: Optional[int] = None,
                        defect_stale_pad: Optional[float] = None, defect_drop_rows: int = 0, J: Optional[int] = None) -> np.ndarray:
    """f - |K_*f R|^2 row-wise.  Defects: a lost group of 8 cache columns; a padded column (one past J) that holds `defect_stale_pad`
    instead of zero; the last `defect_drop_rows` training rows lost from the sums."""
    R = R.copy()
    if defect_stale_pad is not None:
        assert J is not None and J < R.shape[1], "no padded column to leave stale"
        R[:, J] = defect_stale_pad
    if defect_drop_rows:
        R[R.shape[0] - defect_drop_rows:] = 0.0
    B = Ksf @ R
    if defect_drop_group is not None:
        B[:, 8 * defect_drop_group: 8 * defect_drop_group + 8] = 0.0
    return variance - (B * B).sum(axis=1)


def predict_var(kind, X, y, lengthscales, variance, noise, mean, Xnew, r: int, wobble: float = 0.0, seed: int = 0, passes: int = 2, **defects):
    """(f_var [n_new], LoveRef) of the cached predictive of rank r."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Kff, Ksf = kernel_matrices(kind, X, Xnew, lengthscales, variance, wobble, seed)
    K = Kff + noise * np.eye(len(X))
    ref = build(K, y - mean, r, passes)
    return variance_from_cache(Ksf, ref.R, variance, J=ref.J, **defects), ref


def exact_var(kind, X, y, lengthscales, variance, noise, mean, Xnew) -> np.ndarray:
    """The exact predictive variance (gpr_ref.predict)."""
    g = gpr_ref.evaluate(kind, X, y, lengthscales, variance, noise, mean, with_grad=False)
    return gpr_ref.predict(kind, X, g, lengthscales, variance, mean, Xnew)[1]
