"""Numpy restatement of the iterative exact-GP estimator (test helper, not a test module): batched preconditioned CG with stochastic
Lanczos quadrature, as the library's cglb_itergp_* entry points define it (include/cglb_hip.h).

    K = f kappa(X, X) + s I,  e = y - c,  P = Q_ff + s I with Z = the k greedily selected training points,  A = L^-1 K_uf / sqrt(s)
    probes      z_i = sqrt(s) (A^T eps_i[:k] + eps_i[k:])                       (covariance P for eps_i ~ N(0, I))
    one solve   K [alpha, a_1 .. a_t] = [e, z_1 .. z_t], no restart steps, stop on 1/2 sum_b r_b^T P^-1 r_b <= max_error (the rule of oracle.pcg, summed)
    log|K|   ~= log|P| + (1/t) sum_i rz_0i e_1^T log(T_i) e_1,  log|P| = N log s + 2 sum log diag LB
    lml         = -1/2 e^T alpha - 1/2 log|K| - N/2 log 2 pi
    gradient    g = sum_b u_b^T (dK) v_b,  (u_0, v_0) = (alpha / 2, alpha),  (u_i, v_i) = (-a_i / (2 t), P^-1 z_i);  mean entry sum alpha

Built on oracle/cglb_oracle.py and tests/gpr_ref.py, imported and not modified.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from oracle import cglb_oracle as orc


#: (N, D, k) of the exact-limit checks, and their hyper-parameters: the trained-like set of gpr_ref with noise 0.2
EXACT_LIMIT_CASES = [(40, 3, 6), (67, 2, 9)]


def exact_limit_hypers(D: int) -> dict:
    from gpr_ref import hypers
    return dict(hypers(D, True), noise=0.2)


@dataclass
class IterGPRef:
    lml: float
    quad: float          # -1/2 e^T alpha
    logdet: float        # -1/2 log|K|, estimated
    logdet_P: float      # log|P|
    correction: float    # (1/t) sum_i rz_0i e_1^T log(T_i) e_1
    grad: Optional[Dict[str, np.ndarray]]
    steps: int
    half_rz: float
    rz_log: np.ndarray   # [steps + 1, 1 + t]
    pap_log: np.ndarray  # [steps, 1 + t]
    V: np.ndarray        # [N, 1 + t] solutions; column 0 is alpha
    pivots_Z: np.ndarray


def unit_probes(k: int, N: int) -> np.ndarray:
    """eps = sqrt(t) I, t = k + N: sum_i z_i z_i^T = t P exactly, so the estimator has no sampling error left."""
    t = k + N
    return math.sqrt(t) * np.eye(t)


def usable_steps(rz, pap, col, lanczos_iter) -> int:
    J = min(pap.shape[0], lanczos_iter)
    for j in range(J):
        r = rz[j, col]
        with np.errstate(all="ignore"):
            g = r / pap[j, col]
        if r == 0.0 or not np.isfinite(r) or g == 0.0 or not np.isfinite(g):
            return j
    return J


def tridiagonal(rz, pap, col, J):
    diag, off = np.zeros(J), np.zeros(J)
    for j in range(J):
        gamma = rz[j, col] / pap[j, col]
        diag[j] = 1.0 / gamma
        if j > 0:
            gp = rz[j - 1, col] / pap[j - 1, col]
            diag[j] += (rz[j, col] / rz[j - 1, col]) / gp
        if j + 1 < J:
            off[j] = math.sqrt(rz[j + 1, col] / rz[j, col]) / gamma
    return diag, off


def e1_log_e1(diag, off) -> float:
    J = len(diag)
    T = np.diag(diag) + np.diag(off[:J - 1], 1) + np.diag(off[:J - 1], -1)
    lam, V = np.linalg.eigh(T)
    return float((V[0] ** 2 * np.log(lam)).sum())


def logdet_correction(rz, pap, lanczos_iter) -> float:
    t = rz.shape[1] - 1
    total = 0.0
    for i in range(1, t + 1):
        J = usable_steps(rz, pap, i, lanczos_iter)
        if J:
            total += rz[0, i] * e1_log_e1(*tridiagonal(rz, pap, i, J))
    return total / t


def batched_pcg(matmat, precond, B, V0, max_error, max_cg_iter):
    """oracle.pcg on the columns of B in lockstep, without restart steps: own gamma_b and beta_b per column, one stop test on the sum.  A zero
    denominator gives a zero factor.  Returns (V, steps, half_rz, rz_log, pap_log)."""
    def ratio(a, b):
        out = np.zeros_like(a)
        nz = b != 0.0
        out[nz] = a[nz] / b[nz]
        return out
    V = V0.copy()
    R = B - matmat(V) if np.any(V != 0.0) else B.copy()
    Zv = precond(R)
    rz = (R * Zv).sum(axis=0)
    Pd = Zv.copy()
    rz_log, pap_log = [rz.copy()], []
    i = 0
    while 0.5 * rz.sum() > max_error and i < max_cg_iter:
        AP = matmat(Pd)
        pap = (Pd * AP).sum(axis=0)
        gamma = ratio(rz, pap)
        V = V + Pd * gamma
        R = R - AP * gamma
        Zv = precond(R)
        new_rz = (R * Zv).sum(axis=0)
        Pd = Zv + Pd * ratio(new_rz, rz)
        rz = new_rz
        i += 1
        rz_log.append(rz.copy())
        pap_log.append(pap.copy())
    return V, i, 0.5 * float(rz.sum()), np.array(rz_log), np.array(pap_log).reshape(i, B.shape[1])


def evaluate(kind, X, y, lengthscales, variance, noise, mean, eps, k, jitter=1e-6, v0=None, max_error=1.0, max_cg_iter=1000, lanczos_iter=20,
             with_grad=True, perturb: float = 0.0, perturb_seed: int = 0) -> IterGPRef:
    """`perturb`: relative size of a symmetric random perturbation of every kernel value (the round-off model the GPU tolerances are measured with)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N, D = X.shape
    ls = np.array(np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (D,)))
    eps = np.asarray(eps, dtype=np.float64)
    t = eps.shape[0]
    k = min(k, N)
    assert eps.shape == (t, k + N)
    Z = orc.greedy_conditional_variance(X, k, lambda a, b, full_cov: (orc.kernel_matrix(kind, a, b, ls, variance) if full_cov
                                                                      else orc.kernel_diag(kind, a, variance)), jitter)
    hyp = orc.Hypers(ls, float(variance), float(noise), float(mean), Z, float(jitter))
    terms = orc.common_terms(kind, X, hyp)
    A, LB, s = terms.A, terms.LB, float(noise)
    d2 = orc.scaled_sqdist(X, X, ls)
    wobble = 1.0
    if perturb:
        Rm = np.random.default_rng(perturb_seed).uniform(-1.0, 1.0, (N, N))
        wobble = 1.0 + perturb * (np.triu(Rm) + np.triu(Rm, 1).T)
    kappa = orc.kernel_from_sqdist(kind, d2, 1.0) * wobble
    K = variance * kappa + s * np.eye(N)

    def precond(R):
        return np.stack([orc.nystrom_precond(A, LB, s, R[:, b])[0] for b in range(R.shape[1])], axis=1)

    e = y - mean
    Zp = math.sqrt(s) * (A.T @ eps[:, :k].T + eps[:, k:].T)          # [N, t]
    B = np.concatenate([e[:, None], Zp], axis=1)
    V0 = np.zeros_like(B)
    if v0 is not None:
        V0[:, 0] = np.asarray(v0, dtype=np.float64).reshape(-1)
    V, steps, half_rz, rz_log, pap_log = batched_pcg(lambda M_: K @ M_, precond, B, V0, max_error, max_cg_iter)
    alpha = V[:, 0]
    logdet_P = N * math.log(s) + 2.0 * float(np.log(np.diag(LB)).sum())
    corr = logdet_correction(rz_log, pap_log, lanczos_iter)
    quad = -0.5 * float(e @ alpha)
    logdet = -0.5 * (logdet_P + corr)
    lml = quad + logdet - 0.5 * N * math.log(2.0 * math.pi)
    grad = None
    if with_grad:
        U = np.concatenate([0.5 * alpha[:, None], -V[:, 1:] / (2.0 * t)], axis=1)
        W = np.concatenate([alpha[:, None], precond(Zp)], axis=1)
        grad = bilinear_forms(kind, X, ls, variance, U, W, d2=d2, wobble=wobble)
        grad["mean"] = float(alpha.sum())
    return IterGPRef(lml, quad, logdet, logdet_P, corr, grad, steps, half_rz, rz_log, pap_log, V, Z)


def bilinear_forms(kind, X, ls, variance, U, V, d2=None, wobble=1.0) -> Dict[str, np.ndarray]:
    """sum_b u_b^T (dK/d theta) v_b for theta = lengthscales, variance, noise; U, V: [N, S].  Also "abs": the same sums over absolute values of
    the terms (lengthscales and variance), the scale a tolerance on them refers to."""
    X = np.asarray(X, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64)
    if d2 is None:
        d2 = orc.scaled_sqdist(X, X, ls)
    G = U @ V.T                                     # sum_b u_bi v_bj
    Gabs = np.abs(U) @ np.abs(V).T
    H = orc.kernel_grad_factor(kind, d2, variance) * wobble
    kap = orc.kernel_from_sqdist(kind, d2, 1.0) * wobble
    Xs = X / ls
    g_ls, a_ls = np.empty(X.shape[1]), np.empty(X.shape[1])
    for d in range(X.shape[1]):
        diff = Xs[:, d][:, None] - Xs[:, d][None, :]
        g_ls[d] = float((G * H * diff * diff).sum()) / ls[d]
        a_ls[d] = float((Gabs * H * diff * diff).sum()) / ls[d]
    return {"lengthscales": g_ls, "variance": float((G * kap).sum()), "noise": float((U * V).sum()),
            "abs": np.concatenate([a_ls, [float((Gabs * kap).sum())]])}


def grad_vector(g: dict) -> np.ndarray:
    return np.concatenate([np.asarray(g["lengthscales"], dtype=np.float64).reshape(-1), [g["variance"], g["noise"], g["mean"]]])
