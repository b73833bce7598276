"""Multi-output truth composed from the single-output oracle (oracle/cglb_oracle.py), shared by the multi-output tests.

`lockstep_pcg` restates the batched solver's semantics in numpy: P independent preconditioned CG recurrences (conjugate_gradient.py:41-86
per column, own gamma_b and beta_b) that share the stop test 1/2 sum_b r_b^T P r_b <= max_error and the restart step; a zero p^T A p gives
gamma_b = 0 and a zero r^T P r gives beta_b = 0.  For a fixed V the bound, gradient and prediction are sums / per-column calls of the
single-output oracle: every single bound carries one log-det and one constant, so the sum is the multi-output bound exactly."""
from __future__ import annotations

import numpy as np

from oracle import cglb_oracle as orc

GRAD_KEYS = ("lengthscales", "variance", "noise", "mean", "Z")


def lockstep_pcg(cov, B, V0, precond, max_error=1.0, max_cg_iter=100, restart_cg_iter=40):
    """cov [N, N]; B, V0 [N, P].  Returns (V [N, P], steps, per-column 1/2 r^T P r [P])."""
    P = B.shape[1]
    V = V0.copy()
    R = B - cov @ V
    Z, rz = np.empty_like(R), np.empty(P)
    for b in range(P):
        Z[:, b], rz[b] = precond(R[:, b])
    Pd = Z.copy()
    i = 0
    while 0.5 * rz.sum() > max_error and i < max_cg_iter:
        Ap = cov @ Pd
        pap = (Pd * Ap).sum(0)
        gamma = np.where(pap == 0.0, 0.0, rz / np.where(pap == 0.0, 1.0, pap))
        V = V + gamma * Pd
        restart = i % restart_cg_iter == restart_cg_iter - 1
        R = (B - cov @ V) if restart else (R - gamma * Ap)
        new_rz = np.empty(P)
        for b in range(P):
            Z[:, b], new_rz[b] = precond(R[:, b])
        beta = np.where(rz == 0.0, 0.0, new_rz / np.where(rz == 0.0, 1.0, rz))
        Pd = Z.copy() if restart else Z + Pd * beta
        rz = new_rz
        i += 1
    return V, i, 0.5 * rz


def stable_steps(cov, B, V0, precond, max_error, **kw):
    """Steps of the lockstep loop, asserted equal under a +-1e-10 perturbation of max_error: a step-count mismatch is then a failure of the
    code under test, not noise."""
    V, steps, half = lockstep_pcg(cov, B, V0, precond, max_error, **kw)
    for eps in (-1e-10, 1e-10):
        assert lockstep_pcg(cov, B, V0, precond, max_error + eps, **kw)[1] == steps, "fixture: stop step not stable"
    return V, steps, half


def composed_objective(kind, X, Y, hyp, V, with_grad=True, cov=None):
    """Sum over the columns of the single-output evaluation at v_b (run_cg False)."""
    cov = orc.dense_cov(kind, X, hyp) if cov is None else cov
    tot = dict(bound=0.0, lower=0.0, upper=0.0, logdet=0.0)
    grad = None
    for b in range(Y.shape[1]):
        o = orc.objective(kind, X, Y[:, b], hyp, V[:, b], run_cg=False, with_grad=with_grad, cov=cov)
        for k in tot:
            tot[k] += getattr(o, k)
        if with_grad:
            grad = {k: np.asarray(o.grad[k], dtype=np.float64).copy() for k in GRAD_KEYS} if grad is None else \
                {k: grad[k] + np.asarray(o.grad[k]) for k in GRAD_KEYS}
    return tot, grad


def problem(N, D, M, P, seed=0, trained=True):
    """(X, Y [N, P], hypers): the oracle's synthetic inputs with P target columns of different frequencies."""
    X, y, Z = orc.synthetic_problem(N, D, M, seed=seed)
    rng = np.random.default_rng(seed + 77)
    cols = [y]
    for b in range(1, P):
        a = rng.standard_normal(D) / np.sqrt(D)
        yb = np.cos((1.0 + 0.5 * b) * (X @ a)) + 0.1 * rng.standard_normal(N)
        cols.append((yb - yb.mean()) / yb.std())
    hyp = orc.trained_like_hypers(D, Z) if trained else orc.reference_init_hypers(D, Z)
    return X, np.stack(cols, axis=1), hyp
