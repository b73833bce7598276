"""Deterministic synthetic regression sets for benchmarks and examples.

The reference loads UCI sets through robustgp_experiments (cglb_experiments/datasets.py:47-76: z-normalise,
67/33 split); those need a network download, so the benchmarks use this generator of the same shape:
X ~ N(0,1)^{N x D} (already unit variance like datasets.py:35-39), y = sin(X a) + 0.1 eps z-normalised,
Z = first M rows of a seeded permutation of X (stand-in for robustgp's greedy conditional-variance init,
cglb/backend/config.py:62-65)."""
from __future__ import annotations

import math

import numpy as np


def synthetic_problem(N: int, D: int, M: int, seed: int = 0, dtype=np.float64, P: int = 1):
    """P = 1: y [N].  P > 1: Y [N, P]; column 0, X and Z are exactly the P = 1 arrays, the further columns sin(X a_b + phase_b) + noise
    come from one generator per column, so that they do not disturb that stream and column b is the same whatever P."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    a = rng.standard_normal(D) / math.sqrt(D)
    y = np.sin(X @ a) + 0.1 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    perm = rng.permutation(N)
    Z = X[perm[:M]].copy()
    if P > 1:
        cols = [y]
        for b in range(1, P):
            rng_p = np.random.default_rng([seed, b])   # per column: the sets are nested, column b is the same for every P > b
            ab = rng_p.standard_normal(D) / math.sqrt(D)
            yb = np.sin(X @ ab + rng_p.uniform(0.0, math.pi)) + 0.1 * rng_p.standard_normal(N)
            cols.append((yb - yb.mean()) / yb.std())
        y = np.stack(cols, axis=1)
    return X.astype(dtype), y.astype(dtype), Z.astype(dtype)


def reference_init_hypers(D: int):
    """cglb/backend/config.py:74-76 (variance=1, lengthscales=1) and :104-107 (noise=1); mean 0."""
    return dict(lengthscales=np.ones(D), variance=1.0, noise=1.0, mean=0.0)


def trained_like_hypers(D: int):
    """A point typical of a trained model: longer lengthscales, small noise (harder system, more CG steps)."""
    return dict(lengthscales=np.full(D, 1.5), variance=1.0, noise=0.05, mean=0.0)
