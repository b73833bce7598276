"""Matern-5/2 reference (test helper, not a test module; runs on any CPU).

    k = f (1 + s + s^2 / 3) exp(-s),   h = 5/3 f (1 + s) exp(-s),   s = sqrt(5) r,   r^2 = sum_d ((x_d - x'_d) / l_d)^2

with h in the convention of `oracle.cglb_oracle.kernel_grad_factor`: dk/dl_d = h delta_d^2 / l_d, dk/dx_d = -h delta_d / l_d.

The oracle package knows RBF and Matern-3/2 only and is not edited.  It resolves `kernel_from_sqdist`, `kernel_grad_factor` and `KINDS`
through its module globals, so `oracle_with_matern52()` swaps them for wrappers that add kind 2 and delegate every other kind to the
originals - for the duration of a `with` block only.  Everything built on the oracle (`objective`, `objective_grad`, `predict`,
`common_terms`, `roundoff_sensitivity`, and the helpers gpr_ref, itergp_ref, predict_ref, geometry_cases, multi_output_ref,
fp32_error_model) then works for "matern52" unchanged.  tests/bound_variants_ref.py has a torch `kernel_matrix` of its own; it is
swapped the same way for the torch closed form below.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

from oracle import cglb_oracle as orc

KIND = "matern52"
KIND_ID = 2
SQRT5 = math.sqrt(5.0)


def k52(d2, var):
    s = SQRT5 * np.sqrt(d2)
    return var * (1.0 + s + s * s / 3.0) * np.exp(-s)


def h52(d2, var):
    s = SQRT5 * np.sqrt(d2)
    return (5.0 / 3.0) * var * (1.0 + s) * np.exp(-s)


def k32(d2, var):
    """The Matern-3/2 profile (what a kernel that fell through to the 3/2 branch would compute)."""
    s = math.sqrt(3.0) * np.sqrt(d2)
    return var * (1.0 + s) * np.exp(-s)


def h32(d2, var):
    return 3.0 * var * np.exp(-math.sqrt(3.0) * np.sqrt(d2))


def _is52(kind) -> bool:
    return kind == KIND_ID or (isinstance(kind, str) and kind in ("matern52", "Matern52", "mat52"))


@contextlib.contextmanager
def oracle_with_matern52(profile=k52, grad_factor=h52):
    """Teach the oracle kind 2 for the duration of the block.  `profile` / `grad_factor`: the functions used for kind 2 (the host tests
    hand in the Matern-3/2 ones to show that the GPU tests' tolerances tell the two apart)."""
    saved = (orc.kernel_from_sqdist, orc.kernel_grad_factor, dict(orc.KINDS))
    kinds = orc.KINDS
    orig_k, orig_h = saved[0], saved[1]

    def kernel_from_sqdist(kind, d2, var):
        return profile(d2, var) if _is52(kind) else orig_k(kind, d2, var)

    def kernel_grad_factor(kind, d2, var):
        return grad_factor(d2, var) if _is52(kind) else orig_h(kind, d2, var)

    orc.kernel_from_sqdist, orc.kernel_grad_factor = kernel_from_sqdist, kernel_grad_factor
    for name in ("matern52", "Matern52", "mat52"):
        kinds[name] = KIND_ID
    try:
        yield orc
    finally:
        orc.kernel_from_sqdist, orc.kernel_grad_factor = orig_k, orig_h
        kinds.clear()
        kinds.update(saved[2])


def torch_kernel_matrix(kind, X1, X2, ls, var):
    """bound_variants_ref.kernel_matrix with the Matern-5/2 closed form (d^2 clamped before the root, as that file does)."""
    import torch
    if not _is52(kind):
        return bref_kernel_matrix_original(kind, X1, X2, ls, var)
    a, b = X1 / ls, X2 / ls
    d2 = torch.zeros((X1.shape[0], X2.shape[0]), dtype=X1.dtype, device=X1.device)
    for d in range(X1.shape[1]):
        d2 = d2 + (a[:, d, None] - b[None, :, d]) ** 2
    s = SQRT5 * torch.sqrt(d2.clamp_min(1e-300))
    return var * (1.0 + s + s * s / 3.0) * torch.exp(-s)


bref_kernel_matrix_original = None


@contextlib.contextmanager
def bound_variants_with_matern52():
    """bound_variants_ref with the torch closed form for kind 2, inside `oracle_with_matern52()` (its `orc.kind_id` needs the name)."""
    global bref_kernel_matrix_original
    import bound_variants_ref as bref
    with oracle_with_matern52():
        bref_kernel_matrix_original = bref.kernel_matrix
        bref.kernel_matrix = torch_kernel_matrix
        try:
            yield bref
        finally:
            bref.kernel_matrix = bref_kernel_matrix_original
            bref_kernel_matrix_original = None


def dense_matvec(X, hyp, p, profile=k52, r0=0, r1=None):
    """(K_ff + noise I)[r0:r1] p by direct differences in numpy (the blocked C oracle has no Matern-5/2)."""
    r1 = X.shape[0] if r1 is None else r1
    K = profile(orc.scaled_sqdist(X[r0:r1], X, np.asarray(hyp.lengthscales, dtype=np.float64)), hyp.variance)
    return K @ p + hyp.noise * p[r0:r1]
