"""Launch-geometry cases of the symmetric K_ff mat-vec (test helper, not a test module; runs on any CPU).

Which work list and slab layout a mat-vec gets is decided from N, the rows-per-lane class R of (dtype, D), the column chunk and the
world size (kernels_kff_sym.hip: kff_sym_generic, ensure_sym_items).  The large-N branches of that decision are brought down to
N <= ~3100, where the fp64 direct-difference oracle is cheap, by forcing the chunk with the option `sym_chunk`.

The covering design (shared by tests/test_gpu_sym_geometry.py and, for its discrimination claim, tests/test_geometry_cases_host.py):

* CLASSES: one (dtype, D) per rows-per-lane class - fp64 D = 3 (R = 8), 8 (R = 4), 12 (R = 4, the CGLB_SYM_R4_MAX_DP edge), 16 (R = 2),
  20 (R = 1), 50 (R = 1, the mid-width instance of padded width 64, wide_reg 1); fp32 D = 3 (R = 8), 16 (R = 4), 24 (R = 2);
* CHUNKS: every forced chunk value with every class (9 x 7 cells): 16, 128, 256, 512, 1000 (rounds to 1008), 1024, 4096 (clamps to 1024);
* the three two-valued axes (sym_order, kernel kind, precision) are NOT crossed with the cells: cell number x = class index + chunk
  index takes sym_order = x % 2, kind = (x // 2) % 2, precision = (x // 4) % 2.  The seven cells of a class have seven consecutive x,
  and any seven consecutive integers hold both values of each of the three digits: every value of every axis meets every class
  (asserted in the host test), 63 cells instead of 504;
* per cell two or three N (`sizes`): chunk + 1 (a second chunk of one column), 2 chunk + RBROWS + 17 (three chunks, the diagonal block
  of a row block cut by a chunk edge) and, where four row blocks are narrower than the chunk (4 RBROWS < chunk: several groups share
  one diagonal chunk and a group holds -1 entries right of it), 3 chunk + 5; each moved up until it is ragged against 16, 64, RBROWS,
  4 RBROWS and the chunk.
"""
from __future__ import annotations

import numpy as np

import fp32_error_model as em
from oracle import cglb_oracle as orc

CLASSES = (("fp64", 3, {}), ("fp64", 8, {}), ("fp64", 12, {}), ("fp64", 16, {}), ("fp64", 20, {}), ("fp64", 50, {"wide_reg": 1}),
           ("fp32", 3, {}), ("fp32", 16, {}), ("fp32", 24, {}))
CHUNKS = (16, 128, 256, 512, 1000, 1024, 4096)
ATOL64 = 2e-12   # fp64 mat-vec: |out - ref| <= ATOL64 * max|ref| (tests/test_gpu_kff_variants.py)


def rbrows(dtype: str, D: int) -> int:
    return 64 * em.rows_per_lane(D, dtype)


def eff_chunk(opt: int) -> int:
    """The launcher's rounding and clamp of a forced chunk."""
    return min((opt + 15) // 16 * 16, 1024)


def sizes(dtype: str, D: int, opt: int):
    rb, ch = rbrows(dtype, D), eff_chunk(opt)
    out = [ch + 1, 2 * ch + rb + 17]
    if 4 * rb < ch:
        out.append(3 * ch + 5)
    ragged = []
    for n in out:
        while any(n % m == 0 for m in (16, 64, rb, 4 * rb, ch)):
            n += 1
        ragged.append(n)
    return ragged


def cells():
    """(id, dtype, D, extra options, forced chunk, sym_order, kind, precision) of the 63 cells."""
    out = []
    for i, (dtype, D, extra) in enumerate(CLASSES):
        for c, opt in enumerate(CHUNKS):
            x = i + c
            order, kind, prec = x % 2, em.KINDS[(x // 2) % 2], (x // 4) % 2
            out.append((f"{dtype}-D{D}-c{opt}-o{order}-{kind}-p{prec}", dtype, D, dict(extra), opt, order, kind, prec))
    return out


def pairs_closed_form(n: int, rb: int, world: int = 1, rank: int = 0) -> int:
    """Kernel pairs one launch evaluates: every row block of the rank against the columns at or right of its first row,
    sum_rb rows(rb) (n - rbase(rb)) - whatever the chunk and the item order."""
    total = 0
    for b in range(rank, (n + rb - 1) // rb, world):
        rbase = b * rb
        total += min(rb, n - rbase) * (n - rbase)
    return total


def problem(N: int, D: int, seed: int = 0):
    """Inputs of a cell: `fp32_error_model.problem` (float32-representable values, so that an fp32 and an fp64 context hold the same
    numbers; lengthscales ~ 0.6 sqrt(D): kernel values of order 0.01 ... 1 over the whole matrix)."""
    return em.problem(N, D, seed=seed)


def reference_case(kind, dtype, X, hyp, p, chunk, r0=0, r1=None, need_K=False) -> em.MatvecCase:
    """THE reference of every geometry test, on the GPU and in the host discrimination test alike: reference, per-row tolerance scale,
    chunk and (need_K, for the planted defects) the kernel rows.  fp32 - the round-off model with the accumulation depth of the forced
    chunk (the bound is TAU['matvec'] * s); fp64 - the blocked C oracle's direct-difference mat-vec (oracle.cglb_oracle_c.kff_matvec) with
    the constant ATOL64 * max|ref| over all N rows in `s` (the bound is 1 * s)."""
    if dtype == "fp32":
        return em.matvec_case(kind, X, hyp, p, r0=r0, r1=r1, chunk=chunk)
    from oracle import cglb_oracle_c as orcc
    r1 = X.shape[0] if r1 is None else r1
    full = orcc.kff_matvec(kind, X, hyp, p)
    K = orc.kernel_matrix(kind, X[r0:r1], X, hyp.lengthscales, hyp.variance) if need_K else None
    return em.MatvecCase(full[r0:r1], np.full(r1 - r0, ATOL64 * np.abs(full).max()), K, chunk)


def bound(dtype: str) -> float:
    """Admissible max_i |out_i - ref_i| / s_i of `reference_case`."""
    return em.TAU["matvec"] if dtype == "fp32" else 1.0


# --------------------------------------------------------------------------- GPU side (imported lazily: the module itself needs no GPU)
def make_ctx(kind, dtype, X, hyp, options, row_range=None):
    import torch
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, np.zeros(len(X)), hyp.Z.shape[0], kind, dtype=torch.float64 if dtype == "fp64" else torch.float32, row_range=row_range)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    return ctx


def reference(kind, dtype, X, hyp, p, chunk, r0=0, r1=None):
    """(ref, s, bound) of `reference_case`."""
    case = reference_case(kind, dtype, X, hyp, p, chunk, r0, r1)
    return case.ref, case.s, bound(dtype)


def check(out, ref, s, bound, what):
    r = em.ratio(out, ref, s)
    print(f"{what}: max |out - ref| / s = {r:.3g} (bound {bound})")
    assert r <= bound, what


def matvec_dot(ctx, p):
    import torch
    from ctypes import c_void_p
    from cglb_amd import _lib
    pd = ctx._dev(p, ctx.N)
    out = ctx.empty(ctx.nloc)
    dot = torch.zeros(1, dtype=torch.float64, device=ctx.device)
    _lib.check(ctx.lib.cglb_matvec_dot(ctx._ctx, c_void_p(pd.data_ptr()), c_void_p(out.data_ptr()), c_void_p(dot.data_ptr())), ctx._ctx)
    return out.double().cpu().numpy(), float(dot.cpu()[0])


def matvec_cyclic(ctx, p_dev, world, rank):
    import torch
    from ctypes import c_void_p
    from cglb_amd import _lib
    _lib.check(ctx.lib.cglb_set_parallel(ctx._ctx, world, rank), ctx._ctx)
    out = torch.empty(ctx.N, dtype=ctx.dtype, device=ctx.device)
    _lib.check(ctx.lib.cglb_matvec_cyclic(ctx._ctx, c_void_p(p_dev.data_ptr()), c_void_p(out.data_ptr())), ctx._ctx)
    return out.double().cpu().numpy()
