"""A context gives back the device memory it took, and a context that is used again computes what a fresh one computes.

Every device buffer of a context belongs to one of three pools ("Device memory of a context"): the context's own, the one of
the N^2M pass, the communicator's.  One "cycle" below creates contexts, drives them through every path that allocates on first use
or grows a buffer, and closes them:

  * fp64 rbf and matern32 with gradient (Guf, Mtmp3/4, gpart, uwh, slabs, sym_items, kpart), fp32;
  * precond_mode 1 (ppart); kff_variant 0 and 1 (kpart from its two other call sites, fragA/B);
  * a mid-width (D = 40) and a wide (D = 100) input (the w* buffers);
  * logdet_bound 2, then a changed n2m_tile and a second evaluation (the N^2M pool released and refilled); quad_term 1 (w_zero);
  * select_inducing and predict (per-call temporaries);
  * a communicator over callbacks at world size 1: evaluation, prediction (the gather buffer), cglb_comm_destroy, a plain mat-vec.

Everything runs in one spawned worker (the process group of the communicator lives there).  The worker runs one warm-up cycle - code
objects, rocBLAS workspaces and torch's caching allocator settle there - reads the free device memory, runs K = 8 more cycles and
reads it again.  Nothing here provokes an error on the GPU.

Bound on the drop of free memory over the K cycles.  The parent of the commit that introduced the pools released its buffers through
hand-kept lists that were checked against the structs and found complete, so what it shows is the noise of the measurement.  This same
test, run three times against that build on an MI355X, read drops of 2 097 152, 2 097 152 and 2 097 152 bytes (one 2 MiB granule, the same in
each run, whose owner was not tracked down; free memory 308 264 566 784 -> 308 262 469 632 bytes).  The smallest per-cycle leak the test claims
to catch is one full-length vector of the test shape, N x 8 bytes = 160 000 bytes, i.e. 1 280 000 bytes over K = 8 cycles; the bound is
therefore 2 097 152 + 1 280 000 = 3 377 152 bytes.  Buffers smaller than a full-length vector (chol_blk, the D-length scale vectors of the
wide path, the 4-entry scalar blocks) are below that resolution; that they are released follows from the structure instead: in
cglb_amd/csrc, hipMalloc( and hipFree( occur only inside the pool and the per-call DevTemps.

Reuse: every context is evaluated once more after a set_hypers change and its bound compared with a fresh context's at 1e-12 relative.
"""
import numpy as np
import pytest
import torch

from cglb_amd.data import synthetic_problem
from test_gpu_dist_backend import _init, _spawn

pytestmark = pytest.mark.gpu

N, M, K = 20000, 256, 8
PARENT_MAX_DROP = 2097152               # bytes; the largest of the three readings of the parent build (all three: 2 MiB)
BOUND = PARENT_MAX_DROP + N * 8 * K     # + one full-length fp64 vector per cycle


def _hypers(D, changed):
    ls = 1.5 * np.sqrt(D / 8.0)
    if changed:
        return dict(lengthscales=np.full(D, 1.15 * ls), variance=1.1, noise=0.12, mean=0.05)
    return dict(lengthscales=np.full(D, ls), variance=1.0, noise=0.1, mean=0.0)


def _evaluate(ctx, h, Z):
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
    v = torch.zeros(ctx.N, dtype=ctx.dtype, device=ctx.device)
    return ctx.objective_and_grad(v, run_cg=True, max_error=1.0), v


# (name, D, kind, dtype, options set before the first evaluation)
CASES = [
    ("rbf", 8, "rbf", torch.float64, {}),
    ("matern32", 8, "matern32", torch.float64, {}),
    ("fp32", 8, "rbf", torch.float32, {}),
    ("precond_implicit", 8, "matern32", torch.float64, {"precond_mode": 1}),
    ("kff_plain", 8, "matern32", torch.float64, {"kff_variant": 0}),
    ("kff_matrix_pipe", 8, "rbf", torch.float64, {"kff_variant": 1}),
    ("mid_width", 40, "rbf", torch.float64, {}),
    ("wide", 100, "matern32", torch.float64, {}),
    ("n2m", 8, "rbf", torch.float64, {"logdet_bound": 2}),
    ("exact_quad", 8, "rbf", torch.float64, {"logdet_bound": 1, "quad_term": 1}),
    ("select_predict", 8, "rbf", torch.float64, {}),
    ("communicator", 8, "rbf", torch.float64, {}),
]


def _make(name, data, kind, dtype, options):
    from cglb_amd.dist_context import DistHipContext
    from cglb_amd.hip_context import HipContext
    X, y, _ = data
    if name == "communicator":
        ctx = DistHipContext(X, y, M, kind, dtype=dtype, collectives="callbacks")
    else:
        ctx = HipContext(X, y, M, kind, dtype=dtype, device=torch.device("cuda", 0))
    for k, val in options.items():
        ctx.set_option(k, val)
    return ctx


def _cycle(problems):
    """One pass over CASES; returns {case: (bound of the used context after the set_hypers change, bound of a fresh context)}."""
    from cglb_amd.hip_context import HipContext
    out = {}
    for name, D, kind, dtype, options in CASES:
        data = problems[D]
        X, _, Z = data
        ctx = _make(name, data, kind, dtype, options)
        try:
            _, v = _evaluate(ctx, _hypers(D, False), Z)
            if name == "n2m":                      # drops the tiles of the N^2M pass; the next evaluation allocates them at the new edge
                ctx.set_option("n2m_tile", 2048)
                _evaluate(ctx, _hypers(D, False), Z)
            if name == "select_predict":
                h = _hypers(D, False)
                ctx.select_inducing(h["lengthscales"], h["variance"], return_Z=True)
                _, v = _evaluate(ctx, h, Z)        # select_inducing must be followed by set_hypers
            if name in ("select_predict", "communicator"):
                ctx.setup()
                ctx.predict(v, X[:3000])
            if name == "communicator":             # the context stays alive without its communicator and computes whole mat-vecs again
                assert ctx.lib.cglb_comm_destroy(ctx._ctx) == 0
                HipContext.matvec(ctx, v)
                ctx.close()
                ctx = _make(name, data, kind, dtype, options)
                _evaluate(ctx, _hypers(D, False), Z)
            used, _ = _evaluate(ctx, _hypers(D, True), Z)
        finally:
            ctx.close()
        ctx = _make(name, data, kind, dtype, options)
        try:
            if name == "n2m":
                ctx.set_option("n2m_tile", 2048)
            fresh, _ = _evaluate(ctx, _hypers(D, True), Z)
        finally:
            ctx.close()
        out[name] = (used.bound, fresh.bound)
    return out


def _worker(rank, world, port, q):
    dist = _init(rank, world, port, "gloo")
    try:
        problems = {D: synthetic_problem(N, D, M, seed=D) for D in sorted({c[1] for c in CASES})}
        _cycle(problems)                                   # warm-up
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        bounds = None
        for _ in range(K):
            bounds = _cycle(problems)
        torch.cuda.synchronize()
        free_after = torch.cuda.mem_get_info()[0]
        q.put((rank, free_before, free_after, bounds))
    finally:
        dist.destroy_process_group()


def test_a_context_gives_back_what_it_took_and_can_be_used_again():
    (_, free_before, free_after, bounds), = _spawn(_worker, 1, (), 1, timeout=1200)
    drop = free_before - free_after
    print(f"free device memory before {free_before} after {free_after}: drop {drop} bytes over {K} cycles (bound {BOUND})")
    for name, (used, fresh) in bounds.items():
        print(f"{name}: used {used!r} fresh {fresh!r} rel {abs(used - fresh) / abs(fresh):.3e}")
    assert drop <= BOUND, (free_before, free_after)
    for name, (used, fresh) in bounds.items():
        assert np.isfinite(fresh) and abs(used - fresh) <= 1e-12 * abs(fresh), (name, used, fresh)
