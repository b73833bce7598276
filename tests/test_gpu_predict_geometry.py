"""Every predictive path at the geometry edges of the NEW points: row-block tails and second blocks of the cross mat-vec, its column slabs
at small and odd N, the 32-row chunks of the K_us panel and its padded leading dimension, the second row tile of the wide path, the second
batch of the dense class, a group of one point in the iterative class, and fewer new points than ranks.  The table, the references, the
tolerances and the way the two-valued axes are dealt over the cells: tests/predict_ref.py; that the table can catch an index defect at
these tolerances: tests/test_predict_ref_host.py.

Every output tensor is pre-filled with NaN (the wrappers of predict_ref call the C ABI directly) and must be finite before it is compared:
an entry a kernel never writes cannot pass on a freshly zeroed allocation.  The last new point of every case lies at 1e3 in every
coordinate, where the mean must be mu and the variance f to the same tolerance.  Each check prints its worst error in units of the tolerance."""
import functools

import numpy as np
import pytest
import torch

import predict_ref as pr
from test_gpu_dist_backend import _init, _spawn

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def _nan_v(case):
    return np.full(case.N, np.nan)


# ---- A: cross mat-vec, narrow --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.cases("A"), ids=_ids(pr.cases("A")))
def test_cross_matvec(case):
    refs = pr.references(case)
    ctx = pr.make_ctx(case)
    try:
        out = pr.cross_matvec(ctx, pr.xnew(case), pr.problem(case)[3])
    finally:
        ctx.close()
    pr.check(case, {"cross": out}, refs)


def test_cross_matvec_leaves_the_plain_matvec_bitwise_unchanged():
    """kff_variant 0: launch_cross_matvec switches the context to the range-clamped 2^x for its own launch and has to switch it back."""
    case = pr.Case("A", "fp64", 8, 1100, 1, 65, "rbf", False, 1, options=(("kff_variant", 0),), block=1024)
    p = torch.from_numpy(pr.problem(case)[3])
    ctx = pr.make_ctx(case)
    try:
        first = ctx.matvec(p).cpu().numpy()
        out = pr.cross_matvec(ctx, pr.xnew(case), p)
        second = ctx.matvec(p).cpu().numpy()
    finally:
        ctx.close()
    pr.check(case, {"cross": out}, {"cross": pr.cross_ref(case)})
    assert np.array_equal(first, second)


# ---- B, C: the SGPR-corrected predictor, narrow and wide ---------------------------------------------------------------------------------
def _predict_both_terms(case, with_cross):
    refs = pr.references(case)
    Xn, v = pr.xnew(case), pr.problem(case)[3]
    outs = {}
    ctx = pr.make_ctx(case)
    try:
        if with_cross:
            outs["cross"] = pr.cross_matvec(ctx, Xn, v)
        ctx.setup()
        outs["mean0"], outs["var0"] = pr.predict(ctx, v, Xn)
        ctx.set_option("logdet_bound", 1)
        ctx.set_option("quad_term", 1)
        ctx.setup()
        outs["mean1"], outs["var1"] = pr.predict(ctx, _nan_v(case), Xn)      # that branch must not read v
    finally:
        ctx.close()
    pr.check(case, outs, refs)


@pytest.mark.parametrize("case", pr.cases("B"), ids=_ids(pr.cases("B")))
def test_predict(case):
    _predict_both_terms(case, with_cross=False)


@pytest.mark.parametrize("case", pr.cases("C"), ids=_ids(pr.cases("C")))
def test_wide_cross_matvec_and_predict(case):
    _predict_both_terms(case, with_cross=True)


@functools.lru_cache(maxsize=None)
def _multi_problem():
    case, = pr.cases("Bmulti")
    X, y, hyp, v = pr.problem(case)
    rng = np.random.default_rng(11)
    Y = np.stack([y, -y, pr.em.f32(0.5 * y + rng.standard_normal(case.N))], axis=1)
    V = np.stack([v, pr.em.f32(rng.standard_normal(case.N)), np.zeros(case.N)], axis=1)
    refs = [pr.cglb_predict(case.kind, X, Y[:, b], hyp, V[:, b], pr.xnew(case)) for b in range(3)]
    return case, Y, V, refs


def test_predict_multi():
    case, Y, V, want = _multi_problem()
    ctx = pr.make_ctx(case)
    try:
        ctx.set_targets(Y)
        ctx.setup()
        mean, var = pr.predict_multi(ctx, V, pr.xnew(case))
    finally:
        ctx.close()
    assert mean.shape == (3, case.n_new) and var.shape == (case.n_new,)
    for b, (m, s2) in enumerate(want):
        refs = {"mean0": pr.Ref(m, np.full(m.shape, 1e-8 * np.abs(m).max()), 1.0), "var0": pr.Ref(s2, np.full(m.shape, 1e-8 * np.abs(s2).max()), 1.0)}
        pr.check(case, {"mean0": mean[b], "var0": var}, refs, what=f"column {b} ")


# ---- D: the dense exact class ----------------------------------------------------------------------------------------------------------
def _gpr_ctx(case):
    ctx = pr.make_ctx(case)
    try:
        hyp = pr.problem(case)[2]
        ctx.gpr_set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean)
    except BaseException:
        ctx.close()
        raise
    return ctx


@pytest.mark.parametrize("case", pr.cases("D"), ids=_ids(pr.cases("D")))
def test_gpr_predict(case):
    refs = pr.references(case)
    ctx = _gpr_ctx(case)
    try:
        mean, var = pr.gpr_predict(ctx, pr.xnew(case))
    finally:
        ctx.close()
    pr.check(case, {"mean": mean, "var": var}, refs)


def test_gpr_predict_reuses_its_buffers_across_batch_sizes():
    """4097 -> 5 -> 8193 -> 4097 new points on one context with no evaluation in between: the batch buffers are re-used with a changing
    bmax; every result against the reference and the last bitwise equal to the first."""
    by_n = {c.n_new: c for c in pr.cases("D") if c.D == 8}
    base = by_n[4097]
    seq = [base, pr.Case("D", "fp64", 8, base.N, 0, 5, base.kind, base.trained, 1, block=pr.GPR_BATCH),
           pr.Case("D", "fp64", 8, base.N, 0, 8193, base.kind, base.trained, 1, block=pr.GPR_BATCH), base]
    ctx = _gpr_ctx(base)
    try:
        outs = [pr.gpr_predict(ctx, pr.xnew(c)) for c in seq]
    finally:
        ctx.close()
    for c, (mean, var) in zip(seq, outs):
        pr.check(c, {"mean": mean, "var": var}, pr.references(c))
    assert np.array_equal(outs[0][0], outs[3][0]) and np.array_equal(outs[0][1], outs[3][1])


# ---- E: the iterative exact class ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.cases("E"), ids=_ids(pr.cases("E")))
def test_itergp_predict(case):
    """Reference and bound of tests/test_gpu_itergp.py::test_predictive_matches_the_dense_one: sqrt(variance 2e-12) + 1e-9 at max_error 1e-12."""
    refs = pr.references(case)
    ctx = pr.make_ctx(case)
    try:
        mean, var = pr.itergp_predict(ctx, pr.xnew(case), max_error=1e-12)
    finally:
        ctx.close()
    pr.check(case, {"mean": mean, "var": var}, refs)


# ---- F: three ranks sharing the GPU, collectives over gloo ----------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    dist = _init(rank, world, port, "gloo")
    try:
        from cglb_amd.dist_context import DistHipContext
        from cglb_amd.distributed import Comm, HipSymLocalOps, PyDistContext, row_partition
        from cglb_amd.hip_context import HipContext
        results = {}
        for case in pr.cases("F"):
            X, y, hyp, v = pr.problem(case)
            Xn = pr.xnew(case)
            ctx = DistHipContext(X, y, case.M, case.kind, collectives="callbacks")
            try:
                ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
                ctx.setup()
                lib = pr.dist_predict(ctx, v, Xn)
            finally:
                ctx.close()
            # the host-driven twin: same kernels, collectives issued from Python
            _, parts = row_partition(case.N, world)
            twin = PyDistContext(HipSymLocalOps(HipContext(X, y, case.M, case.kind, row_range=parts[rank])), Comm())
            try:
                twin.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
                twin.setup()
                tm, tv = twin.predict(torch.from_numpy(v), Xn)
                host = (tm.cpu().numpy(), tv.cpu().numpy())
            finally:
                twin.close()
            results[case.id] = (lib, host)
        q.put((rank, results))
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _three_ranks():
    """One launch of three processes serves every case of the group, the library's loop and the host-driven twin alike."""
    return _spawn(_rank_worker, 3, (), 3)


@pytest.mark.parametrize("which", [0, 1], ids=["library", "host_driven"])
@pytest.mark.parametrize("case", pr.cases("F"), ids=_ids(pr.cases("F")))
def test_fewer_new_points_than_ranks(case, which):
    refs = pr.references(case)
    for rank, results in _three_ranks():
        mean, var = results[case.id][which]
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)), rank
        pr.check(case, {"mean0": mean, "var0": var}, refs, what=f"rank {rank} ")
