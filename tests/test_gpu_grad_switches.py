"""The switches of the gradient algebra against the oracle's analytic gradient: grad_trsm (0 products with the explicit L^-1, 1 triangular
solves, 2 products + one refinement step) x grad_gram (the two forms of the symmetric N^2 pass) on a well- and an ill-conditioned K_uu,
and wide_grad_sym (upper tiles only / every tile of the tiled K_ff gradient pass of wide inputs), on the full square and on row shards."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import cglb_oracle as orc
from tools.fuzz_parity import check_case, named_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("grad_gram", [0, 1])
@pytest.mark.parametrize("grad_trsm", [0, 1, 2])
@pytest.mark.parametrize("kind", ["rbf", "matern32"])
def test_gradient_switches_on_a_well_conditioned_problem(kind, grad_trsm, grad_gram):
    """N = 1200, D = 3, M = 16, l = 1 (the problem of test_gram_form_gradient_pass_against_direct_differences_and_oracle): all six
    combinations meet the tolerances of tests/test_gpu_edge_cases.py - lengthscales rtol 2e-8 + 1e-9 of the largest entry, Z rtol 1e-7 +
    1e-9, noise 1e-8 relative, the bound 1e-11."""
    from cglb_amd.hip_context import HipContext
    N, D, M = 1200, 3, 16
    rng = np.random.default_rng(17)
    X = rng.uniform(-3.0, 3.0, size=(N, D))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    Z = X[:M].copy()
    hyp = orc.Hypers(np.full(D, 1.0), 1.3, 0.2, 0.1, Z, 1e-6)
    v = rng.standard_normal(N) * 0.1
    ref = orc.objective(kind, X, y, hyp, v, run_cg=False, with_grad=True)
    ctx = HipContext(X, y, M, kind)
    ctx.set_option("grad_trsm", grad_trsm)
    ctx.set_option("grad_gram", grad_gram)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
    res = ctx.objective_and_grad(torch.from_numpy(v).to(ctx.device), False)
    assert res.bound == pytest.approx(ref.bound, rel=1e-11)
    np.testing.assert_allclose(res.grad["lengthscales"], ref.grad["lengthscales"], rtol=2e-8, atol=1e-9 * np.abs(ref.grad["lengthscales"]).max())
    np.testing.assert_allclose(res.grad["Z"], ref.grad["Z"], rtol=1e-7, atol=1e-9)
    assert res.grad["noise"] == pytest.approx(ref.grad["noise"], rel=1e-8, abs=1e-10)
    assert res.grad["variance"] == pytest.approx(ref.grad["variance"], rel=1e-8, abs=1e-10 * abs(ref.bound))
    ctx.close()


@pytest.mark.parametrize("grad_gram", [0, 1])
@pytest.mark.parametrize("grad_trsm", [1, 2])
def test_stable_gradient_algebra_on_the_ill_conditioned_named_draw(grad_trsm, grad_gram):
    """Sweep seed 2024, draw 186 (N = 561, D = 1, M = 533, RBF, cond(K_uu) = 3e8): the triangular solves (1) and the refined products (2)
    stay within the parity policy - 10x the oracle's own gradient spread under eps-level moves of Z (orc.grad_roundoff_spread,
    tools/fuzz_parity.py: check_case)."""
    c = named_case(2024, 186)
    assert (c["N"], c["D"], c["M"], c["kind"]) == (561, 1, 533, "rbf")
    ok, line, _ = check_case(c, options={"grad_trsm": grad_trsm, "grad_gram": grad_gram})
    print(line)
    assert ok, line


@pytest.mark.parametrize("grad_gram", [0, 1])
def test_explicit_inverse_gradient_algebra_stays_finite_on_the_ill_conditioned_named_draw(grad_gram):
    """grad_trsm 0 multiplies by the explicit L^-1, which loses cond(L) eps: on this draw it is only required to be finite.  Measured on
    an MI355X (largest deviation from the oracle's gradient / its largest entry): Z 1.6e-4 (8.8e-10 absolute, 37x the oracle's own floor
    of 2.4e-11, so outside the 10x policy), lengthscales 1.5e-13 / 2.9e-13 (grad_gram 0 / 1); modes 1 and 2 give 1.1e-5 ... 2.1e-5 on Z."""
    c = named_case(2024, 186)
    ok, line, d = check_case(c, options={"grad_trsm": 0, "grad_gram": grad_gram})
    print("grad_trsm 0:", line, {k: f"{e:.3g}" for k, e in d["gerr"].items()})
    g = d["res"].grad
    assert all(np.isfinite(np.asarray(g[k])).all() for k in ("lengthscales", "Z", "variance", "noise", "mean"))
    assert d["e_b2"] < 1e-9 and d["e_mv"] < 1e-11, line   # the bound and the operator do not go through L^-1


def _wide_problem(N, D, M, seed):
    X, y, Z = orc.synthetic_problem(N, D, M, seed=seed)
    rng = np.random.default_rng(seed + 100)
    return X, y, Z, orc.Hypers(rng.uniform(0.8, 1.6, size=D) * np.sqrt(D), 1.3, 0.08, 0.15, Z, 1e-6)


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("D,options,tol", [(100, {}, 1e-7), (50, {"wide_reg": 0}, 1e-9)])
def test_wide_gradient_pass_with_and_without_the_symmetric_tile_list(kind, D, options, tol):
    """wide_grad_sym 1 visits the tiles on and right of the diagonal, 0 every tile: D = 100 (Gram tiles only) and D = 50 with wide_reg 0
    (a mid width sent through the tiles), N = 1867 (ragged against the tiles), at a fixed v against the oracle's gradient with the
    tolerances of tests/test_gpu_wide.py (1e-7 / 1e-9 of max(largest entry, 1e-3 |bound|)); both values on one context, back and forth."""
    from cglb_amd.hip_context import HipContext
    N, M = 1867, 40
    X, y, Z, hyp = _wide_problem(N, D, M, seed=D)
    v = np.random.default_rng(9).standard_normal(N) * 0.1
    ref = orc.objective(kind, X, y, hyp, v, run_cg=False, with_grad=True)
    ctx = HipContext(X, y, M, kind)
    for k, val in options.items():
        ctx.set_option(k, val)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
    got = {}
    for sym in (0, 1, 0, 1):
        ctx.set_option("wide_grad_sym", sym)
        res = ctx.objective_and_grad(torch.from_numpy(v).to(ctx.device), False)
        assert res.bound == pytest.approx(ref.bound, rel=1e-10)
        for key in ("lengthscales", "Z", "variance", "noise", "mean"):
            a, b = np.asarray(res.grad[key]), np.asarray(ref.grad[key])
            np.testing.assert_allclose(a, b, rtol=0, atol=tol * max(np.abs(b).max(), 1e-3 * abs(ref.bound)), err_msg=f"{key} (wide_grad_sym {sym})")
        if sym in got:
            assert np.array_equal(got[sym], res.grad["lengthscales"])
        got[sym] = res.grad["lengthscales"]
    ctx.close()


SHARD_SHAPE = (9000, 100, 40)   # two shards of 4500 rows: two row tiles (4096 + 404) each against three column tiles


def _shard_worker(rank, world, port, sym, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cglb_amd.distributed import Comm, HipLocalOps, ShardedCGLB, row_partition
        from cglb_amd.hip_context import HipContext
        torch.cuda.set_device(0)
        N, D, M = SHARD_SHAPE
        X, y, Z, hyp = _wide_problem(N, D, M, seed=D)
        v = np.random.default_rng(9).standard_normal(N) * 0.1
        _, parts = row_partition(N, world)
        r0, r1 = parts[rank]
        ctx = HipContext(X, y, M, "rbf", row_range=(r0, r1))
        ctx.set_option("wide_grad_sym", sym)
        ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
        drv = ShardedCGLB(HipLocalOps(ctx), Comm())
        drv.v_local.copy_(torch.from_numpy(v[r0:r1]).to(ctx.device))
        res = drv.objective_and_grad(False)
        q.put((rank, res.bound, np.asarray(res.grad)))
        dist.barrier()
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("wide_grad_sym", [0, 1])
def test_wide_gradient_pass_on_row_shards_switches_the_symmetric_tile_list_off(wide_grad_sym):
    """Two contexts that own the rows [0, 4500) and [4500, 9000) of a D = 100 problem (Gram tiles; the host-driven sharded evaluation over
    gloo, both ranks on one GPU).  A shard sees a rectangle of K_ff, not the square: a tile right of the shard's diagonal does not stand
    for a mirror image inside the shard, so the pass has to visit every tile whatever wide_grad_sym says (wide_grad_kff: sym only for
    row0 == 0 and nrows == N; rank 0 has row0 == 0 but not all rows).  With the option at 1 and at 0 the all-reduced gradient matches
    the oracle's at the same v, at the tolerances of test_wide_inputs_on_two_ranks (1e-7 of the largest entry, the bound to 1e-10)."""
    N, D, M = SHARD_SHAPE
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [mpc.Process(target=_shard_worker, args=(r, 2, port, wide_grad_sym, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    X, y, Z, hyp = _wide_problem(N, D, M, seed=D)
    v = np.random.default_rng(9).standard_normal(N) * 0.1
    ref = orc.objective("rbf", X, y, hyp, v, run_cg=False, with_grad=True)
    for rank, bound, grad in out:
        assert bound == pytest.approx(ref.bound, rel=1e-10), rank
        for key, got in (("lengthscales", grad[:D]), ("Z", grad[D + 3:].reshape(M, D))):
            err = np.abs(got - ref.grad[key]).max() / np.abs(ref.grad[key]).max()
            print(f"rank {rank} wide_grad_sym {wide_grad_sym} {key}: {err:.3g} (bound 1e-7)")
            np.testing.assert_allclose(got, ref.grad[key], rtol=0, atol=1e-7 * np.abs(ref.grad[key]).max(), err_msg=f"{key} (rank {rank})")
        assert grad[D + 1] == pytest.approx(ref.grad["noise"], rel=1e-7, abs=1e-7 * abs(ref.bound))
    assert np.array_equal(out[0][2], out[1][2])
