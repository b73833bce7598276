"""Launch geometry of the symmetric K_ff mat-vec (kernels_kff_sym.hip) against the fp64 direct-difference oracle.

The column chunk (128 ... 1024), the item order, the rows-per-lane class R and the world size select the work list, the slab layout and the
LDS staging of a launch; without forcing, everything but chunk 128 is reached only at N >= 46 000.  Here the option `sym_chunk` forces
every chunk value at N <= ~3100.  The design - one (dtype, D) per R class, every chunk value with every class, sym_order / kind /
precision rotated over the cells so that each of their values meets every class, two or three ragged N per cell - is written down and
pruned in tests/geometry_cases.py; tests/test_geometry_cases_host.py shows on the CPU that a kernel losing one median pair or one
chunk-edge column would fail these assertions by more than 10x.

Bounds: fp64 |out - ref| <= 2e-12 max|ref| (as tests/test_gpu_kff_variants.py); fp32 the round-off model of tests/fp32_error_model.py
with the accumulation depth n_acc of the forced chunk, ratio <= TAU['matvec']."""
import math

import numpy as np
import pytest
import torch

import fp32_error_model as em
import geometry_cases as gc
from oracle import cglb_oracle_c as orcc

pytestmark = pytest.mark.gpu

_ctx, _reference, _check, _matvec_dot, _cyclic = gc.make_ctx, gc.reference, gc.check, gc.matvec_dot, gc.matvec_cyclic

CELLS = gc.cells()


@pytest.mark.parametrize("name,dtype,D,extra,opt,order,kind,prec", CELLS, ids=[c[0] for c in CELLS])
def test_forced_chunk_matvec_matches_the_oracle(name, dtype, D, extra, opt, order, kind, prec):
    chunk, rb = gc.eff_chunk(opt), gc.rbrows(dtype, D)
    for N in gc.sizes(dtype, D, opt):
        X, _, hyp, p = gc.problem(N, D)
        ctx = _ctx(kind, dtype, X, hyp, dict(extra, sym_chunk=opt, sym_order=order, precision=prec))
        out = ctx.matvec(torch.from_numpy(p)).double().cpu().numpy()
        ref, s, bound = _reference(kind, dtype, X, hyp, p, chunk)
        _check(out, ref, s, bound, f"{name} N={N}")
        assert ctx.get_stat("k1_pairs_per_launch") == gc.pairs_closed_form(N, rb), (name, N)
        out2, dot = _matvec_dot(ctx, p)
        assert np.array_equal(out2, out), f"{name} N={N}: a second call differs"
        pf = p.astype(np.float32).astype(np.float64) if dtype == "fp32" else p
        assert dot == pytest.approx(math.fsum(pf * out2), rel=1e-12), (name, N)
        ctx.close()


def test_sym_chunk_beyond_the_rounding_range_is_refused():
    """The launcher rounds a forced chunk up to a multiple of 16 before clamping it: a value next to INT64_MAX would wrap negative."""
    X, _, hyp, p = gc.problem(300, 8)
    ctx = _ctx("rbf", "fp64", X, hyp, {})
    for bad in (2 ** 63 - 1, 2 ** 63 - 8, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="sym_chunk"):
            ctx.set_option("sym_chunk", bad)
    ctx.set_option("sym_chunk", 2 ** 20)   # clamps to 1024
    ref = orcc.kff_matvec("rbf", X, hyp, p)
    np.testing.assert_allclose(ctx.matvec(torch.from_numpy(p)).cpu().numpy(), ref, rtol=0, atol=gc.ATOL64 * np.abs(ref).max())
    ctx.close()


# (dtype, D, extra options, N, world, forced chunk, sym_order, kind); D = 3: 512-row blocks, so N = 1500 / 2200 gives 3 / 5 row blocks and
# ranks 3 ... 7 / 5 ... 7 of world 8 launch nothing
CYCLIC = [("fp64", 8, {}, 2999, 2, 128, 1, "rbf"), ("fp64", 8, {}, 2999, 3, 512, 0, "matern32"), ("fp64", 3, {}, 1500, 8, 1024, 1, "rbf"),
          ("fp64", 20, {}, 2100, 8, 512, 0, "rbf"), ("fp64", 16, {}, 2500, 3, 1024, 1, "matern32"), ("fp64", 12, {}, 2300, 2, 1024, 0, "rbf"),
          ("fp64", 50, {"wide_reg": 1}, 1100, 3, 128, 1, "rbf"), ("fp64", 50, {"wide_reg": 1}, 2100, 2, 1024, 0, "matern32"),
          ("fp32", 16, {}, 2999, 2, 1024, 1, "rbf"), ("fp32", 3, {}, 2200, 8, 128, 0, "matern32"), ("fp32", 24, {}, 1700, 3, 512, 1, "rbf"),
          ("fp32", 3, {}, 2999, 3, 1024, 1, "rbf"), ("fp64", 3, {}, 2999, 2, 512, 0, "matern32"), ("fp64", 20, {}, 1301, 3, 128, 1, "matern32")]


@pytest.mark.parametrize("dtype,D,extra,N,world,opt,order,kind", CYCLIC, ids=[f"{c[0]}-D{c[1]}-N{c[3]}-w{c[4]}-c{c[5]}-o{c[6]}-{c[7]}" for c in CYCLIC])
def test_forced_chunk_cyclic_partials_sum_to_the_oracle(dtype, D, extra, N, world, opt, order, kind):
    """The per-rank partials of the cyclic split (all ranks emulated on one context) add up to the oracle's (K_ff + noise I) p and the
    per-rank pair counts to the closed form; a world larger than the number of row blocks leaves ranks with an empty grid."""
    rb = gc.rbrows(dtype, D)
    X, _, hyp, p = gc.problem(N, D, seed=world)
    ctx = _ctx(kind, dtype, X, hyp, dict(extra, sym_chunk=opt, sym_order=order))
    p_dev = ctx._dev(p, N)
    total, pairs = np.zeros(N), 0
    for rank in range(world):
        part = _cyclic(ctx, p_dev, world, rank)
        got = ctx.get_stat("k1_pairs_per_launch")
        assert got == gc.pairs_closed_form(N, rb, world, rank), (rank, got)
        if rank >= (N + rb - 1) // rb:
            assert got == 0 and not part.any(), f"rank {rank} owns no row block: its partial must be zero"
        assert np.array_equal(_cyclic(ctx, p_dev, world, rank), part)
        total += part
        pairs += got
    assert pairs == gc.pairs_closed_form(N, rb)
    ref, s, bound = _reference(kind, dtype, X, hyp, p, gc.eff_chunk(opt))
    _check(total, ref, s, bound, f"cyclic {dtype} D={D} N={N} world={world} chunk={opt}")
    ctx.close()


SHARDS = em.SHARDS + ((1600, 1601),)
SHARD_CASES = [(dtype, D, kind, r0, r1, (128, 512, 1024, 16)[(i + q) % 4], (1, 7, 512)[(i + q) % 3])
               for i, (dtype, D, kind) in enumerate((("fp64", 8, "rbf"), ("fp64", 20, "matern32"), ("fp32", 16, "rbf"), ("fp64", 3, "matern32")))
               for q, (r0, r1) in enumerate(SHARDS)]


@pytest.mark.parametrize("dtype,D,kind,r0,r1,opt,jsplit", SHARD_CASES, ids=[f"{c[0]}-D{c[1]}-{c[2]}-{c[3]}-{c[4]}-c{c[5]}-j{c[6]}" for c in SHARD_CASES])
def test_row_shards_with_forced_chunk_and_column_split(dtype, D, kind, r0, r1, opt, jsplit):
    """A row shard of N = 2999: the symmetric kernel on the shard's own square, the plain kernel on the column ranges left and right of
    it with a forced kff_jsplit: 1 slot, 7, and 512, which kff_pairs_range clamps to ncols / 64 - 24 slots at most per side here, ONE
    for the 37-column left range of the shard (37, 2999).  The 2 x 512 slots that plain_slots_max reserves are never all written at a
    size with a dense reference; what is checked is the offset of the row- and column-sum slabs behind a varying number of plain slots."""
    N = 2999
    X, _, hyp, p = gc.problem(N, D, seed=7)
    ctx = _ctx(kind, dtype, X, hyp, dict(sym_chunk=opt, kff_jsplit=jsplit), row_range=(r0, r1))
    out = ctx.matvec(torch.from_numpy(p)).double().cpu().numpy()
    ref, s, bound = _reference(kind, dtype, X, hyp, p, gc.eff_chunk(opt), r0, r1)
    _check(out, ref, s, bound, f"shard {dtype} D={D} [{r0},{r1}) chunk={opt} jsplit={jsplit}")
    assert ctx.get_stat("k1_pairs_per_launch") == gc.pairs_closed_form(r1 - r0, gc.rbrows(dtype, D))
    out2, dot = _matvec_dot(ctx, p)
    assert np.array_equal(out2, out)
    pf = p.astype(np.float32).astype(np.float64) if dtype == "fp32" else p
    assert dot == pytest.approx(math.fsum(pf[r0:r1] * out2), rel=1e-12)
    ctx.close()


@pytest.mark.parametrize("dtype,D,kind", [("fp64", 8, "rbf"), ("fp32", 16, "matern32"), ("fp64", 20, "rbf")])
def test_one_context_through_a_shuffled_sequence_of_geometries(dtype, D, kind):
    """Chunk, order and world/rank change from one mat-vec to the next on ONE context: the cache key of the work list
    (ensure_sym_items) and the reallocation of the list and of the partial-sum slabs; every mat-vec is checked."""
    from cglb_amd import _lib
    N, rb = 2333, gc.rbrows(dtype, D)
    X, _, hyp, p = gc.problem(N, D, seed=3)
    ctx = _ctx(kind, dtype, X, hyp, {})
    p_dev = ctx._dev(p, N)
    seq = [(c, o, w) for c in (16, 128, 512, 1000, 1024, 0) for o in (0, 1) for w in (1, 2, 8)]
    np.random.default_rng(5).shuffle(seq)
    refs = {}
    for step, (opt, order, world) in enumerate(seq):
        ctx.set_option("sym_chunk", opt)
        ctx.set_option("sym_order", order)
        chunk = gc.eff_chunk(opt) if opt else em.sym_chunk(N, D, world, dtype=dtype)
        if chunk not in refs:
            refs[chunk] = _reference(kind, dtype, X, hyp, p, chunk)
        ref, s, bound = refs[chunk]
        if world == 1:
            _lib.check(ctx.lib.cglb_set_parallel(ctx._ctx, 1, 0), ctx._ctx)
            out = ctx.matvec(p_dev).double().cpu().numpy()
            assert ctx.get_stat("k1_pairs_per_launch") == gc.pairs_closed_form(N, rb)
        else:
            out, pairs = np.zeros(N), 0
            for rank in np.random.default_rng(step).permutation(world):
                out += _cyclic(ctx, p_dev, world, int(rank))
                pairs += ctx.get_stat("k1_pairs_per_launch")
            assert pairs == gc.pairs_closed_form(N, rb)
        _check(out, ref, s, bound, f"step {step}: chunk {opt} order {order} world {world}")
    ctx.close()
