"""The launch-geometry design of tests/geometry_cases.py, checked without a GPU:

* the pruned design still covers what it claims (every chunk value, sym_order, kind and precision with every rows-per-lane class);
* every N of a cell is ragged against 16, 64, RBROWS, 4 RBROWS and the chunk, and small enough for the dense oracle;
* the closed form of the pair count agrees with a direct count over the work list of `ensure_sym_items`;
* the cases discriminate: with the lengthscales and p of the cells, a kernel that loses ONE median-magnitude pair, or the last column
  of one chunk, moves the result by more than 10x the bound the GPU tests assert (fp64: 2e-12 max|ref|; fp32: TAU s)."""
import numpy as np
import pytest

import fp32_error_model as em
import geometry_cases as gc


def test_design_covers_every_axis_value_with_every_class():
    cells = gc.cells()
    assert len(cells) == len(gc.CLASSES) * len(gc.CHUNKS) == 63
    assert sorted({em.rows_per_lane(D, dt) for dt, D, _ in gc.CLASSES if dt == "fp64"}) == [1, 2, 4, 8]
    assert sorted({em.rows_per_lane(D, dt) for dt, D, _ in gc.CLASSES if dt == "fp32"}) == [2, 4, 8]
    for dtype, D, _ in gc.CLASSES:
        mine = [c for c in cells if c[1] == dtype and c[2] == D]
        assert [c[4] for c in mine] == list(gc.CHUNKS)
        assert {c[5] for c in mine} == {0, 1} and {c[6] for c in mine} == set(em.KINDS) and {c[7] for c in mine} == {0, 1}
    assert [gc.eff_chunk(o) for o in gc.CHUNKS] == [16, 128, 256, 512, 1008, 1024, 1024]


def test_sizes_are_ragged_and_reach_the_large_n_geometry():
    for _, dtype, D, _, opt, _, _, _ in gc.cells():
        rb, ch = gc.rbrows(dtype, D), gc.eff_chunk(opt)
        ns = gc.sizes(dtype, D, opt)
        assert len(ns) == (3 if 4 * rb < ch else 2) and max(ns) <= 3200
        for n in ns:
            assert all(n % m for m in (16, 64, rb, 4 * rb, ch)), (dtype, D, opt, n)
        assert ns[0] > ch and (ns[1] + ch - 1) // ch >= 3           # a second chunk; three chunks
        if len(ns) == 3:  # several groups of four row blocks start inside one chunk
            assert (ns[2] + 4 * rb - 1) // (4 * rb) > (ns[2] + ch - 1) // ch


def _count_pairs(n, rb, chunk, world, rank):
    """The work list of ensure_sym_items, item by item."""
    nrb = (n + rb - 1) // rb
    total = 0
    for b in range(rank, nrb, world):
        rbase = b * rb
        rows = min(rb, n - rbase)
        for k in range(rbase // chunk, (n + chunk - 1) // chunk):
            j0, j1 = max(k * chunk, rbase), min((k + 1) * chunk, n)
            total += rows * max(j1 - j0, 0)
    return total


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_pair_count_closed_form_equals_the_work_list(world):
    for n, rb, chunk in [(17, 512, 16), (1041, 256, 1024), (2321, 256, 1024), (2999, 64, 128), (1500, 512, 1024), (3077, 128, 1008), (129, 64, 16)]:
        per_rank = [gc.pairs_closed_form(n, rb, world, r) for r in range(world)]
        assert per_rank == [_count_pairs(n, rb, chunk, world, r) for r in range(world)]
        assert sum(per_rank) == gc.pairs_closed_form(n, rb)
    assert gc.pairs_closed_form(1000, 256) == 256 * 1000 + 256 * 744 + 256 * 488 + 232 * 232


DISCRIMINATION = [(dtype, D, kind, opt, which) for dtype, D, _ in gc.CLASSES for kind in em.KINDS for opt, which in ((16, 0), (1024, -1))]


@pytest.mark.parametrize("dtype,D,kind,opt,which", DISCRIMINATION, ids=[f"{a}-D{b}-{c}-c{d}" for a, b, c, d, _ in DISCRIMINATION])
def test_one_lost_pair_or_chunk_edge_column_clears_ten_times_the_bound(dtype, D, kind, opt, which):
    """The smallest N of the chunk-16 cell and the largest N of the chunk-1024 cell of every class, both kinds."""
    N, chunk = gc.sizes(dtype, D, opt)[which], gc.eff_chunk(opt)
    X, _, hyp, p = gc.problem(N, D)
    case = gc.reference_case(kind, dtype, X, hyp, p, chunk, need_K=True)
    limit = 10.0 * gc.bound(dtype)
    # one pair of median magnitude (over the off-diagonal terms k_ij p_j)
    terms = np.abs(case.K * p[None, :])
    np.fill_diagonal(terms, np.nan)
    med = np.nanmedian(terms)
    i, j = np.unravel_index(np.nanargmin(np.abs(terms - med)), terms.shape)
    r_pair = em.ratio(em.defect_drop_pair(case, p, i, j), case.ref, case.s)
    assert r_pair > limit, f"a lost median pair ({terms[i, j]:.3g}) moves row {i} by {r_pair:.3g} of s, 10x the bound is {limit}"
    # the last column of the first chunk (of the only column short of N if the chunk is wider)
    col = min(chunk, N) - 1
    r_col = em.ratio(em.defect_drop_last_column(case, p, col=col), case.ref, case.s)
    assert r_col > limit, f"losing column {col} moves the result by {r_col:.3g} of s, 10x the bound is {limit}"
