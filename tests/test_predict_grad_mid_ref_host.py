"""Host checks of tests/predict_grad_mid_ref.py (no GPU): the cell table of the mid-width row-weighted product and its covering claim, the mirror of
the launch geometry, the float64 restatement of the kernel's arithmetic against the longdouble reference at the tolerance the GPU test uses, the
planted defects of that restatement (each misses the tolerance tenfold on every cell it applies to), wide_cases.informative on every reference, and
the two forms of the predictor references against each other."""
import numpy as np
import pytest

import input_grad_mid_ref as igm
import input_grad_ref as ig
import predict_grad_mid_ref as pgm
import predict_grad_ref as pg
import slab_rules
import wide_cases as wc

CELLS = pgm.product_cells()
#: the cells of the restatement: all but the one beyond a launch (its rows are those of the others, 64 times over)
HOST_CELLS = [c for c in CELLS if c["n_new"] <= 65]


# ---- the table and its covering claim ---------------------------------------------------------------------------------------------------------------
def test_every_value_of_every_axis_occurs():
    assert {c["D"] for c in CELLS} >= {33, 48, 49, 64, 65, 80, 81, 96}
    for d in pgm.DIMS:
        B = pgm.rows_per_block(d)
        assert B == 64 and {c["n_new"] for c in CELLS if c["D"] == d} == {1, 2, B - 1, B, B + 1}
    assert sum(c["n_new"] == 4097 for c in CELLS) == 1
    assert {c["n_pts"] for c in CELLS} == {1, 65, 300} and {c["set"] for c in CELLS} == {"train", "inducing"}
    assert {c["jsplit"] for c in CELLS} == {1, 3, 7} and {c["kind"] for c in CELLS} == set(wc.KINDS) and {c["precision"] for c in CELLS} == {0, 1}
    assert all(c["ldw_extra"] > 0 for c in CELLS)
    assert sorted(CELLS[x]["kind"] for x in pgm.PRECISION_CELLS) == sorted(wc.KINDS)
    assert len({pgm.cell_id(c) for c in CELLS}) == len(CELLS) == 41


def test_every_hot_width_meets_every_value():
    for dh in (48, 64, 80, 96):
        cells = [c for c in CELLS if pgm.hot_width(c["D"]) == dh]
        assert {c["D"] for c in cells if c["n_new"] <= 65} == {d for d in pgm.DIMS if pgm.hot_width(d) == dh} and len(cells) >= 10
        assert {c["weights"] for c in cells} == set(pgm.WEIGHTS)
        assert {c["n_pts"] for c in cells} == {1, 65, 300} and {c["set"] for c in cells} == {"train", "inducing"}
        assert {c["jsplit"] for c in cells} == {1, 3, 7} and {c["kind"] for c in cells} == set(wc.KINDS) and {c["precision"] for c in cells} == {0, 1}
        # several chunks occur at every width: the forced split takes effect where the set has more than 64 points
        assert max(pgm.weighted_split(c["n_new"], c["n_pts"], c["D"], c["jsplit"])[0] for c in cells) >= 3
    # every defect meets every width
    for defect in pgm.MID_DEFECTS:
        assert {pgm.hot_width(c["D"]) for c in HOST_CELLS if pgm.defect_applies(defect, c)} == {48, 64, 80, 96}, defect


# ---- the launch geometry ---------------------------------------------------------------------------------------------------------------------------
def test_geometry_mirror():
    """csrc/row_slab.h: predict_grad_mid_split = input_grad_mid_split = 4 at every hot width; csrc/kernels_predict_grad_mid.hip: rows per workgroup
    256 / SPLIT, the kff_jsplit rule with even chunks and the two-weight cap"""
    for d in pgm.DIMS + (40, 77, 90):
        dh = pgm.hot_width(d)
        assert pgm.split(d) == igm.split(d) == 4 and pgm.rows_per_block(d) == 64 and pgm.part_width(d) * 4 == dh and pgm.part_width(d) % pgm.slice_width(d) == 0
        assert 2 * pgm.part_width(d) < d        # "drop_part": part 1 holds real coordinates only
    # forced split: capped by the number of 64-point chunks; even chunk lengths; the chunk count the length gives
    assert pgm.weighted_split(65, 300, 77, 3) == (3, 100) and pgm.weighted_split(65, 300, 77, 7) == (5, 60) and pgm.weighted_split(1, 65, 33, 7) == (2, 34)
    assert pgm.weighted_split(64, 1, 96, 3) == (1, 2)
    # automatic: ceil(8192 / row blocks) = 128 chunks, within the 64-point rule (16 at 1024 points) and the slab's cap (21 at Dh = 96 and 4096 rows)
    assert pgm.weighted_split(4096, 1024, 77)[0] == 16 and pgm.weighted_split(4096, 50000, 90)[0] == 21 and pgm.weighted_split(64, 50000, 90)[0] == 256
    # the cap is that of the two-weight slab whichever weights are given: 2^24 doubles over n_rows * 2 (Dh + 1)
    cap = slab_rules.slot_cap(4096, 2 * 97)
    assert cap == (1 << 24) // (4096 * 2 * 97) == 21 and pgm.weighted_split(4096, 50000, 96, 200)[0] <= cap


# ---- the restatement against the longdouble reference ------------------------------------------------------------------------------------------------
def _cell_reference(c, precision=None):
    X, y, Z, h, xnew, u, Wt = pgm.cell_problem(c)
    P = X if c["set"] == "train" else Z
    uu, ww = pgm.weights_of(c, u, Wt)
    ls, f = h["lengthscales"], h["variance"]
    want = pg.weighted_product(c["kind"], xnew, P, ls, f, uu, ww)
    tol = pgm.level_tolerance(c["kind"], xnew, P, ls, f, uu, ww, c["precision"] if precision is None else precision)
    return X, P, h, xnew, uu, ww, want, tol


@pytest.mark.parametrize("c", HOST_CELLS, ids=pgm.cell_id)
def test_restatement_and_its_defects(c):
    X, P, h, xnew, uu, ww, want, tol = _cell_reference(c)
    ls, f = h["lengthscales"], h["variance"]
    if len(P) > 1:
        wc.check_informative(c["kind"], P, h)       # a reference that is numerically the identity passes any gradient test
    cen = X.mean(axis=0)
    got = pgm.restated_weighted(c["kind"], xnew, P, cen, ls, f, uu, ww, c["jsplit"])
    for g, w in zip(got, want):
        assert (g is None) == (w is None) and (g is None or g.shape == w.shape)
    clean = pgm.miss(got, want, tol)
    assert clean <= 1.0, clean                        # inside the tolerance on every element
    if c["n_new"] > 1:                                # the point at 10^3: within the clamp floor
        for g, t in zip(got, tol):
            assert g is None or np.all(np.abs(g[1]) <= t[1])
    for defect in pgm.MID_DEFECTS:
        if pgm.defect_applies(defect, c):
            bad = pgm.miss(pgm.restated_weighted(c["kind"], xnew, P, cen, ls, f, uu, ww, c["jsplit"], defect=defect), want, tol)
            assert bad >= 10.0, (defect, bad)


def test_wscale_and_the_level_term():
    """the caller's factor of the Wt gradient multiplies the constant; the level term widens the tolerance at precision level 2 alone, by the level's
    kernel error over the 1e-11 of the product rule, and never the floor"""
    c = CELLS[6]
    X, P, h, xnew, _u, _w, _want, _tol = _cell_reference(c)
    _X, _y, _Z, _h, _xn, u, Wt = pgm.cell_problem(c)
    ls, f = h["lengthscales"], h["variance"]
    a = pgm.restated_weighted(c["kind"], xnew, P, X.mean(axis=0), ls, f, u, Wt, c["jsplit"])
    b = pgm.restated_weighted(c["kind"], xnew, P, X.mean(axis=0), ls, f, u, Wt, c["jsplit"], wscale=-2.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(-2.0 * a[3], b[3])
    t1 = pgm.level_tolerance(c["kind"], xnew, P, ls, f, u, Wt, 1)
    t2 = pgm.level_tolerance(c["kind"], xnew, P, ls, f, u, Wt, 2)
    base = pg.weighted_tolerance(c["kind"], xnew, P, ls, f, u, Wt)
    for x in range(4):
        assert np.array_equal(t1[x], base[x]) and np.all(t2[x] >= base[x])
        assert float((t2[x] / base[x]).max()) <= 1.0 + igm.LEVEL2_KERNEL_ERROR / ig.TOL + 1e-9
    far = 1                                            # the point at 10^3: the floor alone, at every level
    assert np.array_equal(t2[0][far], base[0][far]) and np.array_equal(t2[3][far], base[3][far])


# ---- the predictor references ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pgm.SHAPES, ids=lambda s: "N%d_D%d_M%d" % s)
@pytest.mark.parametrize("kind", wc.KINDS)
def test_predictor_references(shape, kind):
    """on the problems of the GPU test: informative kernel matrices; the analytic form (the library's algebra) and fp64 autograd through the textbook
    form agree within the tolerance the library is held to, quad_term 0 and 1, and so do the two forms of the exact class"""
    case = pgm.Case(*shape, 65, kind)
    X, y, hyp, v = pgm.problem(case)
    wc.informative(wc.dense(kind, X, hyp), hyp)
    xn = pgm.xnew(case)
    assert np.array_equal(xn[0], X[0]) and np.array_equal(xn[5], hyp.Z[0]) and np.all(xn[-1] == pgm.FAR)
    for q in (0, 1):
        ref, ana = pgm.cglb_reference(case, q), pgm.cglb_analytic(case, q)
        tol = pg.predictor_tolerance(kind, hyp, ref)
        assert pg.grad_miss(ana, ref, tol) <= 1.0
        assert float(np.abs(ana.mean - ref.mean).max()) <= tol["mean"] and float(np.abs(ana.var - ref.var).max()) <= tol["var"]
        assert float(np.abs(ref.g_mean[:-1]).max()) > 0 and float(np.abs(ref.g_var[:-1]).max()) > 0
    gcase = pgm.Case(shape[0], shape[1], 0, 65, kind)
    Xg, yg, hg, _ = pgm.problem(gcase)
    ref = pgm.gpr_reference(gcase)
    ana = pg.gpr_predict_grad_analytic(kind, Xg, yg, hg, pgm.xnew(gcase))
    assert pg.grad_miss(ana, ref, pg.predictor_tolerance(kind, hg, ref)) <= 1.0
