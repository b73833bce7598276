"""The references of tests/predict_grad_ref.py against each other, against finite differences of the oracle's predictor, and against planted defects
(no GPU).

* The analytic reference (the library's algebra) and the autograd reference (textbook form / dense solve) of each predictor agree within a tenth
  of the GPU tolerance on every cell of the tables.
* Central finite differences of oracle.predict agree loosely with the autograd gradients: the two references do not share a mistake.
* Every planted defect misses the GPU tolerance by >= 10 x on every cell it applies to (predict_grad_ref.defect_applies lists which), and applies
  to at least one cell.
"""
import numpy as np
import pytest

import predict_grad_ref as pg
import predict_ref as pr
from oracle import cglb_oracle as orc

CGLB_CELLS = [(c, q) for c in pg.CGLB_CASES for q in (0, 1)]


def _id(cq):
    return f"{cq[0].id}-q{cq[1]}"


def _close(a: pg.Grad, ref: pg.Grad, tol, fraction):
    for name in ("mean", "var", "g_mean", "g_var"):
        err = np.abs(getattr(a, name) - getattr(ref, name)) / tol[name]
        assert float(err.max()) <= fraction, (name, float(err.max()))


@pytest.mark.parametrize("cq", CGLB_CELLS, ids=_id)
def test_cglb_references_agree(cq):
    case, q = cq
    X, y, hyp, v = pr.problem(case)
    ref = pg.cglb_reference(case, q)
    ana = pg.cglb_predict_grad_analytic(case.kind, X, y, hyp, v, pr.xnew(case), q)
    _close(ana, ref, pg.predictor_tolerance(case.kind, hyp, ref), 0.1)
    if case.n_new >= 2:   # the far point: exact zeros
        assert np.all(ana.g_mean[-1] == 0.0) and np.all(ana.g_var[-1] == 0.0)
        assert np.all(ref.g_mean[-1] == 0.0) and np.all(ref.g_var[-1] == 0.0)


@pytest.mark.parametrize("case", pg.GPR_CASES, ids=lambda c: c.id)
def test_gpr_references_agree(case):
    X, y, hyp, _ = pr.problem(case)
    ref = pg.gpr_reference(case)
    ana = pg.gpr_predict_grad_analytic(case.kind, X, y, hyp, pr.xnew(case))
    _close(ana, ref, pg.predictor_tolerance(case.kind, hyp, ref), 0.1)


def test_textbook_values_are_the_project_references():
    """The value half of the autograd reference is predict_ref's own (sgpr_predict / cglb_predict) on the oracle's kernels."""
    for case in [c for c in pg.CGLB_CASES if c.kind != "matern52"][:6]:
        X, y, hyp, v = pr.problem(case)
        for q in (0, 1):
            r = pr.predict_ref(case, q)
            ref = pg.cglb_reference(case, q)
            assert np.abs(ref.mean - r["mean"].ref).max() <= 0.1 * r["mean"].s.max()
            assert np.abs(ref.var - r["var"].ref).max() <= 0.1 * r["var"].s.max()


@pytest.mark.parametrize("cq", [cq for cq in CGLB_CELLS if cq[0].n_new <= 9 and cq[0].kind != "matern52"], ids=_id)
def test_finite_differences_of_the_oracle(cq):
    case, q = cq
    X, y, hyp, v = pr.problem(case)
    v = np.zeros(case.N) if q else v
    xn = pr.xnew(case)
    ref = pg.cglb_reference(case, q)
    # Matern-3/2 has a kink in the second derivative at a coincident pair: the step error there is O(h), elsewhere O(h^2)
    h = 1e-5
    scale_m = max(np.abs(ref.g_mean).max(), 1.0)
    scale_v = max(np.abs(ref.g_var).max(), 1.0)
    for k in range(case.D):
        e = np.zeros(case.D)
        e[k] = h
        mp, sp, _, _ = orc.predict(case.kind, X, y, hyp, v, xn + e, max_error=1e300)
        mm, sm, _, _ = orc.predict(case.kind, X, y, hyp, v, xn - e, max_error=1e300)
        rows = slice(0, -1) if case.n_new >= 2 else slice(None)   # the far point moves by less than an ulp of 1e3 + h
        assert np.abs((mp - mm)[rows] / (2 * h) - ref.g_mean[rows, k]).max() <= 1e-3 * scale_m
        assert np.abs((sp - sm)[rows] / (2 * h) - ref.g_var[rows, k]).max() <= 1e-3 * scale_v


def test_planted_defects_miss_the_tolerance():
    hit = {d: 0 for d in pg.PREDICT_DEFECTS}
    for case, q in CGLB_CELLS:
        X, y, hyp, v = pr.problem(case)
        ref = pg.cglb_reference(case, q)
        tol = pg.predictor_tolerance(case.kind, hyp, ref)
        for d in pg.PREDICT_DEFECTS:
            if not pg.defect_applies(case, d, q, case.M, hyp.Z):
                continue
            bad = pg.cglb_predict_grad_analytic(case.kind, X, y, hyp, v, pr.xnew(case), q, defect=d)
            miss = pg.grad_miss(bad, ref, tol)
            assert miss >= 10.0, (case.id, q, d, miss)
            hit[d] += 1
    for case in pg.GPR_CASES:
        if case.n_new > 1:     # the larger cells repeat the n_new = 1 cells' algebra at a cost of seconds each
            continue
        X, y, hyp, _ = pr.problem(case)
        ref = pg.gpr_reference(case)
        tol = pg.predictor_tolerance(case.kind, hyp, ref)
        for d in ("sign", "gvar_factor", "lost_rows", "drop_chunk_last", "coincident_nonzero", "swap_uw", "inv_l"):
            bad = pg.gpr_predict_grad_analytic(case.kind, X, y, hyp, pr.xnew(case), defect=d)
            assert pg.grad_miss(bad, ref, tol) >= 10.0, (case.id, d)
    assert all(n > 0 for n in hit.values()), hit


def test_the_cells_reach_every_instance_class():
    assert {pg.rows_per_lane(c["D"]) for c in pg.product_cells()} == set(pg.CLASSES) == {4, 2, 1}
    for c in pg.product_cells():
        assert c["n_new"] in pg.row_counts(c["D"])
    cells = pg.product_cells()
    for key, values in (("n_pts", pg.N_PTS), ("jsplit", pg.JSPLITS), ("kind", pg.ig.KINDS), ("precision", (0, 1)), ("set", ("train", "inducing"))):
        for d in pg.DIMS:
            got = {c[key] for c in cells if c["D"] == d}
            assert len(got) >= 2, (key, d, got)
        assert {c[key] for c in cells} == set(values)
    assert any(c["ldw_extra"] > 0 and c["n_new"] > 1 for c in cells)
