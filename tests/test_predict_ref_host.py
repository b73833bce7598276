"""The design of tests/predict_ref.py, checked without a GPU:

* the two statements of the SGPR predictive - Titsias' textbook form (`sgpr_predict`) and the oracle's tmp1 / tmp2 algebra at v = 0 - agree to
  1e-10 of the largest entry on every case that uses the former (a condition on the chosen inputs);
* the table discriminates: every planted defect (predict_ref.defects), applied to the reference arrays of every case it applies to, misses
  the tolerance the GPU test asserts by at least 100 times;
* the table covers every value of every axis it claims."""
import math

import numpy as np
import pytest

import fp32_error_model as em
import predict_ref as pr

SGPR_CASES = pr.cases("B", "C")


@pytest.mark.parametrize("case", SGPR_CASES, ids=[c.id for c in SGPR_CASES])
def test_the_two_statements_of_the_sgpr_predictive_agree(case):
    X, y, hyp, _ = pr.problem(case)
    Xn = pr.xnew(case)
    m1, v1 = pr.sgpr_predict(case.kind, X, y, hyp, Xn)
    m0, v0 = pr.cglb_predict(case.kind, X, y, hyp, np.zeros(case.N), Xn)
    em_, ev = np.abs(m1 - m0).max() / np.abs(m0).max(), np.abs(v1 - v0).max() / np.abs(v0).max()
    print(f"{case.id}: mean {em_:.2e}, variance {ev:.2e} of the largest entry")
    assert em_ <= 1e-10 and ev <= 1e-10


@pytest.mark.parametrize("case", pr.CASES, ids=[c.id for c in pr.CASES])
def test_every_planted_defect_misses_the_tolerance_a_hundredfold(case):
    refs = pr.references(case)
    assert pr.miss({k: r.ref for k, r in refs.items()}, refs) == 0.0
    smallest, names = math.inf, []
    for name, damaged in pr.defects(case):
        r = pr.miss(damaged, refs)
        names.append(name)
        smallest = min(smallest, r)
        assert r >= 100.0, f"{case.id}: {name} moves the result by {r:.3g} times the tolerance only"
    print(f"{case.id}: smallest planted-defect ratio {smallest:.3g} over {names}")
    # which defects apply follows from the case alone
    n, base = case.n_new, {n_.split("_q")[0] for n_ in names}
    assert "unwritten_edge_row" in base and ("stale_edge_row" in base) == (n >= 2)
    assert ("offset_off_by_one" in base) == (case.group in "CDE" and n > case.block)
    assert ("padded_column" in base) == (case.group in ("B", "Bmulti", "C", "F") and n % 8 != 0)
    assert ("lost_inducing_rows" in base) == (case.group in ("B", "Bmulti", "C", "F"))
    assert ("lost_column_slab" in base) == (case.group in "AC")
    assert ("stale_rank_slice" in base) == (case.group == "F" and n >= 2)


def test_new_points_start_at_the_training_rows_and_end_far_away():
    for case in pr.CASES:
        X, _, hyp, _ = pr.problem(case)
        Xn = pr.xnew(case)
        assert Xn.shape == (case.n_new, case.D) and np.array_equal(Xn, em.f32(Xn))
        k = min(5, case.N, case.n_new - 1 if case.n_new > 1 else 1)
        assert np.array_equal(Xn[:k], X[:k])
        if case.n_new >= 2:
            assert np.all(Xn[-1] == pr.FAR)
            refs = pr.references(case)
            for key, want in pr.far_point(case, refs).items():   # every kernel value underflows there
                assert abs(refs[key].ref[-1] - want) <= 1e-300 + 1e-15 * abs(want), (case.id, key)
        if case.M >= 3 and case.n_new >= 9 and case.N >= 5:
            assert np.array_equal(Xn[5:8], hyp.Z[:3])


def _values(group, attr):
    return {getattr(c, attr) for c in pr.cases(group)}


def test_the_table_covers_every_axis_value():
    # A: every class with every n_new of its own B and every N; both values of the dealt axes with every class; the options
    plain = [c for c in pr.cases("A") if not c.options]
    assert len(plain) == 72
    for dtype, D in pr.A_CLASSES:
        B = 256 * pr.rows_per_thread(D)
        assert B == {3: 1024, 8: 1024, 12: 512, 16: 512}.get(D, 256)
        mine = [c for c in plain if (c.dtype, c.D) == (dtype, D)]
        assert [c.n_new for c in mine] == [1, 2, 63, 65, B - 1, B, B + 1, 2 * B + 17] and all(c.block == B for c in mine)
        assert {c.N for c in mine} == set(pr.A_N) == {1, 65, 129, 1100}
        assert {c.kind for c in mine} == set(em.KINDS) and {c.trained for c in mine} == {False, True} and {c.precision for c in mine} == {0, 1}
    opts = [c for c in pr.cases("A") if c.options]
    assert sorted(c.opt("kff_rows") for c in opts if c.opt("kff_rows")) == [1, 1, 2, 2]
    assert all(c.block == 256 * c.opt("kff_rows") and c.n_new in (c.block, c.block + 1) for c in opts if c.opt("kff_rows"))
    assert sorted(c.opt("kff_jsplit") for c in opts if c.opt("kff_jsplit")) == [1, 3, 7]
    assert [pr.cross_slabs(65, 1100, 2, js)[1] for js in (1, 3, 7)] == [1, 3, 7]
    # the slab rule at the N edges: one column with the chunk rounded past it; odd N with a short last slab; several slabs
    assert pr.cross_slabs(1, 1, 4) == (2, 1)
    for N in (65, 129, 1100):
        jchunk, jsplit = pr.cross_slabs(63, N, 4)
        assert jsplit >= 2 and jchunk % 2 == 0 and 0 < N - (jsplit - 1) * jchunk <= jchunk
        assert N - (jsplit - 1) * jchunk < jchunk
    # B
    assert _values("B", "M") == set(pr.B_M) == {1, 31, 32, 33, 65} and _values("B", "n_new") == set(pr.B_NNEW) == {1, 7, 8, 9, 255, 256, 257}
    assert {(c.dtype, c.D) for c in pr.cases("B")} == set(pr.B_CLASSES) and _values("B", "N") == {130}
    assert len(pr.cases("B")) == 35 and {(c.M, c.n_new) for c in pr.cases("B")} == {(m, n) for m in pr.B_M for n in pr.B_NNEW}
    for attr in ("M", "n_new"):
        for value in _values("B", attr):
            mine = [c for c in pr.cases("B") if getattr(c, attr) == value]
            assert {c.dtype for c in mine} == {"fp64", "fp32"} and {c.kind for c in mine} == set(em.KINDS), (attr, value)
    for attr in ("kind", "trained", "precision"):
        assert len(_values("B", attr)) == 2
    multi, = pr.cases("Bmulti")
    assert (multi.M, multi.n_new) == (33, 9)
    # C
    assert {(c.dtype, c.D, c.options) for c in pr.cases("C")} == set(pr.C_CLASSES)
    assert {(c.dtype, c.D, c.opt("wide_reg", None)) for c in pr.cases("C")} == {("fp64", 40, 0), ("fp64", 40, 1), ("fp64", 100, None), ("fp32", 40, None)}
    for cls in pr.C_CLASSES:
        assert [c.n_new for c in pr.cases("C") if (c.dtype, c.D, c.options) == cls] == [1, 57, 4097]
    assert _values("C", "kind") == set(em.KINDS) and (_values("C", "N"), _values("C", "M")) == ({130}, {33})
    # D
    assert _values("D", "N") == {65, 300} and _values("D", "D") == {1, 8, 20} and _values("D", "kind") == set(em.KINDS)
    for D in pr.D_D:
        assert [c.n_new for c in pr.cases("D") if c.D == D] == [1, 4095, 4096, 4097, 8193]
    for n in pr.D_NNEW:
        assert {c.N for c in pr.cases("D") if c.n_new == n} == {65, 300}
    # E: a group of exactly one new point at n_new = 1, 9, 17
    assert _values("E", "D") == {3, 20} and _values("E", "N") == {257} and _values("E", "trained") == {True}
    for D in pr.E_D:
        assert [c.n_new for c in pr.cases("E") if c.D == D] == [1, 8, 9, 17]
    assert [n % pr.ITERGP_GROUP for n in pr.E_NNEW] == [1, 0, 1, 1]
    # F: fewer new points than ranks, a rank with an empty slice, a short last slice
    assert [c.n_new for c in pr.cases("F")] == [1, 2, 4, 10] and _values("F", "kind") == set(em.KINDS)
    assert {(c.N, c.M, c.D, c.dtype) for c in pr.cases("F")} == {(130, 33, 3, "fp64")}
    assert len({c.id for c in pr.CASES}) == len(pr.CASES)
