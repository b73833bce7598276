"""The helper tests/input_grad_mid_ref.py on the host: the cell table, the reference against central differences, the float64 restatement of the
mid-width kernel's arithmetic and its planted defects against the tolerance tests/test_gpu_input_grad_mid.py holds the library to, and the
measurement behind the g_var tolerance.  Runs on any CPU.

1. The table reaches every (Dh, SPLIT, G) class and every axis value; the precision cells are one per kind.
2. On every cell the longdouble gradient of the reference equals central differences of its longdouble value (steps 2^-20 l_k, the first four new
   points of the cell: a training row, the point at 10^3, two random ones) to 1e-10 of the largest entry, and wide_cases.informative holds for the
   cell's kernel matrix (N > 1).
3. The float64 restatements of the two kernels' arithmetic stay inside input_grad_ref.cross_tolerance / feature_tolerance on every element of
   every cell; every planted defect (input_grad_ref's and the mid-width ones) misses them by >= 10x on every cell it applies to.
4. g_var = -2 sum B G at love_ref's cache under wide_cases.WOBBLE over WOBBLE_SEEDS: the largest change stays below the recorded ceiling.
"""
import numpy as np
import pytest

import input_grad_mid_ref as igm
import input_grad_ref as ig
import wide_cases as wc

LD = np.longdouble
STEP = 2.0 ** -20
CELLS = igm.product_cells()


def test_the_table_reaches_every_class_and_axis_value():
    seen = lambda key: {c[key] for c in CELLS}
    assert seen("D") == set(igm.DIMS) and seen("N") == set(igm.N_VALUES) and seen("jsplit") == set(igm.JSPLITS) and seen("F") == set(igm.F_VALUES)
    assert seen("kind") == set(igm.KINDS)
    for d in igm.DIMS:
        mine = [c for c in CELLS if c["D"] == d]
        assert {c["n_new"] for c in mine} == set(igm.row_counts(d)) and {c["S"] for c in mine} == set(igm.s_values(d))
        cls = (igm.hot_width(d), igm.split(d), igm.group_width(d))
        assert cls in igm.CLASSES and d in igm.CLASSES[cls]
        assert igm.rows_per_block(d) == 64 and igm.part_width(d) % igm.slice_width(d) == 0
    assert {(igm.hot_width(d), igm.split(d), igm.group_width(d)) for d in igm.DIMS} == set(igm.CLASSES)
    assert {igm.hot_width(d) for d in igm.DIMS if igm.hot_width(d) > d} == {igm.hot_width(d) for d in igm.DIMS if igm.hot_width(d) == d} == {48, 64, 80, 96}
    assert any(igm.cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[0] > 1 for c in CELLS)                       # several chunks ...
    assert any(c["N"] % igm.cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[1] for c in CELLS if c["N"] > 1)   # ... and a short last one
    assert {CELLS[i]["kind"] for i in igm.PRECISION_CELLS} == set(igm.KINDS) and all(CELLS[i]["N"] > 1 for i in igm.PRECISION_CELLS)
    assert len(CELLS) == 40
    for defect in igm.MID_DEFECTS:
        assert sum(igm.defect_applies(defect, c) for c in CELLS) >= 5, defect
        assert sum(igm.feature_defect_applies(defect, c) for c in CELLS) >= 5, defect
    for c in CELLS:   # the feature rule at 64 rows per block gives the chunk count input_grad_ref.feature_tolerance counts with
        assert igm.feature_split(c["n_new"], c["F"], c["D"]) == ig.feature_split(c["n_new"], c["F"], c["D"])


def _central_value(kind, x, X, ls, f, V):
    """[n, S, d] central differences of the reference value in longdouble, step 2^-20 l_k in coordinate k"""
    x = np.asarray(x, dtype=LD)
    Vl = np.asarray(V, dtype=LD)
    cols = []
    for k in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, k] += LD(STEP) * LD(ls[k])
        xm[:, k] -= LD(STEP) * LD(ls[k])
        vp, vm = (LD(f) * (ig.cross_terms(kind, xx, X, ls)[0] @ Vl) for xx in (xp, xm))
        cols.append((vp - vm) / (xp[:, k] - xm[:, k])[:, None])
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("c", CELLS, ids=igm.cell_id)
def test_reference_restatement_and_defects(c):
    X, _y, h, xnew, V, omega, b, W = igm.cell_problem(c)
    ls, f, kind = h["lengthscales"], h["variance"], c["kind"]
    if c["N"] > 1:
        wc.check_informative(kind, X, h)
    want_o, want_g = igm.cross_grad(kind, xnew, X, ls, f, V)
    # the reference against central differences of its own value
    few = xnew[:4]
    fd = _central_value(kind, few, X, ls, f, V)
    scale = np.abs(want_g[:len(few)]).max()
    err = float(np.abs(fd - want_g[:len(few)]).max() / scale) if scale > 0 else float(np.abs(fd).max())
    assert err <= 1e-10, err
    # the float64 restatement of the kernel's arithmetic, every element
    tv, tg = igm.cross_tolerance(kind, xnew, X, ls, f, V)
    out, g = igm.restated_cross_grad(kind, xnew, X, ls, f, V, c["jsplit"])
    eo, eg = float((np.abs(out - want_o) / tv).max()), float((np.abs(g - want_g) / tg).max())
    print(f"{igm.cell_id(c)}: central differences {err:.2e}; restatement value {eo:.2e}, gradient {eg:.2e} of the tolerance")
    assert eo <= 1.0 and eg <= 1.0
    if c["N"] == 1:
        assert np.all(g[0] == 0.0)
    # the defects of input_grad_ref that a cell of this table can show, and the mid-width ones
    chunk, group = igm.cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[1], igm.group_width(c["D"])
    live = c["N"] > 1 or c["n_new"] > 2
    for defect in ig.CROSS_DEFECTS:
        applies = {"coincident_nonzero": True, "m32_for_m52": live and kind == "matern52", "transposed": live and c["S"] > 1,
                   "drop_group_last": live and c["S"] % group != 0}.get(defect, live)
        if applies:
            bad = igm.cross_grad(kind, xnew, X, ls, f, V, defect=defect, chunk=chunk, group=group)[1]
            miss = float((np.abs(bad - want_g) / tg).max())
            assert miss >= 10.0, (defect, miss)
    for defect in igm.MID_DEFECTS:
        if igm.defect_applies(defect, c):
            bad = igm.restated_cross_grad(kind, xnew, X, ls, f, V, c["jsplit"], defect=defect)[1]
            miss = float((np.abs(bad - want_g) / tg).max())
            assert miss >= 10.0, (defect, miss)


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("case", wc.CACHE_CASES, ids=lambda c: "N%d_D%d" % c)
def test_wobble_of_the_variance_gradient(case, kind):
    N, D = case
    X, _y, h, _Xnew = wc.itergp_case(N, D)
    wc.check_informative(kind, X, h)
    unit = h["variance"] * np.sqrt(ig.C_KIND[kind]) / np.asarray(h["lengthscales"], dtype=np.float64)
    worst = 0.0
    for r in igm.PREDICT_RANKS:
        base, R = igm.gvar_restatement(kind, N, D, r)
        assert R.shape[1] == (r + 7) // 8 * 8
        changes = [float((np.abs(igm.gvar_restatement(kind, N, D, r, wc.WOBBLE, seed)[0] - base) / unit).max()) for seed in wc.WOBBLE_SEEDS]
        print(f"N={N} D={D} {kind} r={r}: largest change of g_var under a {wc.WOBBLE:.0e} wobble, units of f sqrt(C) / l_k: " + " ".join(f"{c:.2e}" for c in changes))
        worst = max(worst, max(changes))
    assert worst <= igm.GVAR_MEASURED_MAX
    # the factor the reference's own planted defect loses
    base = igm.gvar_restatement(kind, N, D, 8)[0]
    assert float((np.abs(0.5 * base) / igm.gvar_tolerance(kind, h["lengthscales"], h["variance"])).max()) >= 10.0


def _central_feature(x, cen, ls, f, omega, b, W):
    x = np.asarray(x, dtype=LD)
    cols = []
    for k in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, k] += LD(STEP) * LD(ls[k])
        xm[:, k] -= LD(STEP) * LD(ls[k])
        cols.append((igm.feature_grad(xp, cen, ls, f, omega, b, W)[0] - igm.feature_grad(xm, cen, ls, f, omega, b, W)[0]) / (xp[:, k] - xm[:, k])[:, None])
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("c", CELLS, ids=igm.cell_id)
def test_feature_reference_restatement_and_defects(c):
    import sample_ref as sr
    X, _y, h, xnew, _V, omega, b, W = igm.cell_problem(c)
    ls, f = h["lengthscales"], h["variance"]
    cen = sr.centre(X)
    want_o, want_g = igm.feature_grad(xnew, cen, ls, f, omega, b, W)
    few = xnew[2:5] if len(xnew) > 2 else xnew[:1]      # not the point at 10^3: its phases of ~1e3 radians leave central differences ~1e-10 themselves
    fd = _central_feature(few, cen, ls, f, omega, b, W)
    wg = igm.feature_grad(few, cen, ls, f, omega, b, W)[1]
    err = float(np.abs(fd - wg).max() / np.abs(wg).max())
    assert err <= 1e-10, err
    tv, tg = igm.feature_tolerance(xnew, cen, ls, f, omega, b, W)
    out, g = igm.restated_feature_grad(xnew, cen, ls, f, omega, b, W)
    eo, eg = float((np.abs(out - want_o) / tv).max()), float((np.abs(g - want_g) / tg).max())
    print(f"{igm.cell_id(c)}: feature central differences {err:.2e}; restatement value {eo:.2e}, gradient {eg:.2e} of the tolerance")
    assert eo <= 1.0 and eg <= 1.0
    chunk, group = igm.feature_split(c["n_new"], c["F"], c["D"])[1], igm.group_width(c["D"])
    turns = (sr.phases(xnew, cen, ls, omega, b) / (2 * np.arccos(LD(-1)))).astype(np.float64)
    turns -= np.rint(turns)
    quarter = bool(((turns >= 0.26) & (turns < 0.49)).any())
    for defect in ig.FEATURE_DEFECTS:
        applies = {"transposed": c["S"] > 1, "drop_group_last": c["S"] % group != 0, "sin_quarter": quarter}.get(defect, True)
        if applies:
            bad = igm.feature_grad(xnew, cen, ls, f, omega, b, W, defect=defect, chunk=chunk, group=group)[1]
            miss = float((np.abs(bad - want_g) / tg).max())
            assert miss >= 10.0, (defect, miss)
    for defect in igm.MID_DEFECTS:
        if igm.feature_defect_applies(defect, c):
            bad = igm.restated_feature_grad(xnew, cen, ls, f, omega, b, W, defect=defect)[1]
            miss = float((np.abs(bad - want_g) / tg).max())
            assert miss >= 10.0, (defect, miss)
