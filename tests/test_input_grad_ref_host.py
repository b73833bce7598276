"""The dense restatement tests/input_grad_ref.py against the existing restatements, the device sine against longdouble, the solve bound of the
gradient, and the planted defects against the tolerances tests/test_gpu_input_grad.py holds the library to.  Runs on any CPU.

1. The analytic gradients equal central differences of the EXISTING restatements (sample_ref.kernel, sample_ref.features,
   love_ref.variance_from_cache), steps 2^-20 l_k, to 1e-10 of the largest entry.  sample_ref.kernel works in float64, whose own round-off
   (~2e-16 f per value) divided by the step is already 1e-10 per pair, so the kernel's check has two halves: the value of the restatement
   equals sample_ref.kernel @ V to float64 round-off, and the gradient equals central differences of that value taken in longdouble.
2. The sine restatement is within its stated bound of longdouble sin on designed phases and on 1e5 random ones.
3. grad_k k_*^T K^-1 grad_k k_* <= C_kind f / l_k^2, and the ratio comes close to 1 at a training point with small noise (the bound is tight).
4. Every planted defect misses the GPU tolerance by >= 10x on every case it applies to; every axis value of the case tables occurs.
"""
import numpy as np
import pytest
import scipy.linalg

import gpr_ref
import input_grad_ref as ig
import love_ref
import sample_ref as sr

LD = np.longdouble
STEP = 2.0 ** -20


def _central(fn, x, ls):
    """[n, ..., d] central differences of fn(x) [n, ...] in longdouble, step 2^-20 l_k in coordinate k"""
    x = np.asarray(x, dtype=LD)
    cols = []
    for k in range(x.shape[1]):
        h = LD(STEP) * LD(ls[k])
        xp, xm = x.copy(), x.copy()
        xp[:, k] += h
        xm[:, k] -= h
        cols.append((fn(xp) - fn(xm)) / (xp[:, k] - xm[:, k]).reshape((-1,) + (1,) * (fn(xp).ndim - 1)))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("kind", ig.KINDS)
def test_cross_gradient_equals_central_differences(kind):
    N, D, S = 120, 3, 4
    X, _y = gpr_ref.problem(N, D)
    h = ig.cell_hypers(D)
    ls, f = h["lengthscales"], h["variance"]
    rng = np.random.default_rng(5)
    xnew, V = rng.standard_normal((7, D)), rng.standard_normal((N, S))
    out, g = ig.cross_grad(kind, xnew, X, ls, f, V)
    existing = sr.kernel(kind, xnew, X, ls, f) @ V
    assert np.abs(out.astype(np.float64) - existing).max() <= 1e-13 * np.abs(existing).max()
    fd = _central(lambda x: ig.cross_grad(kind, x, X, ls, f, V)[0], xnew, ls)
    err = float(np.abs(fd - g).max() / np.abs(g).max())
    # the float64 restatement differenced directly, for the record: its round-off over the step bounds what it can show
    fd64 = _central(lambda x: (sr.kernel(kind, x.astype(np.float64), X, ls, f) @ V).astype(LD), xnew, ls)
    print(f"{kind}: analytic against central differences {err:.2e} of the largest entry (float64 restatement differenced: "
          f"{float(np.abs(fd64 - g).max() / np.abs(g).max()):.2e})")
    assert err <= 1e-10


def test_feature_gradient_equals_central_differences():
    N, D, S, F = 50, 3, 4, 65
    X, _y = gpr_ref.problem(N, D)
    h = ig.cell_hypers(D)
    ls, f = h["lengthscales"], h["variance"]
    c = sr.centre(X)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((7, D))
    omega, b, W = rng.standard_normal((F, D)), rng.uniform(0, 2 * np.pi, F), rng.standard_normal((S, F))
    out, g = ig.feature_grad(x, c, ls, f, omega, b, W)
    assert np.abs(out - sr.features(x, c, ls, f, omega, b, W)).max() <= 1e-17 * np.abs(out).max() + 1e-18
    fd = _central(lambda xx: sr.features(xx, c, ls, f, omega, b, W), x, ls)
    err = float(np.abs(fd - g).max() / np.abs(g).max())
    print(f"feature product: analytic against central differences {err:.2e} of the largest entry")
    assert err <= 1e-10


@pytest.mark.parametrize("kind", ig.KINDS)
def test_variance_gradient_equals_central_differences(kind):
    N, D, r = 120, 3, 8
    X, y = gpr_ref.problem(N, D)
    h = sr.sample_hypers(D)
    ls, f = np.asarray(h["lengthscales"]), h["variance"]
    xnew = np.random.default_rng(7).standard_normal((6, D))
    K = ig.dense_K(kind, X, ls, f, h["noise"])
    R = love_ref.build(K, y - h["mean"], r).R
    mean, gmean, var, gvar = ig.predict_grad(kind, X, y, h, xnew, R=R)
    Ksf = lambda x: LD(f) * ig.cross_terms(kind, x, X, ls)[0]
    assert np.abs(var - love_ref.variance_from_cache(Ksf(xnew), R, f)).max() <= 1e-17
    fd = _central(lambda x: love_ref.variance_from_cache(Ksf(x), R, f), xnew, ls)
    err = float(np.abs(fd - gvar).max() / np.abs(gvar).max())
    alpha = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), y - h["mean"])
    fdm = _central(lambda x: Ksf(x) @ alpha.astype(LD), xnew, ls)
    errm = float(np.abs(fdm - gmean).max() / np.abs(gmean).max())
    print(f"{kind}: variance gradient {err:.2e}, mean gradient {errm:.2e} of the largest entry against central differences")
    assert err <= 1e-10 and errm <= 1e-10


def _designed_phases():
    eighths = np.arange(-16, 17) / 8.0
    out = [eighths]
    for base in eighths:
        x = base
        for _ in range(3):
            x = np.nextafter(x, np.inf)
            out.append(np.array([x]))
        x = base
        for _ in range(3):
            x = np.nextafter(x, -np.inf)
            out.append(np.array([x]))
    big = 2.0 ** np.arange(1, 41)
    for off in (0.0, 0.125, 0.25, 0.375, 0.5, 0.3):
        out += [big + off, -(big + off)]
    out.append(np.array([0.0, -0.0]))
    return np.concatenate(out)


def test_sine_restatement_is_within_its_bound():
    rng = np.random.default_rng(11)
    phases = np.concatenate([_designed_phases(), rng.uniform(-0.5, 0.5, 50000), rng.standard_normal(30000) * 1e3, rng.uniform(-1, 1, 20000) * 2.0 ** 30])
    cv, sv = ig.sincos_turns(phases)
    t = (phases - np.rint(phases)).astype(LD)          # exact in float64
    two_pi = 2 * np.arccos(LD(-1))
    err_s = np.abs(sv.astype(LD) - np.sin(two_pi * t))
    err_c = np.abs(cv.astype(LD) - np.cos(two_pi * t))
    print(f"sine: largest absolute error {float(err_s.max()):.2e} (bound {ig.SIN_TURNS_ERR:.1e}); cosine {float(err_c.max()):.2e}")
    assert np.array_equal(cv, sr.cos_turns(phases))    # the cosine half is the existing restatement, bitwise
    assert float(err_s.max()) <= ig.SIN_TURNS_ERR and float(err_c.max()) <= sr.COS_TURNS_ERR
    assert len(phases) >= 100000


@pytest.mark.parametrize("kind", ig.KINDS)
def test_the_solve_bound_of_the_gradient_holds_and_is_tight(kind):
    N, D = 80, 2
    X, y = gpr_ref.problem(N, D)
    ls, f, noise = np.array([1.1, 0.7]), 1.3, 1e-6
    K = ig.dense_K(kind, X, ls, f, noise)
    xnew = np.concatenate([X[:5], np.random.default_rng(3).standard_normal((5, D))], axis=0)
    _kap, w = ig.cross_terms(kind, xnew, X, ls)
    G = (-f * w).astype(np.float64)                       # [n, N, d]: grad_k k_*
    cho = scipy.linalg.cho_factor(K, lower=True)
    worst = 0.0
    for k in range(D):
        q = np.einsum("ij,ji->i", G[:, :, k], scipy.linalg.cho_solve(cho, G[:, :, k].T))
        ratio = q / (ig.C_KIND[kind] * f / ls[k] ** 2)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0 + 1e-9)
    print(f"{kind}: largest grad_k k_*^T K^-1 grad_k k_* / (C f / l_k^2) = {worst:.3f}")
    if kind == "rbf":          # smooth paths: the derivative at a training point is nearly determined by dense data
        assert worst >= 0.5


CELLS = ig.product_cells()


def test_every_axis_value_of_the_case_tables_occurs():
    seen = lambda key: {c[key] for c in CELLS}
    assert seen("D") == set(ig.DIMS) and seen("N") == set(ig.N_VALUES) and seen("jsplit") == set(ig.JSPLITS) and seen("F") == set(ig.F_VALUES)
    for d in ig.DIMS:
        mine = [c for c in CELLS if c["D"] == d]
        assert {c["n_new"] for c in mine} == set(ig.row_counts(d)) and {c["S"] for c in mine} == set(ig.s_values(d))
        assert (ig.rows_per_lane(d), ig.group_width(d)) in ig.CLASSES and d in ig.CLASSES[(ig.rows_per_lane(d), ig.group_width(d))]
    assert {c["kind"] for c in CELLS if c["D"] == 3} == set(ig.KINDS)
    assert {(ig.rows_per_lane(d), ig.group_width(d)) for d in ig.DIMS} == set(ig.CLASSES)
    assert any(ig.cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[0] > 1 for c in CELLS)           # several chunks ...
    assert any(c["N"] % ig.cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[1] for c in CELLS if c["N"] > 1)   # ... and a short last one
    assert len(CELLS) <= 40


def _applies(defect, c, product, quarter_hit=True):
    """whether a cell can show a defect at all, from the cell's shape alone: the cross product has a pair that is neither coincident nor out
    of range only with a second training row or a third new point (the first two sit on a training row and at 10^3)"""
    S, D, g = c["S"], c["D"], ig.group_width(c["D"])
    live = product == "feature" or c["N"] > 1 or c["n_new"] > 2
    if defect == "coincident_nonzero":
        return True
    if defect == "m32_for_m52":
        return live and c["kind"] == "matern52"
    if defect == "transposed":
        return live and S > 1 and D > 1
    if defect == "drop_group_last":
        return live and S % g != 0
    if defect == "sin_quarter":
        return quarter_hit
    return live


@pytest.mark.parametrize("c", CELLS, ids=ig.cell_id)
def test_every_planted_defect_misses_the_gpu_tolerance(c):
    X, y, xnew, V, omega, b, W = ig.cell_problem(c)
    h = ig.cell_hypers(c["D"])
    ls, f = h["lengthscales"], h["variance"]
    g = ig.group_width(c["D"])
    _tv, tg = ig.cross_tolerance(c["kind"], xnew, X, ls, f, V)
    good = ig.cross_grad(c["kind"], xnew, X, ls, f, V)[1]
    chunk = ig.cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[1]
    for defect in ig.CROSS_DEFECTS:
        if not _applies(defect, c, "cross"):
            continue
        bad = ig.cross_grad(c["kind"], xnew, X, ls, f, V, defect=defect, chunk=chunk, group=g)[1]
        miss = float((np.abs(bad - good) / tg).max())
        assert miss >= 10.0, (defect, miss)
    cen = sr.centre(X)
    _tv, tg = ig.feature_tolerance(xnew, cen, ls, f, omega, b, W)
    good = ig.feature_grad(xnew, cen, ls, f, omega, b, W)[1]
    chunk = ig.feature_split(c["n_new"], c["F"], c["D"])[1]
    turns = (sr.phases(xnew, cen, ls, omega, b) / (2 * np.arccos(LD(-1)))).astype(np.float64)
    turns -= np.rint(turns)
    quarter = bool(((turns >= 0.26) & (turns < 0.49)).any())   # a phase inside the quarter the defect swaps
    for defect in ig.FEATURE_DEFECTS:
        if not _applies(defect, c, "feature", quarter):
            continue
        bad = ig.feature_grad(xnew, cen, ls, f, omega, b, W, defect=defect, chunk=chunk, group=g)[1]
        miss = float((np.abs(bad - good) / tg).max())
        assert miss >= 10.0, (defect, miss)


@pytest.mark.parametrize("case", ig.PREDICT_CASES, ids=lambda c: "N%d_D%d_%s" % c[:3])
def test_the_lost_factor_of_the_variance_gradient_misses_its_tolerance(case):
    N, D, kind, _k = case
    X, y = gpr_ref.problem(N, D)
    h = sr.sample_hypers(D)
    xnew = sr.sample_new_points(X, ig.PREDICT_NEW)
    good = ig.predict_grad(kind, X, y, h, xnew, rank=8)[3]
    bad = ig.predict_grad(kind, X, y, h, xnew, rank=8, defect="gvar_factor")[3]
    tol = ig.gvar_tolerance(kind, h["lengthscales"], h["variance"])
    assert float((np.abs(bad - good) / tol).max()) >= 10.0
