"""What the GPU tests of the pathwise samples rest on, checked on the CPU (tests/sample_ref.py):

* the random features of `draw_features` reproduce each kernel to Hoeffding's bound, and `draw_features` is the stated transformation of
  its raw draws;
* the float64 restatement of the device cosine (the reduction and coefficients of cglb_amd/csrc/devmath.h, read from that file) is inside the
  absolute error bound the header states, against mpmath at 50 digits on 1e5 phases; the header's bound is the measured maximum read at
  the upper end of its last digit.  Measured: 2.2e-16 (the restatement rounds twice per Horner step where the device's fused form rounds
  once);
* the mean over draws of the dense restatement is the predictive mean of tests/gpr_ref.py (an identity of the estimator, for any omega);
  the ratio of the empirical to the exact variance is printed, not asserted: its bias depends on F;
* every planted defect moves a compared quantity of the GPU tests' cases by at least 10 tolerances on every case it applies to.
"""
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest
import torch

import gpr_ref
import sample_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the feature approximation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", sr.KINDS)
def test_features_reproduce_the_kernel_to_hoeffdings_bound(kind, D):
    from cglb_amd.backend.models import draw_features
    F, n = 65536, 40
    omega, b = draw_features(kind, D, F, torch.Generator(device="cpu").manual_seed(1234))
    omega, b = omega.numpy(), b.numpy()
    x = 1.2 * np.random.default_rng(D).standard_normal((n, D))
    cosv = np.cos(x @ omega.T + b[None, :])                      # unit lengthscales, unit variance, no centre
    approx = (2.0 / F) * (cosv @ cosv.T)
    exact = sr.kernel(kind, x, x, np.ones(D), 1.0)
    pairs = n * (n + 1) // 2
    t = math.sqrt(8.0 * math.log(2.0 * pairs / 1e-6) / F)        # terms 2 cos cos in [-2, 2]; total failure probability 1e-6 over the pairs
    err = np.abs(approx - exact)[np.triu_indices(n)].max()
    print(f"{kind} D={D}: largest deviation over {pairs} pairs {err:.4f}, Hoeffding t = {t:.4f}")
    assert err <= t


@pytest.mark.parametrize("kind", sr.KINDS)
def test_draw_features_is_the_stated_transformation(kind):
    from cglb_amd.backend.models import draw_features, feature_draws
    d, F = 3, 50
    omega, b = draw_features(kind, d, F, torch.Generator(device="cpu").manual_seed(7))
    z, chi2, u = feature_draws(kind, d, F, torch.Generator(device="cpu").manual_seed(7))
    assert (chi2 is None) == (kind == "rbf")
    want_omega, want_b = sr.features_from_draws(kind, z.numpy(), None if chi2 is None else chi2.numpy(), u.numpy())
    np.testing.assert_allclose(omega.numpy(), want_omega, rtol=4e-16, atol=0)
    np.testing.assert_allclose(b.numpy(), want_b, rtol=4e-16, atol=0)
    assert omega.shape == (F, d) and b.shape == (F,) and 0.0 <= float(b.min()) and float(b.max()) < 2 * math.pi
    if chi2 is not None:
        assert float(chi2.min()) > 0.0


# ---- the cosine ----------------------------------------------------------------------------------------------------------------------
def _devmath_cos():
    text = open(os.path.join(ROOT, "cglb_amd", "csrc", "devmath.h")).read()
    body = text[text.index("double cos_turns(double phi)"):]
    body = body[:body.index("\n}\n")]
    hexes = [float.fromhex(h) for h in re.findall(r"-?0x1\.[0-9a-f]+p[+-]\d+", body)]
    bound = float(re.search(r"#define CGLB_COS_TURNS_ERR (\S+)", text).group(1))
    return hexes, bound


def test_restatement_has_the_devices_coefficients_and_bound():
    hexes, bound = _devmath_cos()
    assert tuple(reversed(hexes)) == sr.COS_COEF[1:]             # Horner order in the header, ascending here; the constant term is 1.0
    assert sr.COS_COEF[0] == 1.0 and bound == sr.COS_TURNS_ERR


def _phases():
    rng = np.random.default_rng(0)
    k = rng.integers(-2 ** 33, 2 ** 33, 10000).astype(np.float64) / 8.0          # exact eighths of a turn up to 2^30 ...
    eighths = np.concatenate([k, np.nextafter(k, np.inf), np.nextafter(k, -np.inf)])   # ... and their neighbours
    small = np.arange(-16, 17) / 8.0
    small = np.concatenate([small, np.nextafter(small, np.inf), np.nextafter(small, -np.inf)])
    out = np.concatenate([eighths, small, rng.uniform(-1, 1, 30000), rng.uniform(-1, 1, 20000) * 2.0 ** rng.integers(0, 31, 20000),
                          rng.uniform(-1, 1, 10000) * 2.0 ** -rng.integers(1, 60, 10000), rng.uniform(0.2, 0.3, 9901)])
    assert out.size >= 100000 and np.abs(out).max() > 2.0 ** 29
    return out


def test_cosine_restatement_is_inside_the_stated_bound():
    mp.mp.dps = 50
    phi = _phases()
    got = sr.cos_turns(phi)
    worst = 0.0
    for p, g in zip(phi.tolist(), got.tolist()):
        worst = max(worst, float(abs(mp.cospi(2 * mp.mpf(p)) - mp.mpf(g))))
    digit = 10.0 ** math.floor(math.log10(worst))
    print(f"cos_turns: largest absolute error over {phi.size} phases {worst:.3e}; stated bound {sr.COS_TURNS_ERR:.0e}")
    assert worst <= sr.COS_TURNS_ERR
    assert sr.COS_TURNS_ERR <= (math.floor(worst / digit) + 1) * digit * (1 + 1e-12)   # the measured maximum at the upper end of its last digit
    assert sr.cos_turns(np.array([0.0, 1.0, -3.0, 2.0 ** 40]))[:].tolist() == [1.0, 1.0, 1.0, 1.0]   # whole turns: exactly 1


# ---- the estimator's mean ------------------------------------------------------------------------------------------------------------
def test_sample_mean_is_the_predictive_mean():
    N, D, F, S, kind = 60, 3, 64, 4096, "matern32"
    X, y = gpr_ref.problem(N, D)
    h = sr.sample_hypers(D)
    rng = np.random.default_rng(11)
    xnew = np.concatenate([X[:3], 1.5 * rng.standard_normal((9, D))])
    omega, b = sr.features_from_draws(kind, rng.standard_normal((F, D)), rng.chisquare(3, F), rng.uniform(0, 1, F))   # fixed
    f, _ = sr.sample(kind, X, y, h, xnew, omega, b, rng.standard_normal((S, F)), rng.standard_normal((S, N)))
    dense = gpr_ref.evaluate(kind, X, y, with_grad=False, **h)
    mean, var = gpr_ref.predict(kind, X, dense, h["lengthscales"], h["variance"], h["mean"], xnew)
    emp_mean, emp_var = f.mean(axis=0), f.var(axis=0, ddof=1)
    z = np.abs(emp_mean - mean) / np.sqrt(emp_var / S)
    print(f"sample mean: largest deviation {z.max():.2f} standard errors; empirical / exact variance at F = {F}: "
          f"{np.array2string(emp_var[3:] / var[3:], precision=2)} (new points), {np.array2string(emp_var[:3] / var[:3], precision=2)} (training rows)")
    assert np.all(z <= 6.0)


# ---- planted defects -----------------------------------------------------------------------------------------------------------------
def _applies(defect, cell, x, c, ls, omega, b, W):
    _id, d, n, F, S, mode, _training = cell
    if not np.any(W):
        return False
    if defect == "sin_quarter":
        t = np.asarray(sr.phases(x, c, ls, omega, b) / (2 * np.arccos(np.longdouble(-1))), dtype=np.float64)
        t = t - np.rint(t)
        return bool(np.any((t >= 0.25 + 1e-9) & (t < 0.5 - 1e-9)))
    if defect == "centre_kept":
        return bool(np.any(omega))
    if defect == "ninth_as_first":
        return S >= 9
    return True


@pytest.mark.parametrize("cell", sr.feature_cells(), ids=lambda c: c[0])
def test_planted_defects_move_the_feature_product(cell):
    X, _y, x, omega, b, W = sr.feature_problem(cell)
    d = cell[1]
    h = sr.feature_hypers(d)
    rows = X if x is None else x
    c, ls, f = sr.centre(X), h["lengthscales"], h["variance"]
    clean = sr.features(rows, c, ls, f, omega, b, W)
    tol = sr.feature_tolerance(rows, c, ls, f, omega, b, W)
    chunk = sr.feature_split(rows.shape[0], len(b), d)[1]
    for defect in sr.FEATURE_DEFECTS:
        if not _applies(defect, cell, rows, c, ls, omega, b, W):
            continue
        moved = np.asarray(np.abs(sr.features(rows, c, ls, f, omega, b, W, defect, chunk) - clean), dtype=np.float64)
        print(f"{cell[0]} {defect}: moved by {(moved / tol).max():.2e} tolerances")
        assert (moved / tol).max() >= 10.0, defect


@pytest.mark.parametrize("case", sr.SAMPLE_CASES, ids=lambda c: "N%d_D%d_%s" % c[:3])
def test_planted_defects_move_the_samples(case):
    N, D, kind, _k = case
    X, y = gpr_ref.problem(N, D)
    h = sr.sample_hypers(D)
    bound = math.sqrt(2.0 * h["variance"] * 1e-12) + 1e-9 * math.sqrt(h["variance"])   # the solve check at max_error = 1e-12
    for S in sr.SAMPLE_S:
        omega, b, W, eps = sr.sample_draws(N, D, kind, S)
        for n_new in sr.SAMPLE_NEW:
            xnew = sr.sample_new_points(X, n_new)
            clean, _ = sr.sample(kind, X, y, h, xnew, omega, b, W, eps)
            for defect in sr.FEATURE_DEFECTS + sr.SAMPLE_DEFECTS:
                if defect == "ninth_as_first" and S < 9:
                    continue
                moved = np.abs(sr.sample(kind, X, y, h, xnew, omega, b, W, eps, defect=defect)[0] - clean).max()
                print(f"{kind} N={N} S={S} n_new={n_new} {defect}: moved by {moved / bound:.2e} bounds")
                assert moved >= 10.0 * bound, defect


def test_case_tables_cover_what_they_claim():
    cells = sr.feature_cells()
    assert len(cells) <= 40 and len({c[0] for c in cells}) == len(cells)
    assert {c[1] for c in cells} == set(sr.DIMS) | {12} and {c[4] for c in cells} >= set(sr.COLS) and {c[5] for c in cells} == set(sr.MODES)
    assert {c[3] for c in cells} >= set(sr.F_SMALL) | set(sr.F_LARGE)
    for d in sr.DIMS:
        assert {c[2] for c in cells if c[1] == d} >= set(sr.row_counts(d))
        assert len({c[3] for c in cells if c[1] == d}) >= 4 and len({c[4] for c in cells if c[1] == d}) >= 4
    # both sides of every chunk-count edge of the launcher's rule that the cells reach: 1 | 2 | 3 chunks, and the slot cap
    assert [sr.feature_split(1, F, 3)[0] for F in (64, 65, 128, 129, 16384, 16385)] == [1, 2, 2, 3, 256, 253]
    assert {sr.rows_per_lane(c[1]) for c in cells} == {1, 2, 4} and sr.pad_dim(40) == 40 and sr.pad_dim(17) == 20
    assert any(c[6] for c in cells)
