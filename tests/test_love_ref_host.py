"""The numpy restatement of the Lanczos variance cache (tests/love_ref.py) and the host half of the library's build
(cglb_amd/csrc/lanczos_host.h), checked without a GPU.

The restatement is what tests/test_gpu_itergp_var_cache.py holds the device to, so this file checks the restatement itself: against the exact
predictive of tests/gpr_ref.py where the two must agree (J = N), the properties of a Galerkin projection of K^-1, its own sensitivity to
kernel values that are accurate to 1e-13 (the default precision level of the device), and that the mistakes a kernel could make are far
outside the GPU tolerances.  Everything is in units of the kernel variance f.  The restatement is evaluated once per (kind, case, rank) and shared.

The header is plain C++: tests/host/lanczos_check.cpp (own main, no HIP) is compiled against it with the host compiler behind the Makefile's
hipcc, once plainly and once with -fsanitize=address,undefined, as tests/test_slq_host.py does for slq_host.h."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import gpr_ref
import love_ref as lref
import matern52_ref as m52

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cglb_amd", "csrc")
GPU_TOL, GPU_TOL_EXACT = 1e-10, 1e-9       # tests/test_gpu_itergp_var_cache.py: against the restatement; exact limit on the device
#: (kind, (N, D), rank, GPU tolerance) of every comparison the GPU test makes against this restatement or, at J = N, against the exact variance
GPU_CASES = ([(kind, case, r, GPU_TOL) for kind in ("matern32", "matern52") for case in lref.CASES for r in lref.RANKS]
             + [("rbf", (300, 3), 33, GPU_TOL)] + [("matern32", case, case[0], GPU_TOL_EXACT) for case in ((40, 3), (67, 2))])


def _args(kind, case):
    N, D = case
    X, y = gpr_ref.problem(N, D)
    h = lref.hypers(D)
    return (kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], lref.new_points(N, D))


@functools.lru_cache(maxsize=None)
def _cached(kind, case, r):
    with m52.oracle_with_matern52():
        v, c = lref.predict_var(*_args(kind, case), r)
    v.setflags(write=False)
    return v, c


@functools.lru_cache(maxsize=None)
def _exact(kind, case):
    with m52.oracle_with_matern52():
        v = lref.exact_var(*_args(kind, case))
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("case", lref.CASES, ids=lambda c: "N%d_D%d" % c)
def test_exact_limit(case):
    v, c = _cached("matern32", case, case[0])
    err = np.abs(v - _exact("matern32", case)).max()
    print(f"Matern-3/2 {case}: J = {c.J}, largest error {err:.2e} f")
    assert c.J == case[0]
    assert err <= 1e-12


def test_early_stop_of_the_rbf_kernel():
    case = (67, 2)
    v, c = _cached("rbf", case, 67)
    err = np.abs(v - _exact("rbf", case)).max()
    print(f"RBF {case}: J = {c.J}, last beta / alpha_0 = {c.beta[-1] / c.alpha[0]:.2e}, largest error {err:.2e} f")
    assert c.J < 67 and c.beta[-1] <= lref.STOP * c.alpha[0]
    assert err <= 1e-7


@pytest.mark.parametrize("kind", ["rbf", "matern32", "matern52"])
@pytest.mark.parametrize("case", lref.CASES, ids=lambda c: "N%d_D%d" % c)
def test_upper_bound_that_tightens_with_the_rank(case, kind):
    exact, prev = _exact(kind, case), None
    for r in (1, 8, 9, 33, 100):
        v, _ = _cached(kind, case, min(r, case[0]))
        assert np.all(v >= exact - 1e-12)
        if prev is not None:
            assert np.all(v <= prev + 1e-12)
        prev = v


def test_own_sensitivity_on_the_gpu_cases():
    worst = 0.0
    for kind, case, r, _tol in GPU_CASES:
        v, _ = _cached(kind, case, r)
        for seed in (1, 2):
            with m52.oracle_with_matern52():
                w, _ = lref.predict_var(*_args(kind, case), r, wobble=1e-13, seed=seed)
            worst = max(worst, float(np.abs(w - v).max()))
    print(f"a relative 1e-13 wobble of every kernel value moves the variance by at most {worst:.2e} f")
    assert worst <= 1e-11


@pytest.mark.parametrize("defect", ["lost_group", "stale_pad", "lost_rows", "one_pass"])
def test_planted_defects_miss_the_gpu_tolerance_by_two_decades(defect):
    """A lost group of 8 cache columns (the last one), a padded column that holds a stale unit vector instead of zeros, the last two training
    rows lost from every sum (one short column chunk) and one Gram-Schmidt pass instead of two at r = N, where the basis loses its
    orthogonality: the factorisation then meets a pivot that is not positive, which the library reports as CGLB_ERR_NOT_PD."""
    smallest, seen = np.inf, 0
    for kind, case, r, tol in GPU_CASES:
        v, c = _cached(kind, case, r)
        with m52.oracle_with_matern52():
            if defect == "lost_group":
                w, _ = lref.predict_var(*_args(kind, case), r, defect_drop_group=(c.J - 1) // 8)
            elif defect == "stale_pad":
                if c.J % 8 == 0:
                    continue
                w, _ = lref.predict_var(*_args(kind, case), r, defect_stale_pad=1.0 / np.sqrt(case[0]))
            elif defect == "lost_rows":
                w, _ = lref.predict_var(*_args(kind, case), r, defect_drop_rows=2)
            else:
                if r != case[0]:
                    continue
                try:
                    w, _ = lref.predict_var(*_args(kind, case), r, passes=1)
                except ValueError:
                    seen += 1
                    continue
        seen += 1
        ratio = float(np.abs(w - v).max()) / tol
        smallest = min(smallest, ratio)
        assert ratio >= 100.0, (kind, case, r, ratio)
    print(f"{defect}: {seen} cases, the smallest miss is {smallest:.1e} tolerances")
    assert seen >= 2


# ---- the bidiagonal factor header ------------------------------------------------------------------------------------------------------
def _hipcc():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", text, re.M).group(1)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lanczos") / request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "lanczos_check.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr

    def run(commands):
        out = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _fmt(values):
    return " ".join(repr(float(v)) for v in np.asarray(values, dtype=np.float64).reshape(-1))


def test_factor_matches_the_restatement_and_the_tridiagonal(program):
    cases = [_cached("matern32", (40, 3), 40)[1], _cached("rbf", (67, 2), 67)[1], _cached("matern52", (300, 3), 9)[1], _cached("matern32", (40, 3), 1)[1]]
    lines = program([f"factor {c.J} {_fmt(c.alpha)} {_fmt(c.beta[:c.J - 1])}".rstrip() for c in cases])
    for c, line in zip(cases, lines):
        got = np.array([float(x) for x in line.split()])
        d, l = lref.bidiagonal_factor(c.alpha, c.beta)
        assert got[0] == 0 and len(got) == 1 + 2 * c.J
        np.testing.assert_allclose(got[1:1 + c.J], d, rtol=1e-15)
        np.testing.assert_allclose(got[1 + c.J:], l, rtol=1e-15, atol=0.0)
        L = np.diag(got[1:1 + c.J]) + np.diag(got[1 + c.J:-1], -1)
        T = np.diag(c.alpha) + np.diag(c.beta[:c.J - 1], 1) + np.diag(c.beta[:c.J - 1], -1)
        assert np.abs(L @ L.T - T).max() <= 1e-14 * np.abs(T).max()


def test_a_pivot_that_is_not_positive_is_reported(program):
    lines = program(["factor 2 1.0 1.0 2.0", "factor 3 4.0 1.0 nan 1.0 1.0", "factor 1 0.0", "factor 2 4.0 -1.0 1.0", "factor 0"])
    assert [int(line.split()[0]) for line in lines] == [2, 3, 1, 2, 0]   # 1 + the index of the pivot (the NaN is the third); an empty tridiagonal has none


def test_stop_rule(program):
    lines = program(["stop 0 5 1.0 2.0", "stop 4 5 1.0 2.0", "stop 1 5 2e-10 2.0", "stop 1 5 2.1e-10 2.0", "stop 1 5 nan 2.0", "stop 0 1 1.0 1.0"])
    assert lines == ["0", "1", "1", "0", "1", "1"]
