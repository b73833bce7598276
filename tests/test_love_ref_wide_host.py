"""The tolerance of the variance-cache comparison on wide inputs (tests/test_gpu_itergp_wide.py), measured on the host.

The library's kernel values on wide inputs are good to a relative 1e-11 (the figure tests/test_gpu_wide.py holds wide products to).  This
test moves every kernel value of the numpy restatement (tests/love_ref.py: `wobble`, `seed`) by that much, over three seeds, on the very
cases, ranks and new points of the GPU test, and records the largest change of the cached variance in units of the kernel variance.  The
GPU tolerance is 10x the largest of them and never below 1e-10: wide_cases.cache_tolerance().  The measurements are asserted against
the recorded ceiling wide_cases.CACHE_MEASURED_MAX, so that a change of the cases that moves them is seen here and not on the GPU."""
import functools

import numpy as np
import pytest

import love_ref as lref
import matern52_ref as m52
import wide_cases as wc

@functools.lru_cache(maxsize=None)
def restatement(kind, N, D, r, wobble=0.0, seed=0):
    X, y, h, Xnew = wc.itergp_case(N, D)
    with m52.oracle_with_matern52():
        v, c = lref.predict_var(kind, X, y, h["lengthscales"], h["variance"], h["noise"], h["mean"], Xnew, r, wobble=wobble, seed=seed)
    v.setflags(write=False)
    return v, c.J


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("case", wc.CACHE_CASES, ids=lambda c: "N%d_D%d" % c)
def test_wobble_of_the_restatement(case, kind):
    N, D = case
    X, _y, h, _Xnew = wc.itergp_case(N, D)
    wc.check_informative(kind, X, h)
    worst = 0.0
    for r in wc.CACHE_RANKS:
        base, J = restatement(kind, N, D, r)
        assert J == r                                # no early stop at these ranks: rank_out of the GPU run is r exactly
        changes = []
        for seed in wc.WOBBLE_SEEDS:
            moved, Jm = restatement(kind, N, D, r, wc.WOBBLE, seed)
            assert Jm == J
            changes.append(np.abs(moved - base).max() / h["variance"])
        print(f"N={N} D={D} {kind} r={r}: largest change under a {wc.WOBBLE:.0e} wobble " + " ".join(f"{c:.2e}" for c in changes))
        worst = max(worst, max(changes))
    assert worst <= wc.CACHE_MEASURED_MAX
    # the cached variance is a Galerkin bound: never below the exact one, not increasing with the rank
    with m52.oracle_with_matern52():
        exact = lref.exact_var(kind, X, _y, h["lengthscales"], h["variance"], h["noise"], h["mean"], _Xnew)
    prev = None
    for r in wc.CACHE_RANKS:
        v = restatement(kind, N, D, r)[0]
        assert np.all(v >= exact - 1e-9 * h["variance"])
        assert prev is None or np.all(v <= prev + 1e-12 * h["variance"])
        prev = v
