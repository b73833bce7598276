"""Problems of the tests of wide inputs (33 - 96 dimensions and beyond) behind the multi-column K_ff product and the iterative exact-GP
class (test helper, not a test module): tests/test_gpu_multi_mid.py, tests/test_gpu_itergp_wide.py, tests/test_love_ref_wide_host.py.

Standard-normal inputs, lengthscales U(0.8, 1.6) sqrt(D) as in tests/test_gpu_wide.py, so that off-diagonal kernel values are of order
0.1: `informative` asserts that on every host reference (a reference that is numerically the identity tests nothing).  `ell_factor` 0.12,
the value of tests/test_gpu_wide.py, shortens the lengthscales until set_hypers selects the range-clamped kernel instances; at those
lengthscales the off-diagonal values vanish by construction, so those references cannot pass `informative` - `outlier_problem` is the
clamped case that can: one far row widens the exponent range and every other kernel value stays where it was."""
import functools

import numpy as np

from oracle import cglb_oracle as orc

import matern52_ref as m52

KINDS = ("rbf", "matern32", "matern52")
VARIANCE, NOISE, MEAN = 1.3, 0.08, 0.15
#: (N, D) and ranks of the variance-cache comparison against tests/love_ref.py; the wobble of the host measurement behind its tolerance
CACHE_CASES = [(300, 40), (300, 77)]
CACHE_RANKS = [1, 8, 9, 33]
WOBBLE, WOBBLE_SEEDS = 1e-11, (1, 2, 3)   # 1e-11: the figure tests/test_gpu_wide.py holds wide products to

#: tests/test_love_ref_wide_host.py: the largest measured change of the restatement under WOBBLE, rounded up (units of the kernel variance).  Per rank 1 / 8 / 9 / 33, largest of the three seeds:
#:   (300, 40)  rbf 2.1e-12 4.0e-12 2.7e-12 1.4e-11 | matern32 1.6e-12 3.1e-12 2.0e-12 1.2e-11 | matern52 1.8e-12 3.4e-12 2.2e-12 1.4e-11
#:   (300, 77)  rbf 3.6e-12 2.6e-12 3.8e-12 1.3e-11 | matern32 2.7e-12 2.9e-12 3.7e-12 2.59e-11 | matern52 3.0e-12 2.6e-12 3.3e-12 1.7e-11
CACHE_MEASURED_MAX = 2.6e-11


def cache_tolerance():
    """Tolerance of the GPU comparison against the restatement, in units of the kernel variance."""
    return max(10.0 * CACHE_MEASURED_MAX, 1e-10)


def problem(N, D, M, seed, ell_factor=1.0):
    X, y, Z = orc.synthetic_problem(N, D, M, seed=seed)
    rng = np.random.default_rng(seed + 100)
    ls = rng.uniform(0.8, 1.6, size=D) * np.sqrt(D) * ell_factor
    return X, y, Z, orc.Hypers(ls, VARIANCE, NOISE, MEAN, Z, 1e-6)


def outlier_problem(N, D, M, seed, shift=30.0):
    """`problem` with the last row moved by `shift` in every coordinate: the RBF exponent range 2 sum_d (range_d / l_d)^2 log2(e) grows to
    about 2 shift^2 / 1.44 octaves (1250 at 30, beyond the 950 the unclamped 2^x takes) whatever D is, and the far row's kernel values against
    all others vanish."""
    X, y, Z, hyp = problem(N, D, M, seed)
    X = X.copy()
    X[-1] += shift
    return X, y, Z, hyp


def dense(kind, X, hyp):
    with m52.oracle_with_matern52():
        return orc.dense_cov(kind, X, hyp)


def informative(cov, hyp):
    """The median off-diagonal value of K / variance is at least 0.01."""
    N = len(cov)
    off = cov[~np.eye(N, dtype=bool)] / hyp.variance
    med = float(np.median(off))
    assert med >= 0.01, f"median off-diagonal kernel value {med:.3g}: the reference is numerically the identity"
    return med


@functools.lru_cache(maxsize=None)
def matmat_case(kind, N, D, ell_factor=1.0, outlier=False):
    """(X, hyp, V [N, 9], cov @ V), computed once per case and never modified."""
    X, _y, _Z, hyp = outlier_problem(N, D, 8, seed=D) if outlier else problem(N, D, 8, seed=D, ell_factor=ell_factor)
    V = np.random.default_rng(N + D).standard_normal((N, 9))
    cov = dense(kind, X, hyp)
    if ell_factor == 1.0:
        informative(cov, hyp)
    ref = cov @ V
    for a in (X, V, ref):
        a.setflags(write=False)
    return X, hyp, V, ref


def itergp_case(N, D):
    """(X, y, hypers as the keyword arguments of gpr_ref / love_ref, new points): 19 new points, 7 of them training rows."""
    X, y, _Z, hyp = problem(N, D, 8, seed=N + D)
    h = dict(lengthscales=hyp.lengthscales, variance=VARIANCE, noise=NOISE, mean=MEAN)
    Xnew = np.concatenate([X[:7], np.random.default_rng(5).standard_normal((12, D))], axis=0)
    return X, y, h, Xnew


def check_informative(kind, X, h):
    hyp = orc.Hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:1], 1e-6)
    return informative(dense(kind, X, hyp), hyp)
