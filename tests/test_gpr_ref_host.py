"""The dense restatement of the exact GPR objective (tests/gpr_ref.py) on the CPU: its value against scipy's Gaussian log density, its
gradient against central differences, its own round-off floor at every shape the GPU tests use, and the order bound <= lml."""
import numpy as np
import pytest
import scipy.stats

import gpr_ref as ref
from oracle import cglb_oracle as orc

KINDS = ["rbf", "matern32"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("trained", [False, True])
def test_lml_is_the_gaussian_log_density(kind, trained):
    N, D = 50, 3
    X, y = ref.problem(N, D)
    h = ref.hypers(D, trained)
    K = orc.kernel_matrix(kind, X, X, h["lengthscales"], h["variance"]) + h["noise"] * np.eye(N)
    want = scipy.stats.multivariate_normal.logpdf(y, mean=np.full(N, h["mean"]), cov=K)
    got = ref.evaluate(kind, X, y, **h)
    assert abs(got.lml - want) <= 1e-11 * abs(want), (got.lml, want)
    assert got.lml == got.quad + got.logdet - 0.5 * N * np.log(2.0 * np.pi)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("trained", [False, True])
def test_gradient_matches_central_differences(kind, trained):
    N, D = 300, 3
    X, y = ref.problem(N, D)
    h = ref.hypers(D, trained)
    g = ref.grad_vector(ref.evaluate(kind, X, y, **h).grad)
    theta = np.concatenate([h["lengthscales"], [h["variance"], h["noise"], h["mean"]]])

    def lml_at(t):
        return ref.lml_only(kind, X, y, t[:D], t[D], t[D + 1], t[D + 2])

    fd = np.empty_like(theta)
    for k in range(theta.size):
        # Richardson step of two central differences: truncation O(step^4), round-off ~ 1e-16 |lml| / step
        step = 1e-3 * max(abs(theta[k]), 0.05)
        d = []
        for s in (step, 0.5 * step):
            tp, tm = theta.copy(), theta.copy()
            tp[k] += s
            tm[k] -= s
            d.append((lml_at(tp) - lml_at(tm)) / (2.0 * s))
        fd[k] = (4.0 * d[1] - d[0]) / 3.0
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print(f"{kind} trained={trained}: gradient vs central differences {err:.2e} of the largest entry")
    assert err <= 1e-8, (g, fd)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "N%d_D%d" % s[:2])
def test_permutation_floor(shape):
    """Reordering the rows changes only the order of the floating-point operations: the spread is the restatement's own round-off, which
    must stay 10x inside the 1e-10 / 1e-8 the GPU tests allow."""
    N, D, _ = shape
    X, y = ref.problem(N, D)
    perm = np.random.default_rng(0).permutation(N)
    for kind in KINDS:
        for trained in (False, True):
            h = ref.hypers(D, trained)
            a = ref.evaluate(kind, X, y, **h)
            b = ref.evaluate(kind, X[perm], y[perm], **h)
            scale = abs(a.quad) + abs(a.logdet) + 0.5 * N * np.log(2.0 * np.pi)
            e_lml = abs(a.lml - b.lml) / scale
            ga, gb = ref.grad_vector(a.grad), ref.grad_vector(b.grad)
            e_grad = np.abs(ga - gb).max() / max(np.abs(ga).max(), 1e-300)
            print(f"N={N} D={D} {kind} trained={trained}: lml floor {e_lml:.2e}, gradient floor {e_grad:.2e}")
            assert e_lml <= 1e-11 and e_grad <= 1e-11, (e_lml, e_grad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("trained", [False, True])
def test_cglb_bound_is_below_the_lml(kind, trained):
    N, D, M = 300, 3, 16
    from cglb_amd.data import synthetic_problem
    X, y, Z = synthetic_problem(N, D, M, seed=N + D)
    h = ref.hypers(D, trained)
    hyp = orc.Hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
    bound = orc.objective(kind, X, y, hyp, np.zeros(N), True, 1.0).bound
    lml = ref.evaluate(kind, X, y, with_grad=False, **h).lml
    assert bound <= lml, (bound, lml)
