"""The numpy restatement of the iterative exact-GP estimator (tests/itergp_ref.py) against the dense one (tests/gpr_ref.py), without a GPU.

With the unit probes eps = sqrt(t) I, t = k + N, the probes satisfy sum_i z_i z_i^T = t P exactly; run to convergence with
max_cg_iter = lanczos_iter = N the estimator is then the dense log-determinant and its gradient the exact one.  The errors printed here are
what the GPU tolerances of tests/test_gpu_itergp.py hang on."""
import numpy as np
import pytest

import gpr_ref as ref
import itergp_ref as iref

CASES = iref.EXACT_LIMIT_CASES


def exact_limit(kind, N, D, k):
    X, y = ref.problem(N, D)
    h = iref.exact_limit_hypers(D)
    want = ref.evaluate(kind, X, y, **h)
    got = iref.evaluate(kind, X, y, eps=iref.unit_probes(k, N), k=k, max_error=1e-20, max_cg_iter=N, lanczos_iter=N, **h)
    return X, y, h, want, got


def exact_limit_errors(kind, N, D, k):
    """(value error / scale, gradient error / largest entry, solve residual / |e|) of the restatement with unit probes."""
    X, y, h, want, got = exact_limit(kind, N, D, k)
    scale = abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi)
    verr = max(abs(got.lml - want.lml), abs(got.quad - want.quad), abs(got.logdet - want.logdet)) / scale
    g, rg = iref.grad_vector(got.grad), ref.grad_vector(want.grad)
    gerr = np.abs(g - rg).max() / np.abs(rg).max()
    K = want.L @ want.L.T
    e = y - h["mean"]
    res = np.linalg.norm(K @ got.V[:, 0] - e) / np.linalg.norm(e)
    return verr, gerr, res, got


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_D%d_k%d" % c)
def test_unit_probes_give_the_dense_value_and_gradient(case, kind):
    N, D, k = case
    verr, gerr, res, got = exact_limit_errors(kind, N, D, k)
    print(f"N={N} D={D} k={k} {kind}: steps {got.steps}, value {verr:.2e} of the scale, gradient {gerr:.2e} of the largest entry, residual {res:.2e}")
    assert got.steps <= N
    assert verr <= 1e-11 and gerr <= 1e-9 and res <= 1e-10


def test_probes_have_covariance_P():
    N, D, k = 40, 3, 6
    X, y = ref.problem(N, D)
    h = iref.exact_limit_hypers(D)
    got = iref.evaluate("rbf", X, y, eps=iref.unit_probes(k, N), k=k, max_error=1e30, max_cg_iter=0, with_grad=False, **h)
    assert got.steps == 0 and got.pap_log.shape == (0, 1 + k + N) and got.correction == 0.0
    # rz_0i = z_i^T P^-1 z_i and sum_i of it = t tr(P^-1 P) = t N
    t = k + N
    assert abs(got.rz_log[0, 1:].sum() - t * N) <= 1e-9 * t * N


def test_random_probes_are_close_and_the_kernel_perturbation_is_small():
    N, D, k, t = 300, 3, 8, 10
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    eps = np.random.default_rng(0).standard_normal((t, k + N))
    want = ref.evaluate("rbf", X, y, **h)
    scale = abs(want.quad) + abs(want.logdet) + 0.5 * N * np.log(2.0 * np.pi)
    for iters in (5, 20):
        a = iref.evaluate("rbf", X, y, eps=eps, k=k, max_error=0.0, max_cg_iter=iters, **h)
        b = iref.evaluate("rbf", X, y, eps=eps, k=k, max_error=0.0, max_cg_iter=iters, perturb=1e-13, **h)
        assert a.steps == b.steps == iters
        print(f"{iters} steps: estimate {a.lml!r}, dense {want.lml!r}; kernel values perturbed by 1e-13: {abs(a.lml - b.lml) / scale:.2e} of the scale")
        # The recurrence is not restarted: once the leading Ritz values have converged (RBF: within ~10 steps) the Lanczos vectors lose their
        # orthogonality and a perturbation of 1e-13 grows to 1e-5 .. 1e-3 of the iterate at step 20, while 5 steps stay at round-off.
        if iters == 5:
            assert abs(a.lml - b.lml) <= 1e-11 * scale
    assert abs(a.logdet - want.logdet) <= 0.01 * abs(want.logdet)     # ten probes, 20 Lanczos steps: the log-determinant to a per cent
