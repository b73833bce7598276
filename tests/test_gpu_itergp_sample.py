"""Pathwise posterior samples of the iterative exact-GP class (cglb_itergp_sample, `SampleIterGPR`) against the dense restatement
tests/sample_ref.py.

Cases: gpr_ref.problem at (N, D) = (300, 3) with all three kernels, (257, 8) and (200, 40) with Matern-3/2; F = 65 features, S in (1, 9)
samples, n_new in (1, 17) new points that include a training row and a point at 10^3 in every coordinate.

1. Re-assembly: with the library's own solves U, the samples equal mean + Phi(X*) w + K_*f U of the restatement to 1e-10 of
   max(|f|, sqrt(variance)) - the level the cross products are held to elsewhere; independent of the CG path.
2. The solve: P = Q_ff + noise I is below K, so r^T K^-1 r <= r^T P^-1 r <= 2 max_error and every sample value is within
   sqrt(2 variance max_error) of its value at the exact solve (include/cglb_hip.h); 1e-9 sqrt(variance) for the kernel values.  At
   max_error = 1e-12 and at the default 1e-3, where the bound is loose but must hold.  The returned half_rz is at most max_error unless the
   step limit ended the solve.
3. Bitwise repeatable; cglb_itergp_predict before and after returns bitwise equal means and variances; a valid variance cache stays valid.
4. `SampleIterGPR`: shape [S, n_new, 1], reproducible from the model's seed, fresh draws at every call, one prior basis with fixed_features.
5. CGLB_ERR_BAD_ARG with a message on an fp32 context, with two target columns and with logdet_bound 1.
"""
import functools
import math

import numpy as np
import pytest
import torch

import gpr_ref as ref
import sample_ref as sr

pytestmark = pytest.mark.gpu
CASE_IDS = ["N%d_D%d_%s" % c[:3] for c in sr.SAMPLE_CASES]


def _context(X, y, kind, h, k, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, k, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)   # Z is a placeholder: the class selects its own
    return ctx


@functools.lru_cache(maxsize=None)
def _dense(case, S, n_new):
    """The dense restatement of a case, computed once and shared (read-only)."""
    N, D, kind, _k = case
    X, y = ref.problem(N, D)
    xnew = sr.sample_new_points(X, n_new)
    omega, b, W, eps = sr.sample_draws(N, D, kind, S)
    f, _ = sr.sample(kind, X, y, sr.sample_hypers(D), xnew, omega, b, W, eps)
    f.setflags(write=False)
    return X, y, xnew, (omega, b, W, eps), f


@pytest.mark.parametrize("n_new", sr.SAMPLE_NEW)
@pytest.mark.parametrize("S", sr.SAMPLE_S)
@pytest.mark.parametrize("case", sr.SAMPLE_CASES, ids=CASE_IDS)
def test_samples_match_the_dense_restatement(case, S, n_new):
    N, D, kind, k = case
    h = sr.sample_hypers(D)
    X, y, xnew, draws, dense = _dense(case, S, n_new)
    scale = math.sqrt(h["variance"])
    ctx = _context(X, y, kind, h, k)
    try:
        tight = ctx.itergp_sample(xnew, *draws, max_error=1e-12, max_cg_iter=1000, return_solves=True)   # no evaluation yet: the preconditioner is built first
        again = ctx.itergp_sample(xnew, *draws, max_error=1e-12, max_cg_iter=1000, return_solves=True)
        loose = ctx.itergp_sample(xnew, *draws)                                                            # max_error = 1e-3
    finally:
        ctx.close()
    f, U = tight.samples.cpu().numpy(), tight.solves.cpu().numpy()
    assert f.shape == (S, n_new) and U.shape == (S, N) and loose.solves is None
    # 1. re-assembly at the library's solves
    want, _ = sr.sample(kind, X, y, h, xnew, *draws, U=U)
    err = np.abs(f - want) / np.maximum(np.abs(want), scale)
    print(f"{kind} N={N} D={D} S={S} n_new={n_new}: re-assembly {err.max():.2e} of max(|f|, sqrt f); steps {tight.steps} / {loose.steps}, "
          f"half_rz {tight.residual_error:.2e} / {loose.residual_error:.2e}")
    assert err.max() <= 1e-10
    # 2. the solve
    for res, max_error in ((tight, 1e-12), (loose, 1e-3)):
        got = res.samples.cpu().numpy()
        bound = math.sqrt(2.0 * h["variance"] * max_error) + 1e-9 * scale
        print(f"    max_error {max_error:.0e}: largest deviation from the dense samples {np.abs(got - dense).max():.2e}, bound {bound:.2e}")
        assert res.residual_error <= max_error or res.steps == 1000
        assert np.abs(got - dense).max() <= bound
    # 3. bitwise repeatable
    assert np.array_equal(again.samples.cpu().numpy(), f) and np.array_equal(again.solves.cpu().numpy(), U)
    assert (again.steps, again.residual_error) == (tight.steps, tight.residual_error)


@pytest.mark.parametrize("case", [sr.SAMPLE_CASES[1], sr.SAMPLE_CASES[4]], ids=[CASE_IDS[1], CASE_IDS[4]])
def test_sampling_leaves_the_predictive_state_alone(case):
    N, D, kind, k = case
    h = sr.sample_hypers(D)
    X, y, xnew, draws, _dense_f = _dense(case, 9, 17)

    def run(sampling):
        """evaluation, cache, then twice (predictive, cached predictive[, samples]): every predictive solve is warm-started at the stored alpha,
        so a sampling call that moved alpha, the preconditioner or the cache would move what follows it"""
        ctx = _context(X, y, kind, h, k)
        out = []
        try:
            ctx.itergp_objective_and_grad(np.random.default_rng(0).standard_normal((2, k + N)), torch.zeros(N, dtype=torch.float64, device=ctx.device),
                                          with_grad=False)
            assert ctx.itergp_var_cache(12) >= 1
            for _ in range(3):
                out += [t.cpu().numpy() for t in ctx.itergp_predict(xnew, max_error=1e-6)]
                out += [t.cpu().numpy() for t in ctx.itergp_predict_cached(xnew, max_error=1e-6)]
                if sampling:
                    out.append(ctx.itergp_sample(xnew, *draws, max_error=1e-6).samples.cpu().numpy())
                    assert int(ctx.get_stat("itergp_cache_request")) == 12
        finally:
            ctx.close()
        return out

    with_samples, plain = run(True), run(False)
    assert np.array_equal(with_samples[4], with_samples[9]) and np.array_equal(with_samples[4], with_samples[14])   # the samples themselves repeat
    # the predictive before and after a sampling call (rounds two and three: the first one moves alpha from the evaluation's to its own tolerance)
    for q in range(4):
        assert np.array_equal(with_samples[5 + q], with_samples[10 + q])
    del with_samples[14], with_samples[9], with_samples[4]
    assert len(with_samples) == len(plain) == 12
    for got, want in zip(with_samples, plain):                        # as if no sample had been drawn in between
        assert np.array_equal(got, want)


@pytest.fixture
def backend(tmp_path):
    from cglb_amd.backend import interface
    interface.configure_backend(logdir=str(tmp_path))
    interface.set_default_float("fp64")
    interface.set_default_jitter(1e-6)
    return interface


@pytest.mark.parametrize("kernel", ["SquaredExponentialConfig", "Matern32Config", "Matern52Config"])
def test_sample_itergpr(backend, kernel):
    from cglb_amd.backend import config
    from cglb_amd.backend.models import PredictIterGPR, SampleIterGPR
    X, y = ref.problem(300, 3)
    xnew = torch.as_tensor(sr.sample_new_points(X, 17))

    def model(seed):
        return backend.create_model(config.IterGPRConfig(getattr(config, kernel)(), prec_size=8, seed=seed), (X, y))

    m = model(3)
    sampler = SampleIterGPR(m)
    assert (sampler.num_features, sampler.max_error, sampler.features) == (1024, 1e-3, None)
    a, b = sampler(xnew, 5), sampler(xnew, 5)
    assert a.shape == (5, 17, 1) and a.dtype == torch.float64 and bool(torch.isfinite(a).all())
    assert not torch.equal(a, b)                                        # fresh draws at every call
    again = SampleIterGPR(model(3))(xnew, 5)
    assert torch.equal(a, again)                                        # reproducible from the model's seed
    assert not torch.equal(a, SampleIterGPR(model(4))(xnew, 5))
    # one prior basis: drawn at construction, so two calls from one generator state draw the same weights and noise
    fixed = SampleIterGPR(m, num_features=65, max_error=1e-6, fixed_features=True)
    state = m.generator.get_state()
    c = fixed(xnew, 3)
    m.generator.set_state(state)
    d = fixed(xnew, 3)
    assert torch.equal(c, d) and fixed.features[0].shape == (65, 3)
    # the draws scatter around the predictive mean on the scale of the predictive deviation (a sanity check of the units, not a test of the law)
    mean, var = PredictIterGPR(m, max_error=1e-8)(xnew)
    many = SampleIterGPR(m, num_features=512, max_error=1e-8)(xnew, 64).cpu()
    z = (many.mean(dim=0) - mean.cpu()).abs() / (var.cpu().clamp(min=1e-12) / 64).sqrt()
    print(f"{kernel}: largest |sample mean - predictive mean| in standard errors of 64 draws: {float(z.max()):.2f}")
    assert float(z.max()) < 8.0
    with pytest.raises(ValueError):
        SampleIterGPR(object())


def test_refusals():
    N, D, k = 65, 3, 4
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    omega, b, W, eps = sr.sample_draws(N, D, "rbf", 2)
    ctx = _context(X, y, "rbf", h, k, dtype=torch.float32)
    try:
        with pytest.raises(ValueError, match="-t fp64"):
            ctx.itergp_sample(X[:3], omega, b, W, eps)
    finally:
        ctx.close()
    ctx = _context(X, y, "rbf", h, k)
    try:
        good = ctx.itergp_sample(X[:3], omega, b, W, eps).samples.cpu().numpy()
        ctx.set_targets(np.stack([y, -y], axis=1))
        with pytest.raises(ValueError, match="logdet_bound 0|one target column"):
            ctx.itergp_sample(X[:3], omega, b, W, eps)
        ctx.set_targets(y)
        ctx.set_option("logdet_bound", 1)
        with pytest.raises(ValueError, match="logdet_bound 0"):
            ctx.itergp_sample(X[:3], omega, b, W, eps)
        ctx.set_option("logdet_bound", 0)
        ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:k].copy(), 1e-6)
        assert np.array_equal(ctx.itergp_sample(X[:3], omega, b, W, eps).samples.cpu().numpy(), good)   # the context is still usable
    finally:
        ctx.close()
