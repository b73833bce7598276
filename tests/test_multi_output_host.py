"""Multi-output targets off the GPU: the data generator, the [N, P] shapes through backend/models.py (a recording stub stands in for the
HIP context), the NotImplementedError cases and the numpy restatement of the batched solver the GPU tests compare against."""
import numpy as np
import pytest
import torch

import multi_output_ref as mref
from oracle import cglb_oracle as orc


def test_synthetic_problem_p1_is_unchanged():
    from cglb_amd.data import synthetic_problem
    for N, D, M, seed in ((50, 3, 8, 0), (33, 1, 4, 7)):
        X, y, Z = synthetic_problem(N, D, M, seed=seed)
        Xo, yo, Zo = orc.synthetic_problem(N, D, M, seed=seed)   # the oracle's twin of today's generator
        assert y.shape == (N,)
        for a, b in ((X, Xo), (y, yo), (Z, Zo)):
            assert a.tobytes() == b.tobytes()
        X1, y1, Z1 = synthetic_problem(N, D, M, seed=seed, P=1)
        assert (X1.tobytes(), y1.tobytes(), Z1.tobytes()) == (X.tobytes(), y.tobytes(), Z.tobytes())
        X3, Y3, Z3 = synthetic_problem(N, D, M, seed=seed, P=3)
        assert Y3.shape == (N, 3) and Y3[:, 0].tobytes() == y.tobytes() and X3.tobytes() == X.tobytes() and Z3.tobytes() == Z.tobytes()
        assert not np.allclose(Y3[:, 1], Y3[:, 2])
        Y2 = synthetic_problem(N, D, M, seed=seed, P=2)[1]
        assert Y2.tobytes() == np.ascontiguousarray(Y3[:, :2]).tobytes()   # nested: column b does not depend on P


def test_cli_dataset_name_with_outputs():
    from cglb_amd.cli import get_dataset
    one, two = get_dataset("synthetic-60-2"), get_dataset("synthetic-60-2-2")
    assert one.train[1].ndim == 1 and two.train[1].shape == (one.train[1].shape[0], 2)
    np.testing.assert_array_equal(two.train[0], one.train[0])
    np.testing.assert_allclose(two.train[1][:, 0], one.train[1], rtol=1e-12, atol=1e-14)  # z-normalised per column: same up to the summation order


class StubContext:
    """Records what the model hands to the engine; returns shapes like HipContext."""

    def __init__(self, X, Y):
        self.N, self.D, self.device, self.world = X.shape[0], X.shape[1], torch.device("cpu"), 1
        self.y = torch.as_tensor(Y, dtype=torch.float64)
        self.P = 1 if self.y.dim() == 1 else self.y.shape[1]
        self.calls = []

    def set_option(self, *a): self.calls.append(("set_option",) + a)
    def set_hypers(self, *a): self.calls.append(("set_hypers",))
    def setup(self): self.calls.append(("setup",))

    def objective_and_grad(self, v, run_cg=True, *a, with_grad=True, **k):
        from cglb_amd.hip_context import ObjectiveResult
        self.calls.append(("objective_and_grad", tuple(v.shape), bool(run_cg)))
        M = 4
        g = dict(lengthscales=np.zeros(self.D), variance=0.0, noise=0.0, mean=0.0, Z=np.zeros((M, self.D)))
        return ObjectiveResult(-1.0, 0.5, 0.75, -0.25, 3, 0.125, g if with_grad else None)

    def pcg_multi(self, B, V0, *a):
        self.calls.append(("pcg_multi", tuple(B.shape), tuple(V0.shape)))
        return torch.ones_like(V0), 2, 0.0, np.zeros(self.P)

    def predict_multi(self, V, xnew):
        self.calls.append(("predict_multi", tuple(V.shape)))
        n = len(xnew)
        return torch.zeros((n, self.P), dtype=torch.float64), torch.ones(n, dtype=torch.float64)


def _model(cls, X, Y, ctx=None, **kw):
    from cglb_amd.backend.models import BaseKernel, GaussianLikelihood, InducingPointKernel, ScaleKernel
    kernel = InducingPointKernel(ScaleKernel(BaseKernel("rbf", X.shape[1])), X[:4])
    return cls((X, Y), GaussianLikelihood(), kernel, context=ctx if ctx is not None else StubContext(X, Y), **kw)


def test_shapes_through_models_with_stub_context():
    from cglb_amd.backend.models import CGLB, LowerBoundCG, PredictCG, log_density
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((20, 2)), rng.standard_normal((20, 3))
    m = _model(CGLB, X, Y)
    assert m.num_outputs == 3 and tuple(m.train_targets.shape) == (20, 3) and tuple(m.v_vec.shape) == (20, 3)
    loss = -LowerBoundCG(m)((torch.as_tensor(X), torch.as_tensor(Y)))
    loss.backward()
    assert ("objective_and_grad", (20, 3), True) in m.hip.calls
    assert m.cg_stats.steps == 3
    f_mean, f_var = PredictCG(m)(torch.as_tensor(X[:5]))
    assert tuple(f_mean.shape) == (5, 3) and tuple(f_var.shape) == (5, 3)
    assert ("pcg_multi", (20, 3), (20, 3)) in m.hip.calls and ("predict_multi", (20, 3)) in m.hip.calls
    assert tuple(log_density(m, Y[:5], f_mean, f_var).shape) == (5,)
    # one output, either shape: the tensors the single-output model always had
    for y1 in (Y[:, 0], Y[:, :1]):
        m1 = _model(CGLB, X, y1)
        assert m1.num_outputs == 1 and tuple(m1.train_targets.shape) == (20,) and tuple(m1.v_vec.shape) == (20, 1)
        LowerBoundCG(m1)(None)
        assert ("objective_and_grad", (20,), True) in m1.hip.calls
    with pytest.raises(ValueError):
        LowerBoundCG(m)((torch.as_tensor(X), torch.as_tensor(Y[:, :2])))


def test_unsupported_multi_output_models_raise():
    from cglb_amd.backend.models import CGLB, CGLBN2M, CGLBNM2, SGPR, SGPRN2M
    rng = np.random.default_rng(1)
    X, Y = rng.standard_normal((12, 2)), rng.standard_normal((12, 2))
    for cls in (SGPR, SGPRN2M, CGLBN2M, CGLBNM2):
        with pytest.raises(NotImplementedError, match="more than one target column"):
            _model(cls, X, Y)
    with pytest.raises(NotImplementedError, match="joint optimisation"):
        _model(CGLB, X, Y, joint_optimization=True)
    ranks = StubContext(X, Y)
    ranks.world = 2
    with pytest.raises(NotImplementedError, match="more than one rank"):
        _model(CGLB, X, Y, ctx=ranks)


def test_abi_declares_and_binds_the_multi_entry_points():
    import os
    import re
    from cglb_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cglb_hip.h")).read()
    declared = set(re.findall(r"\b(cglb_[a-z0-9_]+)\s*\(", header))
    for name in ("cglb_set_targets", "cglb_matmat", "cglb_pcg_solve_multi", "cglb_objective_and_grad_multi", "cglb_predict_multi", "cglb_time_matmat"):
        assert name in declared and name in _lib.SIGNATURES


def test_lockstep_loop_equals_independent_solves_when_they_stop_together():
    """Validation of the REFERENCE the GPU tests compare against (tests/multi_output_ref.py), not of the library: it passes without the
    feature.  With max_error 0 and a step cap every column runs the same number of steps: the lockstep loop must then reproduce P single
    solves of the oracle, and a column equal to the mean must stay exactly zero without disturbing the others."""
    X, Y, hyp = mref.problem(120, 2, 8, 3, seed=3)
    Y[:, 1] = hyp.mean
    cov, terms = orc.dense_cov("rbf", X, hyp), orc.common_terms("rbf", X, hyp)
    pre = lambda r: orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r)
    V, steps, half = mref.lockstep_pcg(cov, Y - hyp.mean, np.zeros_like(Y), pre, 0.0, 7, 5)
    assert steps == 7 and np.all(np.isfinite(V)) and not V[:, 1].any()
    for b in (0, 2):
        v, st = orc.pcg(lambda x: cov @ x, Y[:, b] - hyp.mean, np.zeros(len(X)), pre, 0.0, 7, 5)
        # cov @ [N, P] and cov @ [N] add in different orders: N eps = 1.3e-14 per product, times the condition of the system (noise 0.05
        # under unit variance: <= 1e3 after preconditioning) over 7 steps - 1e-10 bounds it with a decade to spare
        np.testing.assert_allclose(V[:, b], v, rtol=0, atol=1e-10 * np.abs(v).max())
        assert half[b] == pytest.approx(st.residual_error, rel=1e-9)
