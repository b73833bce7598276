"""Model and objective classes — mirror of the reference's cglb/backend/pytorch/models.py for the CGLB path.

Same class names and call contracts (`CGLB`, `CommonTerms`-free `LowerBoundCG`, `PredictCG`, `PredictLogdensityCG`,
`log_density`, `gaussian`); GPyTorch's module tree (likelihood / mean_module / covar_module with raw, softplus-
constrained parameters) is restated with plain torch.nn modules so that `model.parameters()`, the parameter
dictionary keys (interface.model_parameters) and `torch.autograd.grad(loss, params)` (optimizer.py:95-98) behave
the same.  All numerical work is done by libcglb_hip.so through `HipContext`; the bound is exposed to autograd
by a `torch.autograd.Function` whose backward returns the analytic gradient computed on the GPU (v detached,
models.py:257-274).
"""
from __future__ import annotations

import math
import weakref
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from ..dist_context import make_context
from .. import _lib
from ..hip_context import KINDS, HipContext
from .conjugate_gradient import ConjugateGradient, ConjugateGradientStats, KernelOperator, NystromPreconditioner

Tensor = torch.Tensor
GenericTensor = Union[np.ndarray, Tensor]
Data = Tuple[GenericTensor, GenericTensor]


def _inv_softplus(x: Tensor) -> Tensor:
    return x + torch.log(-torch.expm1(-x))


class _Constrained(nn.Module):
    """value = softplus(raw) + lower_bound  (gpytorch Positive / GreaterThan constraints)."""

    def __init__(self, shape, lower_bound: float = 0.0):
        super().__init__()
        self.lower_bound = float(lower_bound)
        self.raw = nn.Parameter(torch.zeros(shape, dtype=torch.float64))

    @property
    def value(self) -> Tensor:
        return F.softplus(self.raw) + self.lower_bound

    def set(self, value, exact: bool = False):
        """raw = inv_softplus(value - lower_bound), which gives `value` back to a unit in the last place.  `exact` (what `load` asks for, so
        that a saved model loads bit for bit): the raw that gives it back exactly, wherever there is one within 1e-9 of that."""
        target = torch.as_tensor(value, dtype=torch.float64).reshape(self.raw.shape)
        v = target - self.lower_bound
        if (v <= 0).any():
            raise ValueError(f"value must exceed the lower bound {self.lower_bound}")
        raw = _inv_softplus(v)
        if exact:   # bisection for the smallest raw whose value is not below the target; kept if its value is the target
            width = 1e-9 * raw.abs().clamp(min=1.0)
            lo, hi = raw - width, raw + width
            for _ in range(64):
                mid = lo + (hi - lo) / 2
                below = F.softplus(mid) + self.lower_bound < target
                lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
            raw = torch.where(F.softplus(hi) + self.lower_bound == target, hi, raw)
        with torch.no_grad():
            self.raw.copy_(raw)


class BaseKernel(nn.Module):
    """RBFKernel / MaternKernel(nu=1.5) with ARD lengthscales (pytorch/interface.py:207-230)."""

    def __init__(self, kind: str, ard_num_dims: int):
        super().__init__()
        self.kind = kind  # "rbf" | "matern32" | "matern52": a key of hip_context.KINDS
        self._lengthscale = _Constrained((1, ard_num_dims))

    @property
    def lengthscale(self) -> Tensor:
        return self._lengthscale.value

    @lengthscale.setter
    def lengthscale(self, value):
        self._lengthscale.set(value)


class ScaleKernel(nn.Module):
    def __init__(self, base_kernel: BaseKernel):
        super().__init__()
        self.base_kernel = base_kernel
        self._outputscale = _Constrained(())

    @property
    def outputscale(self) -> Tensor:
        return self._outputscale.value

    @outputscale.setter
    def outputscale(self, value):
        self._outputscale.set(value)


class InducingPointKernel(nn.Module):
    """gpytorch.kernels.InducingPointKernel stand-in: base kernel + trainable inducing points (interface.py:297-299)."""

    def __init__(self, base_kernel: ScaleKernel, inducing_points):
        super().__init__()
        self.base_kernel = base_kernel
        self.inducing_points = nn.Parameter(torch.as_tensor(inducing_points, dtype=torch.float64).clone())


class _NoiseCovar(nn.Module):
    def __init__(self, lower_bound):
        super().__init__()
        self._noise = _Constrained((1,), lower_bound)

    @property
    def noise(self) -> Tensor:
        return self._noise.value


class GaussianLikelihood(nn.Module):
    """noise >= 1e-6 for SGPR/CGLB (pytorch/interface.py:269-273)."""

    def __init__(self, lower_bound: float = 1e-6):
        super().__init__()
        self.noise_covar = _NoiseCovar(lower_bound)

    @property
    def noise(self) -> Tensor:
        return self.noise_covar.noise

    @noise.setter
    def noise(self, value):
        self.noise_covar._noise.set(value)


class ConstantMean(nn.Module):
    def __init__(self):
        super().__init__()
        self.constant = nn.Parameter(torch.zeros((), dtype=torch.float64))


class GPR(nn.Module):
    """models.py:38-47"""

    def __init__(self, data: Data, likelihood: GaussianLikelihood, kernel: nn.Module):
        super().__init__()
        x = torch.as_tensor(data[0])
        self.train_inputs = (x.reshape(x.shape[0], -1),)
        y = torch.as_tensor(data[1])
        # [N, P] targets stay 2-D for P > 1 (one kernel, mean and noise shared by the outputs); a single column is the flat vector
        self.train_targets = y if (y.dim() == 2 and y.shape[0] == x.shape[0] and y.shape[1] > 1) else y.reshape(-1)
        self.likelihood = likelihood
        self.mean_module = ConstantMean()
        self.covar_module = kernel

    @property
    def num_outputs(self) -> int:
        return int(self.train_targets.shape[1]) if self.train_targets.dim() == 2 else 1

    def check_same_data(self, data: Data) -> None:
        """ValueError unless (x, y) is the training set the HIP context was built on (same shapes and content).  The full comparison
        runs once per data object: the last accepted pair is remembered (weakly), so an
        optimiser that hands over the same arrays at every evaluation does not pay N*D comparisons inside its loop."""
        x, y = data
        if x is self.train_inputs[0] and y is self.train_targets:
            return
        accepted = getattr(self, "_accepted_data", None)   # weak references to the last pair that passed the full comparison
        if accepted is not None and accepted[0]() is x and accepted[1]() is y:
            return
        x_in, y_in = x, y
        # everything on the host in fp64, whatever device the model or the caller keep their tensors on
        x = torch.as_tensor(x).detach().cpu().to(torch.float64)
        y = torch.as_tensor(y).detach().cpu().to(torch.float64)
        x = x.reshape(x.shape[0], -1) if x.ndim else x.reshape(1, 1)
        tx = self.train_inputs[0].detach().cpu().to(torch.float64)
        ty = self.train_targets.detach().cpu().to(torch.float64)
        if ty.dim() == 1:   # one output: [N] and [N, 1] are the same targets
            y = y.reshape(-1)
        if x.shape != tx.shape or y.shape != ty.shape:
            raise ValueError(f"LowerBoundCG was given data of shape {tuple(x.shape)}/{tuple(y.shape)} but the model holds the training set "
                             f"{tuple(tx.shape)}/{tuple(ty.shape)}: the bound is only defined on the model's own training data")
        if not (torch.equal(y, ty) and torch.equal(x, tx)):
            raise ValueError("LowerBoundCG was given data that differs from the model's training set")
        try:
            self._accepted_data = (weakref.ref(x_in), weakref.ref(y_in))
        except TypeError:  # lists / scalars cannot be weakly referenced: compared in full every time
            self._accepted_data = None

    def set_train_inputs(self, x) -> None:
        """Replaces the training inputs ([N, d], any device; the targets stay): the model's `train_inputs`, the remembered pair of `check_same_data`
        and the library's copy (every class whose context is one `HipContext`: SGPR, CGLB and its log-det variants, ExactGPR, IterGPR).  The
        library forgets its hyper-parameters with the inputs (its scaled operand sets are made from both), so whatever the class remembers as
        pushed is void; a warm start (`v_vec`) is kept."""
        x = torch.as_tensor(x).detach()
        x = x.reshape(x.shape[0], -1)
        if tuple(x.shape) != tuple(self.train_inputs[0].shape):
            raise ValueError(f"set_train_inputs was given inputs of shape {tuple(x.shape)} but the model holds {tuple(self.train_inputs[0].shape)}")
        if not hasattr(self.hip, "set_inputs"):
            raise NotImplementedError(f"{type(self).__name__}: the training inputs can be replaced on one rank only")
        self.train_inputs = (x,)
        self._accepted_data = None
        if hasattr(self, "_pushed"):   # IterGPR: the key of the last set_hypers
            self._pushed = None
        self.hip.set_inputs(x)


_ONE_RANK = "{name} is not available on more than one rank (only CGLB runs row-sharded)"


def _one_rank_context(name: str, context, data_x, data_y, num_inducing: int, kind: str, dtype, device):
    """The HIP context of a class that runs on one rank only: the one handed in, or a new `HipContext`; refused on more than one rank."""
    if context is None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(_ONE_RANK.format(name=name) + "; run it as a single process")
        return HipContext(data_x, data_y, num_inducing, kind, dtype=dtype, device=device)
    if getattr(context, "world", 1) > 1:
        raise NotImplementedError(_ONE_RANK.format(name=name))
    return context


def _variant_context(model, data_x, data_y, num_inducing: int, kind: str, dtype, device, context):
    """The HIP context of a model whose bound is not plain CGLB: one rank only (the N-rank path implements the Jensen / CG bound), with the
    two bound options set on it (include/cglb_hip.h "logdet_bound", "quad_term")."""
    context = _one_rank_context(type(model).__name__, context, data_x, data_y, num_inducing, kind, dtype, device)
    context.set_option("logdet_bound", model.LOGDET_BOUND)
    context.set_option("quad_term", model.QUAD_TERM)
    return context


class SGPR(GPR):
    """Titsias' collapsed bound (tensorflow/models.py:353-413 with the NM^2 trace term): the exact quadratic term at v = 0 - no solve, no
    N^2 work - and the log-det bound of option LOGDET_BOUND (1: NM^2, the SGPR ELBO; 2: N^2M, SGPRN2M).  Same module tree and parameter
    keys as CGLB; no v_vec, no cg_stats."""

    LOGDET_BOUND = 1
    QUAD_TERM = 1

    def __init__(self, data: Data, likelihood: GaussianLikelihood, kernel: InducingPointKernel, dtype: torch.dtype = torch.float64,
                 device: Optional[torch.device] = None, context=None):
        super().__init__(data, likelihood, kernel)
        self.dtype = dtype
        if self.num_outputs > 1:
            raise NotImplementedError(f"{type(self).__name__} is not available for more than one target column (only CGLB takes [N, P] targets)")
        kind = kernel.base_kernel.base_kernel.kind
        self.hip = _variant_context(self, self.train_inputs[0], self.train_targets, kernel.inducing_points.shape[0], kind, dtype, device, context)
        self._zero_v = torch.zeros(self.hip.N, dtype=dtype, device=self.hip.device)  # the library treats v as 0 (quad_term 1); shape check only

    # constrained hyper-parameters, as tensors attached to the raw parameters
    def hyper_tensors(self):
        k = self.covar_module
        return (k.base_kernel.base_kernel.lengthscale.reshape(-1), k.base_kernel.outputscale.reshape(()),
                self.likelihood.noise.reshape(()), self.mean_module.constant.reshape(()), k.inducing_points)

    def push_hypers(self, jitter: float):
        ls, var, noise, mean, Z = [t.detach() for t in self.hyper_tensors()]
        self.hip.set_hypers(ls.cpu().numpy(), float(var), float(noise), float(mean), Z.cpu(), jitter)


class SGPRN2M(SGPR):
    """SGPR with the N^2M log-det bound (tensorflow/models.py:353-413): one N^2 M pass per evaluation (kernels_n2m.hip), fp64 only."""

    LOGDET_BOUND = 2


class CGLB(SGPR):
    """models.py:54-87: SGPR + the persistent warm-start vector v_vec (zeros[N,1], no grad) and cg_stats."""

    LOGDET_BOUND = 0   # Jensen (models.py:215-244); QUAD_TERM 0: the CG quadratic term.  Plain CGLB leaves the options untouched
    QUAD_TERM = 0

    def __init__(self, data: Data, likelihood: GaussianLikelihood, kernel: InducingPointKernel, dtype: torch.dtype = torch.float64,
                 device: Optional[torch.device] = None, max_error: Optional[float] = None, joint_optimization: bool = False,
                 vzero: bool = False, context=None):
        """`context`: the engine behind the model - by default `make_context` builds it: a `HipContext` in a single-process run, one rank
        of a `DistHipContext` (rows of K_ff dealt over the ranks, collectives inside libcglb_hip.so) when a torch.distributed process
        group with more than one rank is initialised; every rank then holds the full replicated `v_vec` and evaluates identical
        (loss, gradient) pairs.  Tests inject `distributed.PyDistContext` here.
        The three arguments before it are the TF twin's (tensorflow/models.py:31-51): the torch reference never passes them
        (pytorch/interface.py:315-323) and neither does `create_model` unless `configure_backend(config_semantics="tf")`.
        `max_error` becomes the default tolerance of `LowerBoundCG`; `joint_optimization` (without `vzero`) makes `v_vec` a trainable
        parameter and skips CG; `vzero` keeps v = 0 and skips CG (tensorflow/models.py:161-164)."""
        GPR.__init__(self, data, likelihood, kernel)
        self.dtype = dtype
        self.max_error, self.joint_optimization, self.vzero = max_error, bool(joint_optimization), bool(vzero)
        kind = kernel.base_kernel.base_kernel.kind
        if self.num_outputs > 1:
            name = type(self).__name__
            if self.LOGDET_BOUND != 0:
                raise NotImplementedError(f"{name} is not available for more than one target column (only CGLB takes [N, P] targets)")
            if self.joint_optimization and not self.vzero:
                raise NotImplementedError("joint optimisation of v (the TF twin's opt-in) is not available for more than one target column")
            import torch.distributed as dist
            if getattr(context, "world", 1) > 1 or (context is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
                raise NotImplementedError(f"{name} with more than one target column is not available on more than one rank; "
                                          f"run it as a single process")
        if self.LOGDET_BOUND != 0:   # a log-det ablation: one rank, the option set on the context
            context = _variant_context(self, self.train_inputs[0], self.train_targets, kernel.inducing_points.shape[0], kind, dtype, device, context)
        elif context is None:
            context = make_context(self.train_inputs[0], self.train_targets, kernel.inducing_points.shape[0], kind, dtype=dtype, device=device)
        self.hip = context
        if getattr(context, "world", 1) > 1 and self.joint_optimization and not self.vzero:
            raise NotImplementedError("joint optimisation of v (the TF twin's opt-in) is not available on more than one rank")
        v0 = self._build_v_vec()
        # v0 trainable only under joint optimisation (tensorflow/models.py:47-48); otherwise a plain buffer without grad (models.py:59-68)
        self._v_vec = nn.Parameter(v0) if (self.joint_optimization and not self.vzero) else v0
        self._hyper_token = None

    def _build_v_vec(self) -> Tensor:  # models.py:59-68
        return torch.zeros((self.hip.N, self.num_outputs), dtype=self.dtype, device=self.hip.device, requires_grad=False)

    @property
    def v_vec(self) -> Tensor:
        return self._v_vec

    @property
    def cg_stats(self) -> Optional[ConjugateGradientStats]:
        return getattr(self, "_cg_stats", None)

    @cg_stats.setter
    def cg_stats(self, value: ConjugateGradientStats):  # models.py:80-87
        steps, error = value.steps, value.residual_error
        if isinstance(steps, torch.Tensor):
            steps = steps.detach().cpu().numpy()
        if isinstance(error, torch.Tensor):
            error = error.detach().cpu().numpy()
        self._cg_stats = ConjugateGradientStats(steps, error)

class CGLBN2M(CGLB):
    """CGLB with the N^2M log-det bound (tensorflow/models.py:311-350): one N^2 M pass per setup, one more per gradient, fp64 only."""

    LOGDET_BOUND = 2


class CGLBNM2(CGLB):
    """CGLB with the NM^2 log-det bound log|Q_ff + s I| + tr(K_ff - Q_ff)/s (tensorflow/models.py:271-308)."""

    LOGDET_BOUND = 1


class _NoInducingGPR(GPR):
    """The module tree and parameter keys of the SGPR family without the inducing points: `covar_module` is the ScaleKernel itself."""

    def hyper_tensors(self):
        k = self.covar_module
        return (k.base_kernel.lengthscale.reshape(-1), k.outputscale.reshape(()), self.likelihood.noise.reshape(()),
                self.mean_module.constant.reshape(()))


class ExactGPR(_NoInducingGPR):
    """Exact GP regression (GPRConfig: tensorflow/interface.py:200-206 builds gpflow's GPR with a constant mean; pytorch/interface.py:561-604
    trains it on ExactMarginalLogLikelihood times n).  The N x N kernel matrix is factored on the GPU (cglb_gpr_*: fp64, one rank, one
    target column)."""

    def __init__(self, data: Data, likelihood: GaussianLikelihood, kernel: ScaleKernel, dtype: torch.dtype = torch.float64,
                 device: Optional[torch.device] = None, context=None):
        super().__init__(data, likelihood, kernel)
        self.dtype = dtype
        if self.num_outputs > 1:
            raise NotImplementedError("ExactGPR is not available for more than one target column (only CGLB takes [N, P] targets)")
        # M = 1: placeholder
        self.hip = _one_rank_context("ExactGPR", context, self.train_inputs[0], self.train_targets, 1, kernel.base_kernel.kind, dtype, device)
        self.push_hypers()   # an fp32 context is refused here, with the library's message, not at the first evaluation

    def push_hypers(self):
        ls, var, noise, mean = [t.detach() for t in self.hyper_tensors()]
        self.hip.gpr_set_hypers(ls.cpu().numpy(), float(var), float(noise), float(mean))


class IterGPR(_NoInducingGPR):
    """Iterative exact GP regression: the "Iterative GP" baseline (pytorch/interface.py:233-260 builds it on gpytorch's ExactGP with a
    pivoted-Cholesky preconditioner of rank `_prec_size()` = 100, batched CG and stochastic Lanczos quadrature).  The module tree and parameter
    keys of ExactGPR; O(N) memory.  The estimator is the library's (cglb_itergp_*: fp64, one rank, one target column): `num_probes` probe
    vectors drawn on the host from this model's generator, one batched solve warm-started at the persistent `v_vec`, the log-determinant from
    the Lanczos coefficients of the solve.  gpytorch's random numbers and stop rule are not reproduced."""

    def __init__(self, data: Data, likelihood: GaussianLikelihood, kernel: ScaleKernel, dtype: torch.dtype = torch.float64,
                 device: Optional[torch.device] = None, context=None, num_probes: int = 10, prec_size: int = 100, max_error: float = 1.0,
                 max_cg_iter: int = 1000, lanczos_iter: int = 20, seed: int = 0, deterministic_probes: bool = False, pred_var_rank: int = 0):
        super().__init__(data, likelihood, kernel)
        self.dtype = dtype
        self.pred_var_rank = int(pred_var_rank)   # > 0: PredictIterGPR takes its variances from a Lanczos variance cache of this rank
        if self.num_outputs > 1:
            raise NotImplementedError("IterGPR is not available for more than one target column (only CGLB takes [N, P] targets)")
        if dtype != torch.float64:
            raise ValueError("the iterative exact GP class needs fp64 (-t fp64)")
        n = int(self.train_inputs[0].shape[0])
        self.num_probes, self.prec_size = int(num_probes), min(int(prec_size), n)
        self.max_error, self.max_cg_iter, self.lanczos_iter = float(max_error), int(max_cg_iter), int(lanczos_iter)
        context = _one_rank_context("IterGPR", context, self.train_inputs[0], self.train_targets, self.prec_size, kernel.base_kernel.kind, dtype, device)
        self.hip = context
        self.register_buffer("v_vec", torch.zeros(n, dtype=dtype, device=context.device), persistent=False)   # the warm start of the data column
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(int(seed))
        self.deterministic_probes = bool(deterministic_probes)
        self._eps = None
        self.cg_stats: Optional[ConjugateGradientStats] = None
        self._placeholder_Z = self.train_inputs[0][:self.prec_size].detach().cpu().to(torch.float64)   # replaced by the pivots at every evaluation
        self._pushed = None

    def probes(self) -> Tensor:
        """[num_probes, prec_size + N] standard-normal draws: fresh at every call, or one draw kept when `deterministic_probes`."""
        if self._eps is None or not self.deterministic_probes:
            self._eps = torch.randn(self.num_probes, self.prec_size + self.hip.N, dtype=torch.float64, generator=self.generator)
        return self._eps

    def push_hypers(self, jitter: float):
        """Hands the hyper-parameters to the library unless these very values are already there: a new set_hypers would make the library
        forget the preconditioner and the alpha of its last evaluation, which the predictive solve starts from."""
        ls, var, noise, mean = [t.detach() for t in self.hyper_tensors()]
        key = (ls.cpu().numpy().tobytes(), float(var), float(noise), float(mean), float(jitter))
        if key != self._pushed:
            self.hip.set_hypers(ls.cpu().numpy(), float(var), float(noise), float(mean), self._placeholder_Z, jitter)
            self._pushed = key


@dataclass
class Bounds:
    upper_bound: Tensor
    lower_bound: Tensor


_DEFAULT_JITTER = {"value": 1e-6}


def set_cholesky_jitter(value: float):
    _DEFAULT_JITTER["value"] = float(value)


def get_cholesky_jitter() -> float:
    return _DEFAULT_JITTER["value"]


class _Evaluation(torch.autograd.Function):
    """value(*inputs) with the analytic gradient from the GPU (row G of SURVEY 8a).  `evaluate(needs)` makes the library call at the model's
    current hyper-parameters, which `inputs` are, and returns (value, gradient dict or None, gradient of a trainable v or None); `needs`
    says which inputs want a gradient.  The inputs come in the order lengthscales, variance, noise, mean[, Z[, v]]."""

    @staticmethod
    def forward(ctx, evaluate, *inputs):
        value, ctx.grads, ctx.grad_v = evaluate(ctx.needs_input_grad[1:])
        ctx.with_v = len(inputs) > 5
        return torch.tensor(value, dtype=torch.float64)

    @staticmethod
    def backward(ctx, gout):
        g = ctx.grads
        if g is None:
            raise RuntimeError("gradient was not requested in forward")
        gout = gout.to(torch.float64)
        grads = [gout * (torch.from_numpy(g[key]) if key in ("lengthscales", "Z") else g[key])
                 for key in ("lengthscales", "variance", "noise", "mean", "Z") if key in g]
        if ctx.with_v:
            grads.append(None if ctx.grad_v is None else gout.to(ctx.grad_v.device) * ctx.grad_v)
        return (None, *grads)


class _Objective(nn.Module):
    """`Objective(model)(data)`: the model class's training objective through `_Evaluation`.  A subclass names the model class it takes
    (MODEL, and NOT_MODEL for the subclasses of it that it refuses) and makes the library call in `evaluate`.  `data` must be None or the
    model's own training set."""

    MODEL: type = GPR
    NOT_MODEL: tuple = ()
    EXPECTED = "GPR"

    def __init__(self, model):
        if not isinstance(model, self.MODEL) or isinstance(model, self.NOT_MODEL):
            raise ValueError(f"{self.EXPECTED} model expected in the constructor of the {self.__class__}")
        super().__init__()
        object.__setattr__(self, "model", model)  # not a sub-module: parameters stay owned by the model

    def inputs(self):
        return self.model.hyper_tensors()

    def evaluate(self, needs):
        raise NotImplementedError()

    def forward(self, data: Optional[Tuple[Tensor, Tensor]] = None, *params) -> Tensor:
        """The reference evaluates the bound on the `data` it is given (models.py:151-169); here the training set lives in the
        model's HIP context, so `data` must be None or that same training set: anything else (a subset, a held-out set) raises
        instead of silently returning the bound of the training data."""
        if data is not None:
            self.model.check_same_data(data)
        return _Evaluation.apply(self.evaluate, *self.inputs())


class LowerBoundCG(_Objective):
    """models.py:104-286.  `LowerBoundCG(model)(data)` returns the lower bound on the log marginal likelihood."""

    MODEL, EXPECTED = SGPR, "CGLB"  # models.py:112-113

    def __init__(self, model: SGPR, cg_opt: Optional[ConjugateGradient] = None, use_cache: bool = False,
                 cached_v_vec_initial: bool = False):
        super().__init__(model)
        if cg_opt is None:  # the model carries a tolerance only under the TF twin's config semantics (tensorflow/models.py:36-51)
            tol = getattr(model, "max_error", None)
            cg_opt = ConjugateGradient() if tol is None else ConjugateGradient(max_error=float(tol))
        self.cg_opt = cg_opt
        self._cached_v_vec = cached_v_vec_initial
        self._use_cache = use_cache
        self.last_bounds: Optional[Bounds] = None

    @property
    def cached_v_vec(self) -> bool:
        return self._cached_v_vec

    @cached_v_vec.setter
    def cached_v_vec(self, value: bool):
        self._cached_v_vec = value

    @property
    def likelihood(self):
        return self.model.likelihood

    @property
    def kernel(self):
        return self.model.covar_module.base_kernel

    @property
    def inducing_points(self) -> Tensor:
        return self.model.covar_module.inducing_points

    @property
    def noise(self) -> Tensor:
        return self.likelihood.noise.squeeze()

    def inputs(self):
        v_vec = self.model.v_vec
        return (*self.model.hyper_tensors(), v_vec if isinstance(v_vec, nn.Parameter) else None)

    def evaluate(self, needs):
        model, hip = self.model, self.model.hip
        model.push_hypers(get_cholesky_jitter())
        need_grad = any(needs)
        multi = getattr(model, "num_outputs", 1) > 1
        v = model.v_vec.detach() if multi else model.v_vec.detach().reshape(-1)   # [N, P] as it is; one output: the flat vector
        run_cg = not (self._use_cache and self.cached_v_vec)            # models.py:263
        if model.joint_optimization or model.vzero:                     # tensorflow/models.py:161-164: v0 is used as it stands
            run_cg = False
        cg = self.cg_opt
        if run_cg and multi and type(cg) is not ConjugateGradient:
            raise NotImplementedError("a plug-in solver is not available for more than one target column (the batched PCG runs in the library)")
        if run_cg and type(cg) is not ConjugateGradient:
            # foreign plug-in solver through the seam (models.py:266-271): cg_opt(A, b, v, precond)
            hip.setup()
            err = (hip.y - float(model.mean_module.constant)).reshape(-1, 1)
            new_v, stats = cg(KernelOperator(hip), err, model.v_vec, NystromPreconditioner(hip))
            model.cg_stats = stats
            model.v_vec.data.copy_(new_v.reshape(model.v_vec.shape))
            res = hip.objective_and_grad(v, False, with_grad=need_grad)
        else:
            res = hip.objective_and_grad(v, run_cg, cg.max_error, cg.max_cg_iter, cg.restart_cg_iter, with_grad=need_grad)
            if run_cg:
                model.cg_stats = ConjugateGradientStats(res.steps, torch.tensor(res.residual_error, dtype=torch.float64))
        if run_cg:
            self.cached_v_vec = self._use_cache                         # models.py:278
        self.last_bounds = Bounds(upper_bound=torch.tensor(-res.upper), lower_bound=torch.tensor(-res.lower))  # models.py:286
        model.last_bound = float(res.bound)  # value of the most recent evaluation (diagnostics / tests)
        grad_v = None
        if isinstance(model.v_vec, nn.Parameter) and needs[5]:          # joint optimisation: d bound / d v = K w - r, one more mat-vec
            grad_v = hip.objective_grad_v().reshape(model.v_vec.shape)
        return res.bound, res.grad, grad_v


class LowerBoundSGPR(_Objective):
    """`LowerBoundSGPR(model)(data)`: the collapsed bound of an SGPR / SGPRN2M model (tensorflow/models.py:353-413), the `elbo` of the TF
    twin: no v, no solve."""

    MODEL, NOT_MODEL, EXPECTED = SGPR, (CGLB,), "SGPR"

    def evaluate(self, needs):
        model = self.model
        model.push_hypers(get_cholesky_jitter())
        res = model.hip.objective_and_grad(model._zero_v, False, with_grad=any(needs))
        model.last_bound = float(res.bound)
        return res.bound, res.grad, None


class LogMarginalLikelihood(_Objective):
    """`LogMarginalLikelihood(model)(data)`: the exact log marginal likelihood of an ExactGPR model (gpflow GPR.log_marginal_likelihood)."""

    MODEL, EXPECTED = ExactGPR, "ExactGPR"

    def evaluate(self, needs):
        model = self.model
        model.push_hypers()
        res = model.hip.gpr_objective_and_grad(with_grad=any(needs))
        model.last_bound = float(res.lml)
        return res.lml, res.grad, None


class StochasticLogMarginalLikelihood(_Objective):
    """`StochasticLogMarginalLikelihood(model)(data)`: the iterative estimate of the log marginal likelihood of an IterGPR model, with the
    library's unbiased gradient estimate: the backward is NOT the derivative of the forward value (the log-determinant estimate and its
    gradient use the same probes in different estimators)."""

    MODEL, EXPECTED = IterGPR, "IterGPR"

    def evaluate(self, needs):
        model = self.model
        model.push_hypers(get_cholesky_jitter())
        res = model.hip.itergp_objective_and_grad(model.probes(), model.v_vec, model.max_error, model.max_cg_iter, model.lanczos_iter,
                                                  with_grad=any(needs))
        model.last_bound = float(res.lml)
        model.cg_stats = ConjugateGradientStats(steps=res.steps, residual_error=res.residual_error)
        return res.lml, res.grad, None


class _InputEvaluation(torch.autograd.Function):
    """value(x, *hypers) with the analytic gradients from the GPU: `_Evaluation` with the training inputs as one more differentiable argument.
    `evaluate(x, need_x, needs)` sets the model's inputs, makes the library call and returns (value, gradient dict or None, gx or None)."""

    @staticmethod
    def forward(ctx, evaluate, x, *inputs):
        value, ctx.grads, ctx.gx = evaluate(x, ctx.needs_input_grad[1], ctx.needs_input_grad[2:])
        ctx.x_like = (x.shape, x.dtype, x.device)
        return torch.tensor(value, dtype=torch.float64)

    @staticmethod
    def backward(ctx, gout):
        g = ctx.grads
        if g is None:
            raise RuntimeError("gradient was not requested in forward")
        gout = gout.to(torch.float64)
        shape, dtype, device = ctx.x_like
        gx = None if ctx.gx is None else (gout.to(ctx.gx.device) * ctx.gx).reshape(shape).to(device=device, dtype=dtype)
        grads = [gout * (torch.from_numpy(g[key]) if key in ("lengthscales", "Z") else g[key])
                 for key in ("lengthscales", "variance", "noise", "mean", "Z") if key in g]   # "Z": the classes with inducing points, as _Evaluation
        return (None, gx, *grads)


class _InputGradObjective(nn.Module):
    """`Objective(model)(x)`: the model class's training objective as a function of the training INPUTS as well - what a learned feature map in
    front of the kernel (deep kernel learning, input warping, latent inputs) back-propagates through.  `x` [N, d] on any device replaces the
    model's training inputs (`set_train_inputs`), the hyper-parameters are pushed, and one evaluation returns the scalar; its backward delivers
    the hyper-parameter gradients as the plain objective does, plus d value / d x to `x`, computed only when `x` requires grad."""

    MODEL: type = GPR
    EXPECTED = "GPR"

    def __init__(self, model):
        if not isinstance(model, self.MODEL):
            raise ValueError(f"{self.EXPECTED} model expected in the constructor of the {self.__class__}")
        super().__init__()
        object.__setattr__(self, "model", model)  # not a sub-module: parameters stay owned by the model

    def evaluate(self, x, need_x, needs):
        raise NotImplementedError()

    def forward(self, x: Tensor) -> Tensor:
        return _InputEvaluation.apply(self.evaluate, x, *self.model.hyper_tensors())


class InputGradLogMarginalLikelihood(_InputGradObjective):
    """`InputGradLogMarginalLikelihood(model)(x)`: the exact log marginal likelihood of an ExactGPR model at the training inputs `x`, differentiable
    in `x` and the hyper-parameters (fp64, one target column, up to 32 input dimensions)."""

    MODEL, EXPECTED = ExactGPR, "ExactGPR"

    def evaluate(self, x, need_x, needs):
        model = self.model
        model.set_train_inputs(x)
        model.push_hypers()
        res = model.hip.gpr_objective_and_grad(with_grad=need_x or any(needs), with_input_grad=need_x)
        model.last_bound = float(res.lml)
        return res.lml, res.grad, res.grad_x


class InputGradStochasticLogMarginalLikelihood(_InputGradObjective):
    """`InputGradStochasticLogMarginalLikelihood(model)(x)`: the iterative estimate of the log marginal likelihood of an IterGPR model at the
    training inputs `x`, with the library's unbiased gradient estimate with respect to the hyper-parameters AND `x`.  As for
    StochasticLogMarginalLikelihood, the backward is NOT the derivative of the forward value (the log-determinant estimate and its gradient use
    the same probes in different estimators): it is the estimator's gradient, in `x` as in the hyper-parameters.  `v_vec` stays as the warm start."""

    MODEL, EXPECTED = IterGPR, "IterGPR"

    def evaluate(self, x, need_x, needs):
        model = self.model
        model.set_train_inputs(x)
        model.push_hypers(get_cholesky_jitter())
        res = model.hip.itergp_objective_and_grad(model.probes(), model.v_vec, model.max_error, model.max_cg_iter, model.lanczos_iter,
                                                  with_grad=need_x or any(needs), with_input_grad=need_x)
        model.last_bound = float(res.lml)
        model.cg_stats = ConjugateGradientStats(steps=res.steps, residual_error=res.residual_error)
        return res.lml, res.grad, res.grad_x


class InputGradLowerBoundCG(_InputGradObjective):
    """`InputGradLowerBoundCG(model)(x)`: the CGLB bound (CGLB, CGLBNM2) at the training inputs `x`, differentiable in `x`, the hyper-parameters
    and Z: the exact derivative of the value at the v of the evaluation, v detached as LowerBoundCG has it.  `model.v_vec` is the warm start of the
    solve; `run_cg` follows the rules of LowerBoundCG.evaluate (`use_cache` / `cached_v_vec`, `vzero`).  fp64, one rank, one target column, up to
    32 input dimensions; a plug-in solver, `joint_optimization` and the N^2M log-det class are refused."""

    MODEL, EXPECTED = CGLB, "CGLB"

    def __init__(self, model: CGLB, cg_opt: Optional[ConjugateGradient] = None, use_cache: bool = False, cached_v_vec_initial: bool = False):
        super().__init__(model)
        if cg_opt is None:
            tol = getattr(model, "max_error", None)
            cg_opt = ConjugateGradient() if tol is None else ConjugateGradient(max_error=float(tol))
        if type(cg_opt) is not ConjugateGradient:
            raise NotImplementedError("a plug-in solver is not available with the training-input gradient (the solve runs in the library)")
        if model.joint_optimization and not model.vzero:
            raise NotImplementedError("joint optimisation of v is not available with the training-input gradient")
        if model.num_outputs > 1:
            raise NotImplementedError("the training-input gradient of the bound takes one target column")
        self.cg_opt = cg_opt
        self.cached_v_vec = cached_v_vec_initial
        self._use_cache = use_cache
        self.last_bounds: Optional[Bounds] = None

    def evaluate(self, x, need_x, needs):
        model, hip, cg = self.model, self.model.hip, self.cg_opt
        model.set_train_inputs(x)
        model.push_hypers(get_cholesky_jitter())
        run_cg = not (self._use_cache and self.cached_v_vec) and not model.vzero
        res = hip.objective_and_grad(model.v_vec.detach().reshape(-1), run_cg, cg.max_error, cg.max_cg_iter, cg.restart_cg_iter,
                                     with_grad=need_x or any(needs), with_input_grad=need_x)
        if run_cg:
            model.cg_stats = ConjugateGradientStats(res.steps, torch.tensor(res.residual_error, dtype=torch.float64))
            self.cached_v_vec = self._use_cache
        self.last_bounds = Bounds(upper_bound=torch.tensor(-res.upper), lower_bound=torch.tensor(-res.lower))
        model.last_bound = float(res.bound)
        return res.bound, res.grad, res.grad_x


class InputGradLowerBoundSGPR(_InputGradObjective):
    """`InputGradLowerBoundSGPR(model)(x)`: the collapsed bound of an SGPR model at the training inputs `x`, differentiable in `x`, the
    hyper-parameters and Z (fp64, up to 32 input dimensions; SGPRN2M is refused by the library)."""

    MODEL, EXPECTED = SGPR, "SGPR"

    def __init__(self, model: SGPR):
        if isinstance(model, CGLB):
            raise ValueError(f"SGPR model expected in the constructor of the {self.__class__}")
        super().__init__(model)

    def evaluate(self, x, need_x, needs):
        model = self.model
        model.set_train_inputs(x)
        model.push_hypers(get_cholesky_jitter())
        res = model.hip.objective_and_grad(model._zero_v, False, with_grad=need_x or any(needs), with_input_grad=need_x)
        model.last_bound = float(res.bound)
        return res.bound, res.grad, res.grad_x


def _refuse_full_cov(full_cov: bool):
    if full_cov:
        raise NotImplementedError("The predict_f method currently  supports only `full_cov=False` option")  # models.py:311-314


class PredictCG(LowerBoundCG):
    """models.py:289-354: posterior mean/variance with the CG-corrected SGPR predictor (tolerance 1e-3)."""

    def __init__(self, model: SGPR, cg_opt: Optional[ConjugateGradient] = None):
        cg_opt = ConjugateGradient(max_error=1e-3) if cg_opt is None else cg_opt
        super().__init__(model, cg_opt)
        self._v_vec = model.v_vec.detach().clone()
        self.cached = False

    @property
    def v_vec(self):
        return self._v_vec

    def clear_cache(self):
        self.v_vec.copy_(self.model.v_vec.detach().clone())
        self.cached = False

    def forward(self, xnew: Tensor, full_cov: bool = False, full_output_cov: bool = False) -> Tuple[Tensor, Tensor]:
        _refuse_full_cov(full_cov)
        model, hip = self.model, self.model.hip
        with torch.no_grad():
            self._solve()
            if getattr(model, "num_outputs", 1) > 1:
                f_mean, f_var = hip.predict_multi(self.v_vec, xnew)                    # f_mean [n_new, P]; one variance for all outputs
                return f_mean, f_var.reshape(-1, 1).repeat(1, f_mean.shape[1])         # tiled over the outputs (tensorflow/models.py:245)
            f_mean, f_var = hip.predict(self.v_vec.reshape(-1), xnew)                  # models.py:334-352
        return f_mean.reshape(-1, 1), f_var.reshape(-1, 1)

    def _solve(self):
        """The solve for v at the current hyper-parameters, once (until clear_cache)."""
        model, hip = self.model, self.model.hip
        with torch.no_grad():
            if not self.cached:
                model.push_hypers(get_cholesky_jitter())
                hip.setup()                                                            # models.py:327
                ls, var, noise, mean, Z = model.hyper_tensors()
                if getattr(model, "num_outputs", 1) > 1:   # P columns: the batched PCG of the library, one shared K_ff product per step
                    cg = self.cg_opt
                    if type(cg) is not ConjugateGradient:
                        raise NotImplementedError("a plug-in solver is not available for more than one target column")
                    new_v, _steps, _half, _cols = hip.pcg_multi(hip.y - float(mean), self.v_vec, cg.max_error, cg.max_cg_iter, cg.restart_cg_iter)
                else:
                    err = (hip.y - float(mean)).reshape(-1, 1)
                    new_v, _stats = self.cg_opt(KernelOperator(hip), err, self.v_vec, NystromPreconditioner(hip))  # :329
                self.v_vec.data.copy_(new_v.reshape(self.v_vec.shape))
                self.cached = True


class _Predict(nn.Module):
    """`Predict(model)(xnew)`: predict_f mean and variance, each [n_new, 1].  A subclass names the model class it takes (MODEL; None: any)
    and makes the library call in `mean_and_variance`."""

    MODEL: Optional[type] = None

    def __init__(self, model):
        if self.MODEL is not None and not isinstance(model, self.MODEL):
            raise ValueError(f"{self.MODEL.__name__} model expected in the constructor of the {self.__class__}")
        super().__init__()
        object.__setattr__(self, "model", model)

    def mean_and_variance(self, xnew):
        raise NotImplementedError()

    def forward(self, xnew: Tensor, full_cov: bool = False, full_output_cov: bool = False) -> Tuple[Tensor, Tensor]:
        _refuse_full_cov(full_cov)
        with torch.no_grad():
            f_mean, f_var = self.mean_and_variance(xnew)
        return f_mean.reshape(-1, 1), f_var.reshape(-1, 1)


class PredictSGPR(_Predict):
    """Titsias' predictive: PredictCG's formula (models.py:333-354) at v = 0, without a solve (cg_mean = 0, res = e)."""

    def __init__(self, model: SGPR):
        super().__init__(model)
        self.cached = False

    def mean_and_variance(self, xnew):
        model = self.model
        if not self.cached:
            model.push_hypers(get_cholesky_jitter())
            model.hip.setup()
            self.cached = True
        return model.hip.predict(model._zero_v, xnew)


class PredictGPR(_Predict):
    """predict_f of the exact model: mean c + K_*f K^-1 e, variance f - |L^-1 K_f*|^2.  The library keeps the factor of the last evaluation at
    the current hyper-parameters and factors first if there is none."""

    MODEL = ExactGPR

    def mean_and_variance(self, xnew):
        self.model.push_hypers()
        return self.model.hip.gpr_predict(xnew)


class PredictIterGPR(_Predict):
    """predict_f of the iterative model: mean c + K_*f alpha from one solve at `max_error` (1e-3 like PredictCG), warm-started at the alpha of
    the last evaluation, and the variances f - k_*^T K^-1 k_* by batched solves, 8 new points at a time: n_new / 8 solves per call.
    `var_rank` > 0 (None: the model's `pred_var_rank`): the variances from the library's Lanczos variance cache of that rank instead, built once
    per set of hyper-parameters and applied to every new point by one multi-column product (the reference's metrics run under
    gpytorch.settings.fast_pred_var(), pytorch/interface.py:582) - an upper bound of the exact variance that tightens with the rank."""

    MODEL = IterGPR

    def __init__(self, model: IterGPR, max_error: float = 1e-3, var_rank: Optional[int] = None):
        super().__init__(model)
        self.max_error = float(max_error)
        self.var_rank = int(model.pred_var_rank if var_rank is None else var_rank)

    def mean_and_variance(self, xnew):
        self.model.push_hypers(get_cholesky_jitter())
        if self.var_rank > 0:
            return self.model.hip.itergp_predict(xnew, self.max_error, self.model.max_cg_iter, var_rank=min(self.var_rank, self.model.hip.N, 1024))
        return self.model.hip.itergp_predict(xnew, self.max_error, self.model.max_cg_iter)


_FEATURE_NU = {_lib.RBF: None, _lib.MATERN32: 1.5, _lib.MATERN52: 2.5}   # by the library's kind; the names: hip_context.KINDS


def feature_draws(kind: str, d: int, F: int, generator: torch.Generator):
    """The raw draws behind `draw_features`, in its order: z [F, d] standard normal, chi2 [F] (one chi-square draw of 2 nu degrees of freedom
    per feature as the sum of 2 nu squared normals; None for RBF), u [F] uniform on [0, 1)."""
    nu = _FEATURE_NU[KINDS[kind]]
    z = torch.randn(F, d, dtype=torch.float64, generator=generator)
    chi2 = None if nu is None else torch.randn(F, int(2 * nu), dtype=torch.float64, generator=generator).square().sum(dim=1)
    u = torch.rand(F, dtype=torch.float64, generator=generator)
    return z, chi2, u


def draw_features(kind: str, d: int, F: int, generator: torch.Generator) -> Tuple[Tensor, Tensor]:
    """(omega [F, d], b [F]) of F random Fourier features of the unit-lengthscale kernel `kind` ("rbf" | "matern32" | "matern52"), from a
    torch.Generator on the CPU: omega from the kernel's spectral measure - standard normal rows for RBF; for Matern-nu the multivariate
    Student-t with 2 nu degrees of freedom, z sqrt(2 nu / chi2_{2 nu}) with one chi-square draw per feature - and b uniform on [0, 2 pi), so that
    (2 / F) sum_j cos(omega_j . x + b_j) cos(omega_j . x' + b_j) -> kappa(x, x')."""
    nu = _FEATURE_NU[KINDS[kind]]
    z, chi2, u = feature_draws(kind, d, F, generator)
    omega = z if nu is None else z * torch.sqrt(2.0 * nu / chi2).reshape(-1, 1)
    return omega, 2.0 * math.pi * u


class SampleIterGPR(nn.Module):
    """predict_f_samples of the iterative model: `SampleIterGPR(model)(xnew, num_samples)` -> [num_samples, n_new, 1] joint draws of the
    posterior of f at xnew by pathwise conditioning (cglb_itergp_sample): a random-Fourier-feature prior draw of `num_features` features,
    corrected through one batched solve at `max_error` with the class's preconditioner.  O(N) memory.  The draws are exact for the
    `num_features`-feature approximation of the prior (their mean is the exact predictive mean); the spread carries that approximation's
    O(1 / sqrt(num_features)) covariance error.  Frequencies, phases, weights and noise draws come from `model.generator`; with
    `fixed_features` the frequencies and phases are drawn once, here, and successive calls share that prior basis."""

    def __init__(self, model: IterGPR, num_features: int = 1024, max_error: float = 1e-3, fixed_features: bool = False):
        if not isinstance(model, IterGPR):
            raise ValueError(f"IterGPR model expected in the constructor of the {self.__class__}")
        super().__init__()
        object.__setattr__(self, "model", model)
        self.num_features, self.max_error = int(num_features), float(max_error)
        self.features = self._draw() if fixed_features else None

    def _draw(self):
        model = self.model
        return draw_features(model.covar_module.base_kernel.kind, model.hip.D, self.num_features, model.generator)

    def forward(self, xnew: Tensor, num_samples: int = 1) -> Tensor:
        model, S = self.model, int(num_samples)
        with torch.no_grad():
            omega, b = self._draw() if self.features is None else self.features
            W = torch.randn(S, self.num_features, dtype=torch.float64, generator=model.generator)
            eps = torch.randn(S, model.hip.N, dtype=torch.float64, generator=model.generator)
            model.push_hypers(get_cholesky_jitter())
            res = model.hip.itergp_sample(xnew, omega, b, W, eps, self.max_error, model.max_cg_iter)
        return res.samples.reshape(S, -1, 1)


class PredictGradIterGPR(nn.Module):
    """`PredictGradIterGPR(model)(xnew)` -> (mean [n, 1], dmean [n, d], var [n, 1], dvar [n, d]): predict_f of the iterative model and its
    gradients with respect to the new points (cglb_itergp_predict_grad).  The variances come from the Lanczos variance cache of rank `var_rank`
    (None: the model's `pred_var_rank`), built on demand as PredictIterGPR builds it; `dvar` is the exact gradient of that cache's variance
    (an upper bound of the exact variance), not of the exact variance.  Rank 0: `var` and `dvar` are None.
    Up to 32 input dimensions; `wide=True` sets the option "input_grad_mid" on the model's context, which opens 33 to 96 dimensions (fp64, the
    register-resident mid-width path) - without it such a model is refused."""

    def __init__(self, model: IterGPR, max_error: float = 1e-3, var_rank: Optional[int] = None, wide: bool = False):
        if not isinstance(model, IterGPR):
            raise ValueError(f"IterGPR model expected in the constructor of the {self.__class__}")
        super().__init__()
        object.__setattr__(self, "model", model)
        if wide:
            model.hip.set_option("input_grad_mid", 1)
        self.max_error = float(max_error)
        self.var_rank = int(model.pred_var_rank if var_rank is None else var_rank)

    def forward(self, xnew: Tensor):
        model, hip = self.model, self.model.hip
        with torch.no_grad():
            model.push_hypers(get_cholesky_jitter())
            rank = min(self.var_rank, hip.N, 1024)
            if rank > 0 and int(hip.get_stat("itergp_cache_request")) != rank:
                hip.itergp_var_cache(rank)
            mean, dmean, var, dvar = hip.itergp_predict_grad(xnew, self.max_error, model.max_cg_iter, with_var=rank > 0)
        return mean.reshape(-1, 1), dmean, None if var is None else var.reshape(-1, 1), dvar


class _PredictValues(torch.autograd.Function):
    """(mean, var) [n, 1] each of a gradient predictor with the library's gradients: backward contracts the two incoming gradients with the stored
    [n, d] blocks - the only arithmetic torch does."""

    @staticmethod
    def forward(ctx, predictor, x):
        mean, dmean, var, dvar = predictor.forward(x)
        ctx.save_for_backward(dmean, dvar)
        ctx.x_shape, ctx.x_device = x.shape, x.device
        return mean, var

    @staticmethod
    def backward(ctx, grad_mean, grad_var):
        dmean, dvar = ctx.saved_tensors
        g = grad_mean.to(dmean.device).reshape(-1, 1) * dmean + grad_var.to(dvar.device).reshape(-1, 1) * dvar
        return None, g.reshape(ctx.x_shape).to(ctx.x_device)


class _PredictGrad:
    """What the gradient predictors of the cglb / sgpr / gpr classes share: `forward(xnew)` -> (mean [n, 1], dmean [n, d], var [n, 1], dvar [n, d]),
    the gradients with respect to the new points; `mean_and_variance(xnew)` -> (mean, var), differentiable by autograd when `xnew.requires_grad`
    (one torch.autograd.Function whose backward contracts the incoming gradients with dmean and dvar), so any torch acquisition function
    differentiates through the library.
    Up to 32 input dimensions; `wide=True` sets the option "input_grad_mid" on the model's context, exactly as PredictGradIterGPR does, which opens
    33 to 96 dimensions (fp64, wide_reg on: the register-resident mid-width kernels) - without it such a model is refused as before."""

    @staticmethod
    def _open_wide(model, wide):
        if wide:
            model.hip.set_option("input_grad_mid", 1)

    @staticmethod
    def _refuse(model):
        name = type(model).__name__
        if getattr(model, "num_outputs", 1) > 1:
            raise NotImplementedError(f"the input gradients of {name} are not available for more than one target column (only CGLB takes [N, P] targets)")
        if getattr(model.hip, "world", 1) > 1:
            raise NotImplementedError(_ONE_RANK.format(name=f"the input gradients of {name}"))

    def value_and_grad(self, xnew):
        raise NotImplementedError()

    def forward(self, xnew: Tensor):
        with torch.no_grad():
            mean, dmean, var, dvar = self.value_and_grad(xnew.detach())
        return mean.reshape(-1, 1), dmean, var.reshape(-1, 1), dvar

    def mean_and_variance(self, xnew: Tensor):
        if isinstance(xnew, torch.Tensor) and xnew.requires_grad:
            return _PredictValues.apply(self, xnew)
        mean, _, var, _ = self.forward(xnew)
        return mean, var


class PredictGradCG(_PredictGrad, PredictCG):
    """`PredictGradCG(model)(xnew)`: PredictCG (its solve for v, cached until `clear_cache`) with the input gradients of mean and variance
    (cglb_predict_grad).  Takes CGLB, CGLBN2M and CGLBNM2; fp64, one rank, one target column, up to 32 input dimensions, 33 to 96 with
    `wide=True`."""

    def __init__(self, model: CGLB, cg_opt: Optional[ConjugateGradient] = None, wide: bool = False):
        if not isinstance(model, CGLB):
            raise ValueError(f"CGLB model expected in the constructor of the {self.__class__}")
        self._refuse(model)
        PredictCG.__init__(self, model, cg_opt)
        self._open_wide(model, wide)

    def value_and_grad(self, xnew):
        self._solve()
        return self.model.hip.predict_grad(self.v_vec.reshape(-1), xnew)


class PredictGradSGPR(_PredictGrad, nn.Module):
    """`PredictGradSGPR(model)(xnew)`: Titsias' predictive (PredictSGPR: v = 0, no solve) with the input gradients of mean and variance.  Takes
    SGPR and SGPRN2M; 33 to 96 input dimensions with `wide=True`."""

    def __init__(self, model: SGPR, wide: bool = False):
        if not isinstance(model, SGPR) or isinstance(model, CGLB):
            raise ValueError(f"SGPR model expected in the constructor of the {self.__class__}")
        self._refuse(model)
        nn.Module.__init__(self)
        object.__setattr__(self, "model", model)
        self._open_wide(model, wide)
        self.cached = False

    def value_and_grad(self, xnew):
        model = self.model
        if not self.cached:
            model.push_hypers(get_cholesky_jitter())
            model.hip.setup()
            self.cached = True
        return model.hip.predict_grad(model._zero_v, xnew)


class PredictGradGPR(_PredictGrad, nn.Module):
    """`PredictGradGPR(model)(xnew)`: predict_f of the exact model (PredictGPR) with the input gradients of mean and variance
    (cglb_gpr_predict_grad); this class's variance, and so its gradient, is exact.  33 to 96 input dimensions with `wide=True`."""

    def __init__(self, model: ExactGPR, wide: bool = False):
        if not isinstance(model, ExactGPR):
            raise ValueError(f"ExactGPR model expected in the constructor of the {self.__class__}")
        self._refuse(model)
        nn.Module.__init__(self)
        object.__setattr__(self, "model", model)
        self._open_wide(model, wide)

    def value_and_grad(self, xnew):
        self.model.push_hypers()
        return self.model.hip.gpr_predict_grad(xnew)


class _PathValues(torch.autograd.Function):
    """paths(x) with the library's gradient: backward contracts the incoming [S, n, 1] gradient with the stored [S, n, d] block."""

    @staticmethod
    def forward(ctx, paths, x):
        f, g = paths.value_and_grad(x)
        ctx.save_for_backward(g)
        ctx.x_shape, ctx.x_device = x.shape, x.device
        return f

    @staticmethod
    def backward(ctx, grad_f):
        (g,) = ctx.saved_tensors
        return None, (grad_f.to(g.device) * g).sum(dim=0).reshape(ctx.x_shape).to(ctx.x_device)


class PathsIterGPR(nn.Module):
    """`paths = PathsIterGPR(model, num_samples)`: `num_samples` posterior sample paths of the iterative model that are solved ONCE, here
    (cglb_itergp_paths_solve), and evaluated anywhere afterwards without a solve (cglb_itergp_paths_eval): `paths(x)` -> [S, n, 1],
    `paths.value_and_grad(x)` -> ([S, n, 1], [S, n, d]) with the gradients with respect to x.  When `x.requires_grad`, `paths(x)` is
    differentiable by autograd.  Frequencies, phases, weights and noise are drawn from `model.generator` in the order of
    SampleIterGPR.forward (fixed_features False): with the same seed the paths are the samples that class returns.  The paths belong to the
    hyper-parameters and targets they were solved at: evaluating after either changed raises RuntimeError.  Up to 32 input dimensions;
    `wide=True` sets the option "input_grad_mid" on the model's context before the solve, which opens 33 to 96 dimensions (fp64)."""

    def __init__(self, model: IterGPR, num_samples: int, num_features: int = 1024, max_error: float = 1e-3, wide: bool = False):
        if not isinstance(model, IterGPR):
            raise ValueError(f"IterGPR model expected in the constructor of the {self.__class__}")
        super().__init__()
        object.__setattr__(self, "model", model)
        if wide:
            model.hip.set_option("input_grad_mid", 1)
        self.num_samples, self.num_features, self.max_error = int(num_samples), int(num_features), float(max_error)
        S = self.num_samples
        with torch.no_grad():
            self.omega, self.b = draw_features(model.covar_module.base_kernel.kind, model.hip.D, self.num_features, model.generator)
            self.W = torch.randn(S, self.num_features, dtype=torch.float64, generator=model.generator)
            eps = torch.randn(S, model.hip.N, dtype=torch.float64, generator=model.generator)
            model.push_hypers(get_cholesky_jitter())
            res = model.hip.itergp_paths_solve(self.omega, self.b, self.W, eps, self.max_error, model.max_cg_iter)
        self.W = self.W.to(model.hip.device)
        self.solves, self.steps, self.residual_error = res.solves, res.steps, res.residual_error
        self._solved_at = self._state()

    def _state(self):
        model = self.model
        ls, var, noise, mean = [t.detach() for t in model.hyper_tensors()]
        return (ls.cpu().numpy().tobytes(), float(var), float(noise), float(mean), id(model.hip), model.hip.state_version)

    def _check(self):
        if self._state() != self._solved_at:
            raise RuntimeError("the sample paths were solved at other hyper-parameters or data: draw new paths (PathsIterGPR) after a change of either")

    def _eval(self, x, with_grad):
        self._check()
        with torch.no_grad():
            f, g = self.model.hip.itergp_paths_eval(x.detach(), self.omega, self.b, self.W, self.solves, with_grad=with_grad)
        return f.reshape(self.num_samples, -1, 1), g

    def value_and_grad(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        return self._eval(torch.as_tensor(x), True)

    def forward(self, x: Tensor) -> Tensor:
        x = torch.as_tensor(x)
        if x.requires_grad:
            return _PathValues.apply(self, x)
        return self._eval(x, False)[0]


class _PredictLogdensity:
    """Mixed in before a predictor: `forward((x, y))` is the log density of y under that predictor's predictive at x, summed over the outputs."""

    def forward(self, data: Tuple[Tensor, Tensor], full_cov: bool = False, full_output_cov: bool = False):
        if full_cov or full_output_cov:
            raise NotImplementedError(
                "The predict_log_density method currently supports only the argument values full_cov=False and full_output_cov=False")
        x, y = data
        f_mean, f_var = super().forward(x, full_cov=full_cov, full_output_cov=full_output_cov)
        return log_density(self.model, y, f_mean, f_var)


class PredictLogdensityCG(_PredictLogdensity, PredictCG):
    pass


class PredictLogdensityGPR(_PredictLogdensity, PredictGPR):
    pass


class PredictLogdensityIterGPR(_PredictLogdensity, PredictIterGPR):
    pass


def log_density(m, y, f_mean, f_var) -> Tensor:  # models.py:370-372
    noise = m.likelihood.noise.squeeze().detach().to(f_mean.device)
    y = torch.as_tensor(y, dtype=f_mean.dtype, device=f_mean.device)
    return gaussian(y, f_mean, f_var + noise).sum(axis=-1)


def gaussian(x, mu, var):  # models.py:375-379
    pi2 = math.log(2 * math.pi)
    x = x.reshape(*mu.shape)
    return -0.5 * (pi2 + torch.log(var) + (mu - x) ** 2 / var)
