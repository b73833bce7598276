"""Backend interface for the HIP path — mirror of cglb/backend/pytorch/interface.py restricted to what the CGLB
path needs: configure_backend, set_default_float/jitter, get_default_float(_str), create_kernel,
create_model (all five classes of SGPR_CONFIGS: cglb, cglbn2m, cglbnm2, sgpr, sgprn2m, and the exact `gpr` and iterative `itergp` classes of GPR_CONFIGS), model_parameters, optimize (SciPy L-BFGS-B, four-round schedule :445-543; `adam_<lr>` for itergp), save, load,
metrics_fn (:607-658).  gpytorch's own `exactgp` baseline / MultiDeviceKernel branches are out of scope and raise NotImplementedError,
like the reference's unregistered singledispatch defaults (:120-147).
"""
from __future__ import annotations

import json
import os
from contextlib import contextmanager
from dataclasses import asdict
from functools import singledispatch
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import jsonio, metric
from .callbacks import Logger
from .config import (CGLBConfig, CGLBN2MConfig, CGLBNM2Config, ExactGPConfig, GPRConfig, IterGPRConfig, KernelConfig, Matern32Config, Matern52Config, ModelConfig, SGPRConfig,
                     SGPRN2MConfig, SquaredExponentialConfig)
from .models import (CGLB, CGLBN2M, CGLBNM2, GPR, SGPR, SGPRN2M, BaseKernel, ExactGPR, GaussianLikelihood, InducingPointKernel, IterGPR,
                     LogMarginalLikelihood, LowerBoundCG, LowerBoundSGPR, PredictCG, PredictGPR, PredictIterGPR, PredictSGPR, ScaleKernel,
                     StochasticLogMarginalLikelihood, get_cholesky_jitter, log_density, set_cholesky_jitter)
from .optimizer import Scipy

__all__ = ["create_kernel", "create_model", "optimize", "save", "load", "metrics_fn"]

Tensor = torch.Tensor
Data = Tuple[np.ndarray, np.ndarray]

_STATE = {"dtype": torch.float64, "logdir": None, "config_semantics": "torch"}


def configure_backend(logdir: Optional[str] = None, keops: Optional[bool] = None, config_semantics: str = "torch", **kwargs):
    """interface.py:66-88.  `keops` is accepted and ignored: the implicit K_ff mat-vec is always the HIP kernel.
    config_semantics: "torch" (default) mirrors pytorch/interface.py:315-323, which ignores `max_error` / `joint_optimization` / `vzero`
    of CGLBConfig; "tf" consumes them like the TF twin's create_model (tensorflow/interface.py:244-258, models.py:31-51,161-164)."""
    assert logdir is not None
    if config_semantics not in ("torch", "tf"):
        raise ValueError("config_semantics must be 'torch' or 'tf'")
    _STATE["logdir"] = logdir
    _STATE["config_semantics"] = config_semantics
    if not torch.cuda.is_available():
        raise RuntimeError("the hip backend needs an MI355X (HIP device); there is no CPU fallback")


def set_default_jitter(jitter):  # interface.py:90-91
    set_cholesky_jitter(jitter)


def set_default_float(float_type: str) -> None:  # interface.py:94-104
    types = {"fp32": torch.float32, "float32": torch.float32, "fp64": torch.float64, "float64": torch.float64}
    if float_type not in types:
        raise NotImplementedError(f"Unknown float type {float_type}")
    _STATE["dtype"] = types[float_type]


def get_default_float_str() -> str:  # interface.py:107-113
    return {torch.float32: "fp32", torch.float64: "fp64"}[_STATE["dtype"]]


def get_default_float() -> np.dtype:  # interface.py:116-117
    return torch.tensor(1, dtype=_STATE["dtype"]).numpy().dtype


@singledispatch
def create_model(model_cfg: ModelConfig, data: Data):
    raise NotImplementedError()


@singledispatch
def create_kernel(cfg: KernelConfig, data: Data):
    raise NotImplementedError()


@singledispatch
def optimize(model: GPR, dataset, num_steps: int, logger: Logger, optimizer: str):
    raise NotImplementedError()


@singledispatch
def save(model: GPR, logdir: str):
    raise NotImplementedError()


@singledispatch
def load(model: GPR, filepath: str):
    raise NotImplementedError()


@singledispatch
def metrics_fn(model: GPR, dataset_bundle):
    raise NotImplementedError()


def model_parameters(model) -> Dict[str, np.ndarray]:
    """interface.py:150-178 — same keys."""
    kernel = model.covar_module
    params = {
        ".likelihood.variance": _numpy(model.likelihood.noise_covar.noise)[0],
        ".mean_function.c": _numpy(model.mean_module.constant),
    }
    if isinstance(kernel, InducingPointKernel):
        params.update({".inducing_variable.Z": _numpy(kernel.inducing_points)})
        kernel = kernel.base_kernel
    params.update({
        ".kernel.lengthscales": _numpy(kernel.base_kernel.lengthscale)[0, :],
        ".kernel.variance": _numpy(kernel.outputscale).squeeze(),
    })
    return params


def _make_kernel(kind: str, cfg, data: Data) -> ScaleKernel:
    params = cfg.params(data)
    lengthscales = np.asarray(params["lengthscales"], dtype=np.float64)
    base = BaseKernel(kind, ard_num_dims=len(lengthscales))
    base.lengthscale = lengthscales
    kernel = ScaleKernel(base)
    kernel.outputscale = params["variance"]
    return kernel


@create_kernel.register
def _create_kernel_m32(cfg: Matern32Config, data: Data):  # interface.py:220-230 (registered first: subclass of SE config)
    return _make_kernel("matern32", cfg, data)


@create_kernel.register
def _create_kernel_m52(cfg: Matern52Config, data: Data):  # beyond the reference (registered before its base, the SE config)
    return _make_kernel("matern52", cfg, data)


@create_kernel.register
def _create_kernel_se(cfg: SquaredExponentialConfig, data: Data):  # interface.py:207-217
    if isinstance(cfg, Matern32Config):
        return _make_kernel("matern32", cfg, data)
    if isinstance(cfg, Matern52Config):
        return _make_kernel("matern52", cfg, data)
    return _make_kernel("rbf", cfg, data)


def _kernel_numpy(kernel: ScaleKernel, x1, x2, full_cov: bool):
    """init_kernel_fn of interface.py:278-284 (numpy closed form; only used to pick the initial inducing points)."""
    x1 = np.asarray(x1, dtype=np.float64)
    var = float(kernel.outputscale.detach())
    if not full_cov:
        return np.full(x1.shape[0], var)
    ls = _numpy(kernel.base_kernel.lengthscale).reshape(-1)
    x2 = x1 if x2 is None else np.asarray(x2, dtype=np.float64)
    a, b = x1 / ls, x2 / ls
    d2 = np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)
    kind = kernel.base_kernel.kind
    if kind == "rbf":
        return var * np.exp(-0.5 * d2)
    if kind == "matern32":
        s = np.sqrt(3.0 * d2)
        return var * (1.0 + s) * np.exp(-s)
    if kind == "matern52":
        s = np.sqrt(5.0 * d2)
        return var * (1.0 + s + s * s / 3.0) * np.exp(-s)
    raise ValueError(f"no closed form for kernel kind {kind!r}")


class _InitKernel:
    """The init_kernel_fn callback of interface.py:278-284, plus the HIP implementation of the greedy selection it feeds
    (config.py:62-65 -> cglb_select_inducing): the O(N M^2) pivoted Cholesky runs on the GPU, not through this callback."""

    def __init__(self, kernel: ScaleKernel):
        self.kernel = kernel

    def __call__(self, x1, x2=None, full_cov: bool = False):
        return _kernel_numpy(self.kernel, x1, x2, full_cov)

    def select_inducing(self, X: np.ndarray, num_variables: int) -> np.ndarray:
        from ..hip_context import HipContext
        X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
        ctx = HipContext(X, np.zeros(X.shape[0]), num_variables, self.kernel.base_kernel.kind, dtype=_STATE["dtype"])
        try:
            ls = _numpy(self.kernel.base_kernel.lengthscale).reshape(-1)
            indices, _ = ctx.select_inducing(ls, float(self.kernel.outputscale.detach()))
        finally:
            ctx.close()
        return X[indices].copy()


def _likelihood_and_kernel(model_cfg: ModelConfig, data: Data, noise_lower_bound: float = 1e-6):
    likelihood = GaussianLikelihood(lower_bound=noise_lower_bound)
    likelihood.noise = model_cfg.params(data)["noise_variance"]
    return likelihood, create_kernel(model_cfg.kernel, data)


def _likelihood_and_kernel_for_sgpr(model_cfg: SGPRConfig, data: Data):
    """interface.py:263-301"""
    likelihood, base_kernel = _likelihood_and_kernel(model_cfg, data)
    inducing_variable = model_cfg.params(data)["inducing_variable"](_InitKernel(base_kernel))
    return likelihood, InducingPointKernel(base_kernel, inducing_variable)


# config class -> (model class, one rank only, takes max_error / joint_optimization / vzero under config_semantics="tf")
_INDUCING_POINT_CLASSES = {CGLBConfig: (CGLB, False, True), CGLBN2MConfig: (CGLBN2M, True, True), CGLBNM2Config: (CGLBNM2, True, True),
                           SGPRConfig: (SGPR, True, False), SGPRN2MConfig: (SGPRN2M, True, False)}


@create_model.register
def _create_model_sgpr(model_cfg: SGPRConfig, data: Data):
    """interface.py:315-323 for cglb; tensorflow/interface.py:216-292 builds the other four from the same config fields, on the same
    inducing-point initialisation.  Like the reference's torch path, max_error / joint_optimization / vzero of a CGLB config are not
    consumed here (the objective uses ConjugateGradient() defaults) unless the backend was configured with
    config_semantics="tf": the TF twin's create_model hands these to the model (tensorflow/interface.py:244-258).  Only cglb runs on more
    than one rank."""
    cls, one_rank, tf_extras = next(_INDUCING_POINT_CLASSES[c] for c in type(model_cfg).__mro__ if c in _INDUCING_POINT_CLASSES)
    if one_rank:
        _require_one_rank(cls.__name__.lower())
    likelihood, kernel = _likelihood_and_kernel_for_sgpr(model_cfg, data)
    extra = {}
    if tf_extras and _STATE["config_semantics"] == "tf":
        extra = dict(max_error=model_cfg.max_error, joint_optimization=model_cfg.joint_optimization, vzero=model_cfg.vzero)
    model = cls((np.asarray(data[0]), _targets(data[1])), likelihood, kernel, dtype=_STATE["dtype"], **extra)
    if not one_rank:
        _broadcast_parameters(model)
    return model


@create_model.register
def _create_model_gpr(model_cfg: GPRConfig, data: Data):
    """tensorflow/interface.py:200-206: noise 1.0, constant mean, the kernel of the kernel config; no inducing points.  One rank, fp64 (an fp32
    default float is refused with the library's message, which names `-t fp64`)."""
    _require_one_rank("gpr")
    likelihood, kernel = _likelihood_and_kernel(model_cfg, data)
    return ExactGPR((np.asarray(data[0]), _targets(data[1])), likelihood, kernel, dtype=_STATE["dtype"])


@create_model.register
def _create_model_exactgp(model_cfg: ExactGPConfig, data: Data):
    raise NotImplementedError("model class 'exactgp' (gpytorch's iterative exact-GP baseline, pytorch/interface.py:233-260) is out of scope here: "
                              "use 'gpr', the dense Cholesky exact GP")


@create_model.register
def _create_model_itergp(model_cfg: IterGPRConfig, data: Data):
    """The iterative exact GP in the library's own estimator (pytorch/interface.py:233-260 builds the reference's on gpytorch): the noise bound
    1e-4 of the reference's exactgp, constant mean, no inducing points.  One rank, fp64."""
    _require_one_rank("itergp")
    if _STATE["dtype"] != torch.float64:
        raise ValueError("model class 'itergp' needs fp64: run with -t fp64")
    likelihood, kernel = _likelihood_and_kernel(model_cfg, data, noise_lower_bound=1e-4)
    return IterGPR((np.asarray(data[0]), _targets(data[1])), likelihood, kernel, dtype=_STATE["dtype"], num_probes=model_cfg.num_probes,
                   prec_size=model_cfg.prec_size, max_error=model_cfg.max_error, max_cg_iter=model_cfg.max_cg_iter,
                   lanczos_iter=model_cfg.lanczos_iter, seed=model_cfg.seed, pred_var_rank=model_cfg.pred_var_rank)


def _targets(y) -> np.ndarray:
    """Targets as the models take them: [N, P] stays 2-D for P > 1, a single column (either shape) is the flat vector it always was."""
    y = np.asarray(y)
    return y if (y.ndim == 2 and y.shape[1] > 1) else y.reshape(-1)


def _targets_2d(y) -> np.ndarray:
    y = np.asarray(y)
    return y.reshape(y.shape[0], -1)


def _require_one_rank(name: str):
    """The bound variants run on one GPU: refused under a process group of more than one rank before any GPU work (the inducing-point
    initialisation included)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"model class {name!r} is not available on more than one rank (only cglb runs row-sharded): "
                                  f"run it as a single process")


def _broadcast_parameters(model: CGLB):
    """N ranks: every rank built the model from the same data and config (the greedy inducing-point selection is deterministic); the
    initial parameters are broadcast from rank 0 all the same, so that the replicas start from identical bits by construction."""
    ctx = model.hip
    if getattr(ctx, "world", 1) <= 1:
        return
    import torch.distributed as dist
    group = getattr(ctx, "group", None)
    src = dist.get_global_rank(group, 0) if group is not None else 0
    with torch.no_grad():
        for p in model.parameters():
            buf = p.detach().to(ctx.device).contiguous()
            dist.broadcast(buf, src=src, group=group)
            p.copy_(buf.to(p.device))


@contextmanager
def _narrow_host_pools():
    """The optimiser's host side is a handful of small vectors (M D + D + 3 numbers), all heavy work runs on the GPU.  With their default
    widths (one thread per visible core: 128 on a box that grants this process 16) the OpenMP / BLAS pools of torch and numpy spin between
    calls and starve the HIP runtime's own threads: at N = 57k, D = 27 kernel launches stalled for ~70 ms at a time and an evaluation took
    99 ms of wall time for 58 ms of GPU work (47 ms with narrow pools).  CGLB_HOST_THREADS overrides the width (default 4; 0 = leave alone)."""
    n = int(os.environ.get("CGLB_HOST_THREADS", "4"))
    if n <= 0:
        yield
        return
    prev = torch.get_num_threads()
    torch.set_num_threads(min(prev, n))
    try:
        try:
            from threadpoolctl import threadpool_info, threadpool_limits
        except Exception:  # pragma: no cover
            threadpool_limits = None
        if threadpool_limits is None:
            yield
        else:
            # only ever NARROW a pool: a launcher may have set OMP_NUM_THREADS=1 (torch.distributed.run does), and widening a BLAS pool
            # beyond the width it was initialised with crashed SciPy's L-BFGS-B core (SIGSEGV inside _lbfgsb.setulb on both ranks of the
            # first CLI run under torch.distributed.run, round 3)
            limits = {}
            for info in threadpool_info():
                api, cur = info.get("user_api"), int(info.get("num_threads") or 1)
                if api and cur > n:
                    limits[api] = n
            if limits:
                with threadpool_limits(limits=limits):
                    yield
            else:
                yield
    finally:
        torch.set_num_threads(prev)


@optimize.register
def _optimize_cglb(model: CGLB, dataset, num_steps: int, logger: Logger, optimize: str = "scipy"):
    with _narrow_host_pools():
        return _optimize_cglb_impl(model, dataset, num_steps, logger, optimize)


def _assert_ranks_agree(model: CGLB, what: str):
    """N ranks each run the reference's single-process optimiser on what must be identical (loss, gradient) sequences: the loss of the
    last evaluation and a checksum of the parameters are all-gathered once per round; a rank that drifted raises on EVERY rank (all
    see the same gathered numbers), instead of the job running on with replicas that no longer describe one model."""
    ctx = getattr(model, "hip", None)
    if getattr(ctx, "world", 1) <= 1:
        return
    import torch.distributed as dist
    digest = 0.0
    for p in model.parameters():
        digest += float(p.detach().double().abs().sum())
    mine = torch.tensor([float(model.last_bound), digest], dtype=torch.float64, device=ctx.device)
    group = getattr(ctx, "group", None)
    if group is None and getattr(ctx, "comm", None) is not None:
        group = ctx.comm.group
    gathered = [torch.empty_like(mine) for _ in range(ctx.world)]
    dist.all_gather(gathered, mine, group=group)
    vals = torch.stack(gathered).cpu().numpy()
    if not (np.all(vals[:, 0] == vals[0, 0]) and np.all(vals[:, 1] == vals[0, 1])):
        raise RuntimeError(f"ranks disagree {what}: (bound, parameter checksum) per rank = {vals.tolist()}")


def _warm_up(evaluate, params, logger: Logger):
    """interface.py:494-501: one evaluation with its gradient outside the recording and the clock, which starts here."""
    with logger.no_recording():
        torch.autograd.grad(evaluate(), params)
        if torch.cuda.is_available():                       # :499-501
            torch.cuda.synchronize()
    logger.timer.reset()
    logger.timer.start()


def _lbfgs_rounds(model: GPR, objective, num_steps: int, logger: Logger, on_evaluation=None, on_step=None):
    """interface.py:445-543: warm-up evaluation outside the clock, then up to four L-BFGS-B rounds on loss = -objective, the last two
    without the inducing points (if the model has any).  `on_evaluation` runs after every evaluation, `on_step` before the logger at
    every accepted step."""
    lbfgs = Scipy()

    def closure() -> Tensor:
        loss = -objective(None)
        if on_evaluation is not None:
            on_evaluation()
        return loss

    def step_callback(*args):
        if on_step is not None:
            on_step()
        logger(*args)

    params = list(model.parameters())
    _warm_up(closure, params, logger)
    results, remaining = [], num_steps
    for round_id in range(4):                               # :507-543
        if remaining <= 0:
            break
        ips = getattr(model.covar_module, "inducing_points", None)
        if round_id == 2 and ips is not None:
            params = [p for p in model.parameters() if p is not ips]
        result = lbfgs.minimize(closure, params, options=dict(maxiter=remaining, ftol=0.0, gtol=0.0, disp=False), step_callback=step_callback)
        remaining -= result.nit
        results.append(result)
        _assert_ranks_agree(model, f"after optimisation round {round_id}")
    return results


def _optimize_cglb_impl(model: CGLB, dataset, num_steps: int, logger: Logger, optimize: str = "scipy"):
    """The rounds of `_lbfgs_rounds` with the CG statistics logged at every evaluation and the cached v dropped at every step (:476-481)."""
    _require_scipy(model, optimize)
    lower_bound = LowerBoundCG(model)

    def log_cg_stats():
        stats = model.cg_stats                              # None when CG never ran (TF-twin vzero / joint_optimization)
        # steps-per-feval / residual_error-per-feval (:476); without CG the TF optimize logs zeros (tensorflow/interface.py:296-337)
        logger.log_for_feval(**(asdict(stats) if stats is not None else dict(steps=0, residual_error=0.0)))

    def drop_cached_v():
        lower_bound.cached_v_vec = False                    # :480

    return _lbfgs_rounds(model, lower_bound, num_steps, logger, log_cg_stats, drop_cached_v)


@optimize.register
def _optimize_sgpr(model: SGPR, dataset, num_steps: int, logger: Logger, optimize: str = "scipy"):
    """The same L-BFGS-B rounds as CGLB without the v bookkeeping (the TF backend trains every class this way,
    tensorflow/interface.py:296-337)."""
    _require_scipy(model, optimize)
    with _narrow_host_pools():
        return _lbfgs_rounds(model, LowerBoundSGPR(model), num_steps, logger)


@optimize.register
def _optimize_gpr(model: ExactGPR, dataset, num_steps: int, logger: Logger, optimize: str = "scipy"):
    """The same rounds on loss = -lml; there are no inducing points to leave out of the later rounds."""
    _require_scipy(model, optimize)
    with _narrow_host_pools():
        return _lbfgs_rounds(model, LogMarginalLikelihood(model), num_steps, logger)


def _require_scipy(model, optimizer: str):
    """The classes with an exact gradient train with L-BFGS-B only; `adam_<lr>` belongs to the iterative class."""
    if optimizer != "scipy":
        raise ValueError(f"optimizer {optimizer!r} is not available for {type(model).__name__}: this class trains with 'scipy' (L-BFGS-B); "
                         f"'adam_<lr>' is the optimizer of model class 'itergp' (gpr -m itergp)")


def adam_learning_rate(optimizer: str) -> float:
    """The learning rate of an `adam_<lr>` optimizer name (pytorch/interface.py:561-604 parses the same form); ValueError otherwise."""
    name, _, lr = str(optimizer).partition("_")
    try:
        value = float(lr)
    except ValueError:
        value = -1.0
    if name != "adam" or not value > 0.0:
        raise ValueError(f"optimizer {optimizer!r}: expected adam_<learning rate>, e.g. adam_0.1")
    return value


@optimize.register
def _optimize_itergp(model: IterGPR, dataset, num_steps: int, logger: Logger, optimize: str = "adam_0.1"):
    """`num_steps` Adam steps on the full training set with fresh probes at every step - the last phase of the reference's exactgp training
    (pytorch/interface.py:561-604); its L-BFGS and subset phases are out of scope.  L-BFGS-B is refused: it needs gradients that are the
    derivative of the value it is given, and this class returns an unbiased gradient estimate next to a separately estimated value."""
    if optimize == "scipy":
        raise ValueError("model class 'itergp' cannot be trained with -o scipy: its gradient is a stochastic estimate and not the derivative of "
                         "the returned value, which the L-BFGS-B line search assumes; use -o adam_<lr>, e.g. adam_0.1")
    lr = adam_learning_rate(optimize)
    with _narrow_host_pools():
        lml = StochasticLogMarginalLikelihood(model)
        params = list(model.parameters())
        adam = torch.optim.Adam(params, lr=lr)
        _warm_up(lambda: -lml(None), params, logger)
        losses = []
        for step in range(num_steps):
            adam.zero_grad()
            loss = -lml(None)
            loss.backward()
            stats = model.cg_stats
            logger.log_for_feval(steps=stats.steps, residual_error=stats.residual_error)
            adam.step()
            losses.append(float(loss.detach()))
            logger(step)
        return losses


@save.register
def _save(model: GPR, logdir: str):  # interface.py:546-551: json_tricks.dump(model_parameters(model)) -> same encoding (jsonio.py)
    os.makedirs(logdir, exist_ok=True)
    params = model_parameters(model)
    with open(Path(logdir, "model.json"), "w") as file:
        jsonio.dump(params, file)


def _load_hypers(model: GPR, kernel: ScaleKernel, filepath: str) -> dict:
    """The entries every model class has, assigned from a model.json written by `save`; returns all of them."""
    params = jsonio.load(filepath)   # decodes the __ndarray__ objects json_tricks / `save` write; plain lists work too
    model.likelihood.noise_covar._noise.set(params[".likelihood.variance"], exact=True)   # exact: the values `save` wrote, bit for bit
    with torch.no_grad():
        model.mean_module.constant.copy_(torch.as_tensor(np.asarray(params[".mean_function.c"]), dtype=torch.float64).reshape(()))
    kernel.base_kernel._lengthscale.set(params[".kernel.lengthscales"], exact=True)
    kernel._outputscale.set(params[".kernel.variance"], exact=True)
    return params


@load.register
def _load(model: GPR, filepath: str):
    """Reads a model.json written by `save` (the reference's torch `load` expects a state_dict and is asymmetric
    with its own `save`; here the pair round-trips)."""
    params = _load_hypers(model, model.covar_module.base_kernel, filepath)
    with torch.no_grad():
        model.covar_module.inducing_points.copy_(torch.as_tensor(np.asarray(params[".inducing_variable.Z"]), dtype=torch.float64))
    return model


@load.register(ExactGPR)
@load.register(IterGPR)   # the same module tree and parameter keys
def _load_gpr(model: GPR, filepath: str):
    """Parameters saved by ANY model class (cli.py:166-181 evaluates the exact metrics at hyper-parameters a sparse model was trained to): an
    inducing-point entry is ignored."""
    _load_hypers(model, model.covar_module, filepath)
    return model


def _rmse_and_lpd_fn(model: GPR, predictor_cls, dataset_bundle, max_batch: int = int(1e6)):
    """interface.py:627-655: rmse / nlpd of `predictor_cls(model)` on the train and test sets, over all outputs, predicted in one pass of
    at most `max_batch` rows at a time."""
    train, test = dataset_bundle
    x_full = np.concatenate([np.asarray(train[0]), np.asarray(test[0])], axis=0)
    y_full = np.concatenate([_targets_2d(train[1]), _targets_2d(test[1])], axis=0)  # [n, P]
    n = np.asarray(train[0]).shape[0]

    def error_and_logdensity():
        predict_f = predictor_cls(model)
        lpds, errs = [], []
        with torch.no_grad():
            for i in range(0, int(x_full.shape[0]), max_batch):
                f_mean, f_var = predict_f(torch.as_tensor(x_full[i: i + max_batch]))
                y_batch = torch.as_tensor(y_full[i: i + max_batch], dtype=f_mean.dtype, device=f_mean.device)
                lpds.append(_numpy(log_density(model, y_batch, f_mean, f_var)))
                errs.append(_numpy(y_batch - f_mean))
        err, lpd = np.concatenate(errs, axis=0), np.concatenate(lpds, axis=0)
        return (err[:n], err[n:]), (lpd[:n], lpd[n:])

    return metric.rmse_and_lpd_fn(error_and_logdensity)


@metrics_fn.register
def _compute_metrics_gpr(model: ExactGPR, dataset_bundle):
    """tensorflow/interface.py:386-395: lml, loss = -lml, and rmse / nlpd of the exact predictive on the train and test sets."""

    def gpr_metrics():
        with torch.no_grad():
            lml = _numpy(LogMarginalLikelihood(model)(None))
        return dict(lml=lml, loss=-lml)

    rmse_lpd_metrics = _rmse_and_lpd_fn(model, PredictGPR, dataset_bundle)
    return lambda: metric.call_metric_fns(gpr_metrics, rmse_lpd_metrics)


@metrics_fn.register
def _compute_metrics_itergp(model: IterGPR, dataset_bundle):
    """The metrics of the exact class from the iterative estimator: lml (one draw of the probes), loss = -lml, and rmse / nlpd of the predictive
    on the train and test sets; the variances cost (n_train + n_test) / 8 batched solves, or with the model's `pred_var_rank` > 0 that many
    Lanczos steps once per call and one multi-column product over all points (pytorch/interface.py:582 runs under fast_pred_var())."""

    def itergp_metrics():
        with torch.no_grad():
            lml = _numpy(StochasticLogMarginalLikelihood(model)(None))
        stats = model.cg_stats
        return {"lml": lml, "loss": -lml, "cg/steps": stats.steps, "cg/error": stats.residual_error}

    rmse_lpd_metrics = _rmse_and_lpd_fn(model, PredictIterGPR, dataset_bundle)
    return lambda: metric.call_metric_fns(itergp_metrics, rmse_lpd_metrics)


@metrics_fn.register
def _compute_metrics_cglb(model: CGLB, dataset_bundle):
    """interface.py:607-658"""

    def cglb_cg_params():
        if model.cg_stats is not None:
            return {"cg/steps": _numpy(model.cg_stats.steps), "cg/error": _numpy(model.cg_stats.residual_error)}
        return {}

    def cglb_metrics():
        with torch.no_grad():
            lower_bound = LowerBoundCG(model, use_cache=True, cached_v_vec_initial=True)  # no CG: reuse model.v_vec (:619-625)
            loss = -lower_bound(None)
            return dict(loss=_numpy(loss))

    rmse_lpd_metrics = _rmse_and_lpd_fn(model, PredictCG, dataset_bundle)
    return lambda: metric.call_metric_fns(cglb_cg_params, cglb_metrics, rmse_lpd_metrics)


@metrics_fn.register
def _compute_metrics_sgpr(model: SGPR, dataset_bundle):
    """tensorflow/interface.py:395-408 without titsias_upper_bound: loss = -elbo, and rmse / nlpd of the Titsias predictive."""

    def sgpr_metrics():
        with torch.no_grad():
            elbo = _numpy(LowerBoundSGPR(model)(None))
        return dict(elbo=elbo, loss=-elbo)

    rmse_lpd_metrics = _rmse_and_lpd_fn(model, PredictSGPR, dataset_bundle)
    return lambda: metric.call_metric_fns(sgpr_metrics, rmse_lpd_metrics)


def _numpy(tensor) -> np.ndarray:
    if isinstance(tensor, torch.Tensor):
        return tensor.detach().cpu().numpy()
    return np.asarray(tensor)
