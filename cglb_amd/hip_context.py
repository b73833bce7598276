"""Thin object wrapper over the C ABI: one HipContext = one cglb_ctx = one GPU row shard.

torch is used for device memory and streams only; every computation is a call into libcglb_hip.so.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int, c_void_p
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

KINDS = {"rbf": _lib.RBF, "SquaredExponential": _lib.RBF, "matern32": _lib.MATERN32, "Matern32": _lib.MATERN32,
         "mat32": _lib.MATERN32, "matern52": _lib.MATERN52, "Matern52": _lib.MATERN52, "mat52": _lib.MATERN52,
         0: _lib.RBF, 1: _lib.MATERN32, 2: _lib.MATERN52}


def grad_len(D: int, M: int) -> int:
    return D + 3 + M * D


@dataclass
class ObjectiveResult:
    bound: float
    lower: float
    upper: float
    logdet: float
    steps: int
    residual_error: float
    grad: Optional[dict]  # constrained-space gradient of `bound`
    grad_x: Optional[torch.Tensor] = None  # d bound / d X at fixed v, device [N, D] (with_input_grad)


@dataclass
class GPRResult:
    lml: float      # log marginal likelihood = quad + logdet - N/2 log 2 pi
    quad: float     # -1/2 e^T K^-1 e
    logdet: float   # -sum log diag chol(K) = -1/2 log|K|
    grad: Optional[dict]  # d lml / d {lengthscales, variance, noise, mean}
    grad_x: Optional[torch.Tensor] = None  # d lml / d X, device [N, D] (with_input_grad)


@dataclass
class IterGPResult:
    lml: float        # quad + logdet - N/2 log 2 pi
    quad: float       # -1/2 e^T alpha
    logdet: float     # -1/2 log|K|, the stochastic Lanczos estimate
    logdet_P: float   # log|P| of the preconditioner
    steps: int
    residual_error: float
    grad: Optional[dict]  # the unbiased gradient estimate {lengthscales, variance, noise, mean}: not the derivative of `lml`
    grad_x: Optional[torch.Tensor] = None  # the same estimator's gradient with respect to the training inputs, device [N, D] (with_input_grad)


@dataclass
class IterGPSamples:
    samples: torch.Tensor           # [S, n_new] posterior function samples, sample s contiguous
    steps: int                      # iterations of the batched solve
    residual_error: float           # 1/2 sum_s r_s^T P^-1 r_s at its end
    solves: Optional[torch.Tensor]  # [S, N] U_s = K^-1 (e - Phi(X) w_s - sqrt(noise) eps_s) when asked for


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def unpack_grad(g: np.ndarray, D: int, M: int = 0) -> dict:
    """The dict of a packed constrained-space gradient [lengthscales (D), variance, noise, mean, Z (M * D)]; no "Z" entry for M = 0."""
    grad = {"lengthscales": g[:D].copy(), "variance": float(g[D]), "noise": float(g[D + 1]), "mean": float(g[D + 2])}
    if M:
        grad["Z"] = g[D + 3:].reshape(M, D).copy()
    return grad


def check_v_inout(v_inout: torch.Tensor, ctx):
    """ValueError unless v_inout is what the library reads and writes in place: a contiguous device vector of length N in the context dtype."""
    if v_inout.device != ctx.device or v_inout.dtype != ctx.dtype or v_inout.numel() != ctx.N or not v_inout.is_contiguous():
        raise ValueError("v_inout must be a contiguous device vector of length N in the context dtype")


class HipContext:
    def __init__(self, X, y, num_inducing: int, kind, dtype: torch.dtype = torch.float64, device: Optional[torch.device] = None,
                 row_range: Optional[Tuple[int, int]] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("cglb_amd needs a HIP device (MI355X); there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dtype = dtype
        self.kind = KINDS[kind]
        X = torch.as_tensor(X, dtype=dtype).reshape(len(X), -1).contiguous()
        y = torch.as_tensor(y, dtype=dtype)
        self.N, self.D = int(X.shape[0]), int(X.shape[1])
        # targets: [N] or [N, P]; one column (either shape) is the single-output model, P > 1 goes through cglb_set_targets below
        y = y.reshape(self.N, -1) if (y.dim() == 2 and y.shape[0] == self.N and y.shape[1] > 1) else y.reshape(-1)
        if y.shape[0] != self.N:
            raise ValueError("X and y disagree on the number of rows")
        self.P = 1
        self.M = int(num_inducing)
        self.r0, self.r1 = (0, self.N) if row_range is None else (int(row_range[0]), int(row_range[1]))
        self.nloc = self.r1 - self.r0
        self._ctx = c_void_p()
        self.state_version = 0   # counts set_hypers / set_targets: the events after which the library's alpha, preconditioner and variance cache are void
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            rc = self.lib.cglb_ctx_create(byref(self._ctx), self.N, self.r0, self.r1, self.D, self.M,
                                          _lib.F64 if dtype == torch.float64 else _lib.F32, self.kind,
                                          self.device.index or 0, c_void_p(stream))
        _lib.check(rc, None)
        Xd, yd = X.to(self.device), y.to(self.device)
        y0 = yd if yd.dim() == 1 else yd[:, 0].contiguous()
        _lib.check(self.lib.cglb_set_data(self._ctx, _ptr(Xd), _ptr(y0)), self._ctx)
        torch.cuda.synchronize(self.device)
        self.y = yd
        if yd.dim() == 2:
            self.set_targets(yd)

    # -- lifetime ------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.lib.cglb_ctx_destroy(self._ctx)
            self._ctx = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -------------------------------------------------------------------------------------
    def _dev(self, t, n=None) -> torch.Tensor:
        t = torch.as_tensor(t, dtype=self.dtype, device=self.device).reshape(-1).contiguous()
        if n is not None and t.numel() != n:
            raise ValueError(f"expected a vector of length {n}, got {t.numel()}")
        return t

    def empty(self, n) -> torch.Tensor:
        return torch.empty(n, dtype=self.dtype, device=self.device)

    def _xnew(self, xnew) -> torch.Tensor:
        return torch.as_tensor(xnew, dtype=self.dtype).reshape(-1, self.D).contiguous().to(self.device)

    def _ls(self, lengthscales) -> np.ndarray:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (self.D,)))

    def set_option(self, name: str, value: int):
        _lib.check(self.lib.cglb_set_option(self._ctx, name.encode(), int(value)), self._ctx)

    # -- hypers / common terms -----------------------------------------------------------------------
    def set_hypers(self, lengthscales, variance, noise, mean, Z, jitter=1e-6):
        ls = self._ls(lengthscales)
        Zd = torch.as_tensor(Z, dtype=self.dtype).reshape(self.M, self.D).contiguous().to(self.device)
        rc = self.lib.cglb_set_hypers(self._ctx, ls.ctypes.data_as(ctypes.POINTER(c_double)), float(variance), float(noise),
                                      float(mean), _ptr(Zd), float(jitter))
        _lib.check(rc, self._ctx)
        torch.cuda.synchronize(self.device)
        self.noise = float(noise)
        self.state_version += 1

    def setup(self):
        _lib.check(self.lib.cglb_setup(self._ctx), self._ctx)

    def setup_local(self):
        _lib.check(self.lib.cglb_shard_setup_local(self._ctx), self._ctx)

    def aat_tensor(self) -> torch.Tensor:
        """Zero-copy view of the library's partial A A^T buffer (for the all-reduce between setup phases)."""
        ptr = self.lib.cglb_aat_buffer(self._ctx)
        return _wrap_device_pointer(ptr, (self.M * self.M,), self.dtype, self.device)

    def setup_finish(self):
        _lib.check(self.lib.cglb_shard_setup_finish(self._ctx), self._ctx)

    def logdet(self) -> float:
        out = c_double()
        _lib.check(self.lib.cglb_logdet(self._ctx, byref(out)), self._ctx)
        return out.value

    def get_matrix(self, which: str) -> torch.Tensor:
        idx = {"A": 0, "L": 1, "LB": 2, "alpha": 3}[which]   # "alpha": the stored solve [N] of the iterative exact-GP class
        shape = (self.M, self.nloc) if idx == 0 else ((self.N,) if idx == 3 else (self.M, self.M))
        out = torch.empty(shape, dtype=self.dtype, device=self.device)
        _lib.check(self.lib.cglb_get_matrix(self._ctx, idx, _ptr(out)), self._ctx)
        return out

    # -- operator / preconditioner / solver ----------------------------------------------------------
    def matvec(self, p_full: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        p = self._dev(p_full, self.N)
        out = self.empty(self.nloc) if out is None else out
        _lib.check(self.lib.cglb_matvec(self._ctx, _ptr(p), _ptr(out)), self._ctx)
        return out

    def cross_matvec(self, xnew, v_full) -> torch.Tensor:
        xn = self._xnew(xnew)
        v = self._dev(v_full, self.N)
        out = self.empty(xn.shape[0])
        _lib.check(self.lib.cglb_cross_matvec(self._ctx, _ptr(xn), xn.shape[0], _ptr(v), _ptr(out)), self._ctx)
        return out

    def precond(self, r) -> Tuple[torch.Tensor, float]:
        r = self._dev(r, self.N)
        z = self.empty(self.N)
        rz = c_double()
        _lib.check(self.lib.cglb_precond_apply(self._ctx, _ptr(r), _ptr(z), byref(rz)), self._ctx)
        return z, rz.value

    def pcg(self, b, v0, max_error=1.0, max_cg_iter=100, restart_cg_iter=40) -> Tuple[torch.Tensor, int, float]:
        b = self._dev(b, self.N)
        v = self._dev(v0, self.N).clone()  # the reference clones v (conjugate_gradient.py:55)
        steps, half = c_int(), c_double()
        rc = self.lib.cglb_pcg_solve(self._ctx, _ptr(b), _ptr(v), float(max_error), int(max_cg_iter), int(restart_cg_iter),
                                     byref(steps), byref(half))
        _lib.check(rc, self._ctx)
        return v, steps.value, half.value

    # -- multi-output targets: tensors are [N, P] on this side, [P, N] (column b contiguous) in the library ----------------
    def _cols(self, t, s=None) -> torch.Tensor:
        """[N, S] (or [N]) tensor -> contiguous [S, N] device tensor (always a copy for S > 1)."""
        t = torch.as_tensor(t, dtype=self.dtype, device=self.device)
        t = t.reshape(self.N, -1)
        if s is not None and t.shape[1] != s:
            raise ValueError(f"expected {s} columns, got {t.shape[1]}")
        return t.t().contiguous()

    def set_targets(self, Y):
        """Replace the targets by Y [N, P] (or [N]): cglb_set_targets."""
        Yt = self._cols(Y)
        _lib.check(self.lib.cglb_set_targets(self._ctx, _ptr(Yt), int(Yt.shape[0])), self._ctx)
        self.P = int(Yt.shape[0])
        self.y = Yt[0].clone() if self.P == 1 else Yt.t().contiguous()
        self.state_version += 1

    def matmat(self, V) -> torch.Tensor:
        """(K_ff + noise I) V for V [N, S]: one evaluation of every kernel value for up to 8 columns (cglb_matmat)."""
        Vt = self._cols(V)
        out = torch.empty((Vt.shape[0], self.nloc), dtype=self.dtype, device=self.device)
        _lib.check(self.lib.cglb_matmat(self._ctx, _ptr(Vt), int(Vt.shape[0]), _ptr(out)), self._ctx)
        return out.t().contiguous()

    def pcg_multi(self, B, V0, max_error=1.0, max_cg_iter=100, restart_cg_iter=40):
        """Batched PCG on B, V0 [N, S]: returns (V [N, S], steps, 1/2 sum_b r_b^T P r_b, per-column terms [S])."""
        Bt = self._cols(B)
        Vt = self._cols(V0, Bt.shape[0]).clone()
        s = int(Bt.shape[0])
        steps, half = c_int(), c_double()
        cols = np.empty(s, dtype=np.float64)
        rc = self.lib.cglb_pcg_solve_multi(self._ctx, _ptr(Bt), _ptr(Vt), s, float(max_error), int(max_cg_iter), int(restart_cg_iter),
                                           byref(steps), byref(half), cols.ctypes.data_as(ctypes.POINTER(c_double)))
        _lib.check(rc, self._ctx)
        return Vt.t().contiguous(), steps.value, half.value, cols

    def predict_multi(self, V, xnew) -> Tuple[torch.Tensor, torch.Tensor]:
        """f_mean [n_new, P] for the P target columns and the shared f_var [n_new] (cglb_predict_multi)."""
        xn = self._xnew(xnew)
        Vt = self._cols(V, self.P)
        mean = torch.empty((self.P, xn.shape[0]), dtype=self.dtype, device=self.device)
        var = self.empty(xn.shape[0])
        _lib.check(self.lib.cglb_predict_multi(self._ctx, _ptr(Vt), _ptr(xn), xn.shape[0], _ptr(mean), _ptr(var)), self._ctx)
        return mean.t().contiguous(), var

    def time_matmat(self, s: int, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_matmat(self._ctx, int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def objective_and_grad(self, v_inout: torch.Tensor, run_cg=True, max_error=1.0, max_cg_iter=100, restart_cg_iter=40,
                           with_grad=True, with_input_grad=False) -> ObjectiveResult:
        """v_inout (device, length N; [N, P] for P > 1 target columns) is the persistent warm-start vector: updated in place when run_cg.
        with_input_grad: `grad_x`, the exact derivative of `bound` with respect to the raw training inputs at fixed v, besides (needs with_grad;
        cglb_objective_and_grad_x: fp64, one rank, one target column, up to 32 input dimensions, not the N^2M log-det classes); everything else is
        bitwise what it is without."""
        if v_inout.device != self.device or v_inout.dtype != self.dtype:
            raise ValueError("v_inout must be a device tensor in the context dtype")
        if with_input_grad and not with_grad:
            raise ValueError("with_input_grad needs with_grad: the input gradient is formed from the adjoints of the hyper-parameter gradient")
        if with_input_grad:
            if self.P == 1:   # P > 1: the library refuses before it reads v
                check_v_inout(v_inout, self)
            out4 = (c_double * 4)()
            g = np.empty(grad_len(self.D, self.M), dtype=np.float64)
            steps, half = c_int(), c_double()
            gx = self._nan_rows()
            rc = self.lib.cglb_objective_and_grad_x(self._ctx, _ptr(v_inout), int(bool(run_cg)), float(max_error), int(max_cg_iter), int(restart_cg_iter),
                                                    out4, g.ctypes.data_as(ctypes.POINTER(c_double)), byref(steps), byref(half), _ptr(gx))
            _lib.check(rc, self._ctx)
            return ObjectiveResult(out4[0], out4[1], out4[2], out4[3], steps.value, half.value, self.unpack_grad(g), gx)
        if self.P > 1:
            if tuple(v_inout.shape) != (self.N, self.P):
                raise ValueError("v_inout must be a device tensor of shape [N, P] in the context dtype")
            v, entry = v_inout.t().contiguous(), self.lib.cglb_objective_and_grad_multi  # the library's layout: column b contiguous
        else:
            check_v_inout(v_inout, self)
            v, entry = v_inout, self.lib.cglb_objective_and_grad
        out4 = (c_double * 4)()
        g = np.empty(grad_len(self.D, self.M), dtype=np.float64) if with_grad else None
        steps, half = c_int(), c_double()
        rc = entry(self._ctx, _ptr(v), int(bool(run_cg)), float(max_error), int(max_cg_iter), int(restart_cg_iter), out4,
                   g.ctypes.data_as(ctypes.POINTER(c_double)) if with_grad else None, byref(steps), byref(half))
        _lib.check(rc, self._ctx)
        if self.P > 1 and run_cg:
            v_inout.copy_(v.t())  # the persistent warm start, in the caller's layout
        return ObjectiveResult(out4[0], out4[1], out4[2], out4[3], steps.value, half.value, self.unpack_grad(g) if with_grad else None)

    def objective_grad_v(self) -> torch.Tensor:
        """d bound / d v at the v of the evaluation just made (TF twin's joint optimisation of v, tensorflow/models.py:161-164)."""
        out = self.empty(self.N)
        _lib.check(self.lib.cglb_objective_grad_v(self._ctx, _ptr(out)), self._ctx)
        return out

    def unpack_grad(self, g: np.ndarray) -> dict:
        return unpack_grad(g, self.D, self.M)

    def select_inducing(self, lengthscales, variance, jitter=1e-12, return_Z=False):
        """Greedy conditional-variance choice of the M inducing points under the given (initial) kernel - config.py:55-65.
        Returns (indices int64 [min(M, N)], remaining trace) and, if asked, the device tensor Z = X[indices].
        Must be followed by set_hypers before any other call."""
        ls = self._ls(lengthscales)
        msel = min(self.M, self.N)
        idx = np.empty(msel, dtype=np.int64)
        Z = torch.empty((msel, self.D), dtype=self.dtype, device=self.device) if return_Z else None
        trace = c_double()
        rc = self.lib.cglb_select_inducing(self._ctx, ls.ctypes.data_as(ctypes.POINTER(c_double)), float(variance), float(jitter),
                                           idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _ptr(Z), byref(trace))
        _lib.check(rc, self._ctx)
        return (idx, trace.value, Z) if return_Z else (idx, trace.value)

    def predict(self, v_full, xnew) -> Tuple[torch.Tensor, torch.Tensor]:
        xn = self._xnew(xnew)
        v = self._dev(v_full, self.N)
        mean, var = self.empty(xn.shape[0]), self.empty(xn.shape[0])
        _lib.check(self.lib.cglb_predict(self._ctx, _ptr(v), _ptr(xn), xn.shape[0], _ptr(mean), _ptr(var)), self._ctx)
        return mean, var

    # -- exact GPR (cglb_gpr_*): dense Cholesky marginal likelihood, fp64, one rank, one target column; num_inducing is a placeholder ----
    def gpr_set_hypers(self, lengthscales, variance, noise, mean):
        ls = self._ls(lengthscales)
        rc = self.lib.cglb_gpr_set_hypers(self._ctx, ls.ctypes.data_as(ctypes.POINTER(c_double)), float(variance), float(noise), float(mean))
        _lib.check(rc, self._ctx)

    def gpr_objective_and_grad(self, with_grad=True, with_input_grad=False) -> GPRResult:
        """with_input_grad: `grad_x`, d lml / d X with respect to the raw training inputs, besides (needs with_grad)."""
        if with_input_grad and not with_grad:
            raise ValueError("with_input_grad needs with_grad: the input gradient is formed from the inverse the hyper-parameter gradient computes")
        out3 = (c_double * 3)()
        g = np.empty(self.D + 3, dtype=np.float64) if with_grad else None
        gp = g.ctypes.data_as(ctypes.POINTER(c_double)) if with_grad else None
        gx = self._nan_rows() if with_input_grad else None
        if with_input_grad:
            rc = self.lib.cglb_gpr_objective_and_grad_x(self._ctx, out3, gp, _ptr(gx))
        else:
            rc = self.lib.cglb_gpr_objective_and_grad(self._ctx, out3, gp)
        _lib.check(rc, self._ctx)
        return GPRResult(out3[0], out3[1], out3[2], None if g is None else unpack_grad(g, self.D), gx)

    def gpr_predict(self, xnew) -> Tuple[torch.Tensor, torch.Tensor]:
        """predict_f mean and variance at xnew [n_new, D] from the factor of the last evaluation (factored first if there is none)."""
        xn = self._xnew(xnew)
        mean, var = self.empty(xn.shape[0]), self.empty(xn.shape[0])
        _lib.check(self.lib.cglb_gpr_predict(self._ctx, _ptr(xn), xn.shape[0], _ptr(mean), _ptr(var)), self._ctx)
        return mean, var

    # -- iterative exact GP (cglb_itergp_*): batched CG with Lanczos log-det, fp64, one rank, one target column; num_inducing is the rank of
    #    the pivoted-Cholesky preconditioner, re-selected at every evaluation ----
    def itergp_objective_and_grad(self, eps, v_inout: torch.Tensor, max_error=1.0, max_cg_iter=1000, lanczos_iter=20, with_grad=True,
                                  with_input_grad=False) -> IterGPResult:
        """eps [t, M + N]: the probes' standard-normal draws (the library draws none).  v_inout (device, length N) is the persistent warm start of
        the data column, updated in place.  with_input_grad: `grad_x`, the estimator's gradient with respect to the raw training inputs, from one
        further pass over the vectors of the kernel gradient (needs with_grad); everything else is bitwise what it is without."""
        check_v_inout(v_inout, self)
        if with_input_grad and not with_grad:
            raise ValueError("with_input_grad needs with_grad: the input gradient is formed from the vectors of the hyper-parameter gradient")
        e = torch.as_tensor(eps, dtype=torch.float64).reshape(-1, self.M + self.N).contiguous().to(self.device)
        out4 = (c_double * 4)()
        g = np.empty(self.D + 3, dtype=np.float64) if with_grad else None
        gp = g.ctypes.data_as(ctypes.POINTER(c_double)) if with_grad else None
        steps, half = c_int(), c_double()
        gx = self._nan_rows() if with_input_grad else None
        if with_input_grad:
            rc = self.lib.cglb_itergp_objective_and_grad_x(self._ctx, _ptr(e), int(e.shape[0]), _ptr(v_inout), float(max_error), int(max_cg_iter),
                                                           int(lanczos_iter), out4, gp, byref(steps), byref(half), _ptr(gx))
        else:
            rc = self.lib.cglb_itergp_objective_and_grad(self._ctx, _ptr(e), int(e.shape[0]), _ptr(v_inout), float(max_error), int(max_cg_iter),
                                                         int(lanczos_iter), out4, gp, byref(steps), byref(half))
        _lib.check(rc, self._ctx)
        self._itergp_shape = (steps.value, 1 + int(e.shape[0]))
        return IterGPResult(out4[0], out4[1], out4[2], out4[3], steps.value, half.value, None if g is None else unpack_grad(g, self.D), gx)

    def itergp_coefficients(self) -> Tuple[np.ndarray, np.ndarray]:
        """(rz [steps + 1, 1 + t], pAp [steps, 1 + t]) of the last itergp_objective_and_grad."""
        steps, s = self._itergp_shape
        rz, pap = np.empty((steps + 1, s)), np.empty((steps, s))
        rc = self.lib.cglb_itergp_get_coefficients(self._ctx, rz.ctypes.data_as(ctypes.POINTER(c_double)), pap.ctypes.data_as(ctypes.POINTER(c_double)))
        _lib.check(rc, self._ctx)
        return rz, pap

    def itergp_predict(self, xnew, max_error=1e-3, max_cg_iter=1000, var_rank=0) -> Tuple[torch.Tensor, torch.Tensor]:
        """predict_f mean and variance at xnew [n_new, D]: one solve for alpha and n_new / 8 batched solves for the variances.  var_rank > 0:
        the variances from the Lanczos variance cache of that rank instead (built first when there is no valid one of that rank) - an upper
        bound of the exact variance that tightens with the rank."""
        xn = self._xnew(xnew)
        mean, var = self.empty(xn.shape[0]), self.empty(xn.shape[0])
        if var_rank and int(var_rank) > 0:
            if int(self.get_stat("itergp_cache_request")) != int(var_rank):
                self.itergp_var_cache(int(var_rank))
            rc = self.lib.cglb_itergp_predict_cached(self._ctx, _ptr(xn), xn.shape[0], float(max_error), int(max_cg_iter), _ptr(mean), _ptr(var))
        else:
            rc = self.lib.cglb_itergp_predict(self._ctx, _ptr(xn), xn.shape[0], float(max_error), int(max_cg_iter), _ptr(mean), _ptr(var))
        _lib.check(rc, self._ctx)
        return mean, var

    def itergp_var_cache(self, rank: int) -> int:
        """Builds the Lanczos variance cache (K^-1 ~ R R^T, `rank` Lanczos steps started at y - mean) at the current data and hyper-parameters;
        returns the number of columns J <= rank (smaller when the Krylov space closed early)."""
        out = c_int()
        _lib.check(self.lib.cglb_itergp_var_cache(self._ctx, int(rank), byref(out)), self._ctx)
        return out.value

    def itergp_predict_cached(self, xnew, max_error=1e-3, max_cg_iter=1000) -> Tuple[torch.Tensor, torch.Tensor]:
        """cglb_itergp_predict_cached as it is: RuntimeError without a valid cache."""
        xn = self._xnew(xnew)
        mean, var = self.empty(xn.shape[0]), self.empty(xn.shape[0])
        rc = self.lib.cglb_itergp_predict_cached(self._ctx, _ptr(xn), xn.shape[0], float(max_error), int(max_cg_iter), _ptr(mean), _ptr(var))
        _lib.check(rc, self._ctx)
        return mean, var

    def cross_matmat(self, xnew, V, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """variance kappa(xnew, X) V for V [N, S]: [n_new, S], one evaluation of every kernel value per group of 8 columns (cglb_cross_matmat).
        `out`: a contiguous device tensor [n_new, S] to write into."""
        xn = self._xnew(xnew)
        Vt = self._cols(V)
        if out is None:
            out = torch.empty((xn.shape[0], Vt.shape[0]), dtype=self.dtype, device=self.device)
        elif out.device != self.device or out.dtype != self.dtype or tuple(out.shape) != (xn.shape[0], Vt.shape[0]) or not out.is_contiguous():
            raise ValueError("out must be a contiguous device tensor [n_new, S] in the context dtype")
        _lib.check(self.lib.cglb_cross_matmat(self._ctx, _ptr(xn), xn.shape[0], _ptr(Vt), int(Vt.shape[0]), _ptr(out)), self._ctx)
        return out

    def time_cross_matmat(self, n_new: int, s: int, reps: int) -> float:
        """ms per product with s > 0 columns at the first n_new training rows; s < 0: |s| single cross mat-vecs on the same operands."""
        ms = c_double()
        _lib.check(self.lib.cglb_time_cross_matmat(self._ctx, int(n_new), int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def _features(self, omega, phase, W):
        om = torch.as_tensor(omega, dtype=self.dtype).reshape(-1, self.D).contiguous().to(self.device)
        ph = torch.as_tensor(phase, dtype=self.dtype).reshape(-1).contiguous().to(self.device)
        Wt = torch.as_tensor(W, dtype=self.dtype).to(self.device)
        Wt = Wt.reshape(-1, om.shape[0]).contiguous()
        if ph.shape[0] != om.shape[0] or om.shape[0] < 1 or Wt.shape[0] < 1:
            raise ValueError("omega [F, D], phase [F] and W [S, F] must agree on F >= 1")
        return om, ph, Wt

    def feature_matmat(self, x, omega, phase, W, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sqrt(2 variance / F) sum_j W[s, j] cos(omega_j . (x_i - c) / l + phase_j) at the rows x [n_rows, D] (None: the training rows) for
        omega [F, D], phase [F], W [S, F]: [n_rows, S], every cosine evaluated once per group of 8 columns (cglb_feature_matmat).
        `out`: a contiguous device tensor [n_rows, S] to write into."""
        xr = None if x is None else self._xnew(x)
        n = self.N if xr is None else xr.shape[0]
        om, ph, Wt = self._features(omega, phase, W)
        if out is None:
            out = torch.empty((n, Wt.shape[0]), dtype=self.dtype, device=self.device)
        elif out.device != self.device or out.dtype != self.dtype or tuple(out.shape) != (n, Wt.shape[0]) or not out.is_contiguous():
            raise ValueError("out must be a contiguous device tensor [n_rows, S] in the context dtype")
        rc = self.lib.cglb_feature_matmat(self._ctx, _ptr(xr), n, _ptr(om), _ptr(ph), _ptr(Wt), int(om.shape[0]), int(Wt.shape[0]), _ptr(out))
        _lib.check(rc, self._ctx)
        return out

    def time_feature_matmat(self, n_rows: int, f: int, s: int, reps: int) -> float:
        """ms per feature product of f features and s columns at the first n_rows training rows."""
        ms = c_double()
        _lib.check(self.lib.cglb_time_feature_matmat(self._ctx, int(n_rows), int(f), int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def itergp_sample(self, xnew, omega, phase, W, eps, max_error=1e-3, max_cg_iter=1000, return_solves=False) -> IterGPSamples:
        """Pathwise posterior samples at xnew [n_new, D] (cglb_itergp_sample): omega [F, D], phase [F], W [S, F] and eps [S, N] are the
        caller's draws (the library draws none).  Sample s is f_s = mean + Phi(xnew) w_s + K_*f K^-1 (y - mean - Phi(X) w_s - sqrt(noise) eps_s)."""
        xn = self._xnew(xnew)
        om, ph, Wt = self._features(omega, phase, W)
        S = int(Wt.shape[0])
        e = torch.as_tensor(eps, dtype=self.dtype).reshape(S, self.N).contiguous().to(self.device)
        f = torch.empty((S, xn.shape[0]), dtype=self.dtype, device=self.device)
        U = torch.empty((S, self.N), dtype=self.dtype, device=self.device) if return_solves else None
        steps, half = c_int(), c_double()
        rc = self.lib.cglb_itergp_sample(self._ctx, _ptr(xn), xn.shape[0], _ptr(om), _ptr(ph), _ptr(Wt), _ptr(e), int(om.shape[0]), S, float(max_error),
                                         int(max_cg_iter), _ptr(f), _ptr(U), byref(steps), byref(half))
        _lib.check(rc, self._ctx)
        return IterGPSamples(f, steps.value, half.value, U)

    # -- input gradients of predictive and sample paths (cglb_*_grad_matmat, cglb_itergp_predict_grad, cglb_itergp_paths_*): with respect to the
    #    raw coordinates of the new points; the scope of itergp_predict, up to 32 input dimensions.  set_option("input_grad_mid", 1) opens
    #    every one of them at 33 to 96 dimensions (fp64, wide_reg on; get_stat("input_grad_native") tells) ----
    def _out(self, out, shape, what):
        if out is None:
            return torch.empty(shape, dtype=self.dtype, device=self.device)
        if out.device != self.device or out.dtype != self.dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
            raise ValueError(f"{what} must be a contiguous device tensor {list(shape)} in the context dtype")
        return out

    def cross_grad_matmat(self, xnew, V, out: Optional[torch.Tensor] = None, gout: Optional[torch.Tensor] = None, with_value=True):
        """(variance kappa(xnew, X) V [n_new, S] or None, its gradient in xnew [n_new, S, D]) for V [N, S], one evaluation of every pair for both
        (cglb_cross_grad_matmat).  `out`, `gout`: contiguous device tensors to write into; with_value False: the gradient alone."""
        xn = self._xnew(xnew)
        Vt = self._cols(V)
        n, S = xn.shape[0], int(Vt.shape[0])
        out = self._out(out, (n, S), "out") if with_value else None
        gout = self._out(gout, (n, S, self.D), "gout")
        _lib.check(self.lib.cglb_cross_grad_matmat(self._ctx, _ptr(xn), n, _ptr(Vt), S, _ptr(out), _ptr(gout)), self._ctx)
        return out, gout

    def time_cross_grad_matmat(self, n_new: int, s: int, reps: int) -> float:
        """ms per value-and-gradient product with s columns at the first n_new training rows (the operands of time_cross_matmat)."""
        ms = c_double()
        _lib.check(self.lib.cglb_time_cross_grad_matmat(self._ctx, int(n_new), int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def feature_grad_matmat(self, x, omega, phase, W, out: Optional[torch.Tensor] = None, gout: Optional[torch.Tensor] = None, with_value=True):
        """(the feature product of feature_matmat [n_rows, S] or None, its gradient in x [n_rows, S, D]): one phase and one range reduction per
        (row, feature) for cosine and sine (cglb_feature_grad_matmat)."""
        xr = None if x is None else self._xnew(x)
        n = self.N if xr is None else xr.shape[0]
        om, ph, Wt = self._features(omega, phase, W)
        S = int(Wt.shape[0])
        out = self._out(out, (n, S), "out") if with_value else None
        gout = self._out(gout, (n, S, self.D), "gout")
        rc = self.lib.cglb_feature_grad_matmat(self._ctx, _ptr(xr), n, _ptr(om), _ptr(ph), _ptr(Wt), int(om.shape[0]), S, _ptr(out), _ptr(gout))
        _lib.check(rc, self._ctx)
        return out, gout

    def time_feature_grad_matmat(self, n_rows: int, f: int, s: int, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_feature_grad_matmat(self._ctx, int(n_rows), int(f), int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def itergp_predict_grad(self, xnew, max_error=1e-3, max_cg_iter=1000, with_var=True):
        """(mean [n], dmean [n, D], var [n] or None, dvar [n, D] or None) at xnew (cglb_itergp_predict_grad).  with_var needs a valid variance
        cache (itergp_var_cache): var is the cache's variance and dvar its exact gradient - not the gradient of the exact variance."""
        xn = self._xnew(xnew)
        n = xn.shape[0]
        mean, dmean = self.empty(n), torch.empty((n, self.D), dtype=self.dtype, device=self.device)
        var = self.empty(n) if with_var else None
        dvar = torch.empty((n, self.D), dtype=self.dtype, device=self.device) if with_var else None
        rc = self.lib.cglb_itergp_predict_grad(self._ctx, _ptr(xn), n, float(max_error), int(max_cg_iter), _ptr(mean), _ptr(dmean), _ptr(var), _ptr(dvar))
        _lib.check(rc, self._ctx)
        return mean, dmean, var, dvar

    # -- input gradients of the CGLB / SGPR / exact-GP predictive (cglb_cross_grad_weighted, cglb_predict_grad, cglb_gpr_predict_grad): up to 32 input
    #    dimensions; set_option("input_grad_mid", 1) opens them at 33 to 96 (fp64, wide_reg on; get_stat("predict_grad_native") tells) ----
    def cross_grad_weighted(self, xnew, u=None, Wt=None, point_set="train", out_u=None, gout_u=None, out_w=None, gout_w=None,
                            with_value=True, with_grad=True):
        """Row-weighted value and input gradient of the cross product against the training inputs (point_set "train") or the inducing points
        ("inducing"): (out_u [n], gout_u [n, D], out_w [n], gout_w [n, D]) for the shared weight u [n_pts] and / or the per-point weights
        Wt [n_pts, ldw >= n] (new-point index fastest; the columns from n on are never used); the outputs of an absent weight are None
        (cglb_cross_grad_weighted).  `out_*`, `gout_*`: contiguous device tensors to write into; with_value / with_grad False: that half of the
        outputs is not computed."""
        if point_set not in ("train", "inducing"):
            raise ValueError("point_set is 'train' or 'inducing'")
        xn = self._xnew(xnew)
        n, npts = xn.shape[0], (self.N if point_set == "train" else self.M)
        ut = None if u is None else self._dev(u, npts)
        wt, ldw = None, 0
        if Wt is not None:
            wt = torch.as_tensor(Wt, dtype=self.dtype, device=self.device)
            if wt.dim() != 2 or wt.shape[0] != npts or wt.shape[1] < n:
                raise ValueError(f"Wt must be [{npts}, ldw >= {n}]")
            wt = wt.contiguous()
            ldw = int(wt.shape[1])
        for name, t, w in (("out_u", out_u, ut), ("gout_u", gout_u, ut), ("out_w", out_w, wt), ("gout_w", gout_w, wt)):
            if t is not None and w is None:
                raise ValueError(f"{name} was given without its weight")
        res = []
        for w, o, g, names in ((ut, out_u, gout_u, ("out_u", "gout_u")), (wt, out_w, gout_w, ("out_w", "gout_w"))):
            res.append(self._out(o, (n,), names[0]) if (w is not None and with_value) else None)
            res.append(self._out(g, (n, self.D), names[1]) if (w is not None and with_grad) else None)
        rc = self.lib.cglb_cross_grad_weighted(self._ctx, 0 if point_set == "train" else 1, _ptr(xn), n, _ptr(ut), _ptr(wt), ldw,
                                               _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3]))
        _lib.check(rc, self._ctx)
        return tuple(res)

    def _predict_grad_outs(self, n, with_var, f_mean, g_mean, f_var, g_var):
        if not with_var and (f_var is not None or g_var is not None):
            raise ValueError("f_var / g_var were given with with_var False")
        return (self._out(f_mean, (n,), "f_mean"), self._out(g_mean, (n, self.D), "g_mean"),
                self._out(f_var, (n,), "f_var") if with_var else None, self._out(g_var, (n, self.D), "g_var") if with_var else None)

    def predict_grad(self, v_full, xnew, with_var=True, f_mean=None, g_mean=None, f_var=None, g_var=None):
        """(mean [n], dmean [n, D], var [n] or None, dvar [n, D] or None) of the CGLB / SGPR predictive at xnew, the gradients with respect to
        the new points (cglb_predict_grad); mean and var are bitwise those of `predict`."""
        xn = self._xnew(xnew)
        v = self._dev(v_full, self.N)
        outs = self._predict_grad_outs(xn.shape[0], with_var, f_mean, g_mean, f_var, g_var)
        _lib.check(self.lib.cglb_predict_grad(self._ctx, _ptr(v), _ptr(xn), xn.shape[0], *[_ptr(t) for t in outs]), self._ctx)
        return outs

    def gpr_predict_grad(self, xnew, with_var=True, f_mean=None, g_mean=None, f_var=None, g_var=None):
        """(mean [n], dmean [n, D], var [n] or None, dvar [n, D] or None) of the exact-GP predictive at xnew (cglb_gpr_predict_grad); mean and
        var are bitwise those of `gpr_predict`."""
        xn = self._xnew(xnew)
        outs = self._predict_grad_outs(xn.shape[0], with_var, f_mean, g_mean, f_var, g_var)
        _lib.check(self.lib.cglb_gpr_predict_grad(self._ctx, _ptr(xn), xn.shape[0], *[_ptr(t) for t in outs]), self._ctx)
        return outs

    def time_predict_grad(self, n_new: int, with_grad: bool, reps: int) -> float:
        """ms per `predict` (with_grad False) or `predict_grad` call at the first n_new training rows and v = 0."""
        ms = c_double()
        _lib.check(self.lib.cglb_time_predict_grad(self._ctx, int(n_new), int(bool(with_grad)), int(reps), byref(ms)), self._ctx)
        return ms.value

    def itergp_paths_solve(self, omega, phase, W, eps, max_error=1e-3, max_cg_iter=1000) -> IterGPSamples:
        """The solves U [S, N] of S sample paths (cglb_itergp_paths_solve: the first half of itergp_sample); `samples` is None."""
        om, ph, Wt = self._features(omega, phase, W)
        S = int(Wt.shape[0])
        e = torch.as_tensor(eps, dtype=self.dtype).reshape(S, self.N).contiguous().to(self.device)
        U = torch.empty((S, self.N), dtype=self.dtype, device=self.device)
        steps, half = c_int(), c_double()
        rc = self.lib.cglb_itergp_paths_solve(self._ctx, _ptr(om), _ptr(ph), _ptr(Wt), _ptr(e), int(om.shape[0]), S, float(max_error), int(max_cg_iter),
                                              _ptr(U), byref(steps), byref(half))
        _lib.check(rc, self._ctx)
        return IterGPSamples(None, steps.value, half.value, U)

    def itergp_paths_eval(self, xnew, omega, phase, W, U, with_grad=False):
        """(f [S, n_new], df [S, n_new, D] or None) of the paths with solves U [S, N] at xnew, without a solve (cglb_itergp_paths_eval).  Without
        gradients the values are bitwise those of itergp_sample."""
        xn = self._xnew(xnew)
        om, ph, Wt = self._features(omega, phase, W)
        S, n = int(Wt.shape[0]), xn.shape[0]
        Ut = torch.as_tensor(U, dtype=self.dtype).reshape(S, self.N).contiguous().to(self.device)
        f = torch.empty((S, n), dtype=self.dtype, device=self.device)
        g = torch.empty((S, n, self.D), dtype=self.dtype, device=self.device) if with_grad else None
        rc = self.lib.cglb_itergp_paths_eval(self._ctx, _ptr(xn), n, _ptr(om), _ptr(ph), _ptr(Wt), _ptr(Ut), int(om.shape[0]), S, _ptr(f), _ptr(g))
        _lib.check(rc, self._ctx)
        return f, g

    def grad_kff_multi(self, U, V) -> np.ndarray:
        """[sum_b u_b^T (dK_ff / dl_d) v_b for d < D, sum_b u_b^T kappa v_b] for U, V [N, S]: one evaluation of every kernel value for up to 8 pairs."""
        Ut = self._cols(U)
        Vt = self._cols(V, Ut.shape[0])
        out = np.empty(self.D + 1, dtype=np.float64)
        rc = self.lib.cglb_grad_kff_multi(self._ctx, _ptr(Ut), _ptr(Vt), int(Ut.shape[0]), out.ctypes.data_as(ctypes.POINTER(c_double)))
        _lib.check(rc, self._ctx)
        return out

    def time_grad_kff_multi(self, s: int, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_grad_kff_multi(self._ctx, int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def grad_x_kff_multi(self, U, V) -> torch.Tensor:
        """gx [N, D] (device): gx[i, k] = sum_j w_ij d K_ff[i, j] / d x_ik with w_ij = sum_b (u_bi v_bj + v_bi u_bj) for U, V [N, S], with respect to
        the raw training inputs: the pairs of grad_kff_multi differentiated in x_i.  Bitwise repeatable."""
        Ut = self._cols(U)
        Vt = self._cols(V, Ut.shape[0])
        gx = self._nan_rows()
        _lib.check(self.lib.cglb_grad_x_kff_multi(self._ctx, _ptr(Ut), _ptr(Vt), int(Ut.shape[0]), _ptr(gx)), self._ctx)
        return gx

    def time_grad_x_kff_multi(self, s: int, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_grad_x_kff_multi(self._ctx, int(s), int(reps), byref(ms)), self._ctx)
        return ms.value

    def grad_x_kff_pair(self, u, v) -> torch.Tensor:
        """grad_x_kff_multi for ONE pair u, v [N] through the single-pair instance of the pass (cglb_grad_x_kff_pair): the same sums in another
        order, equal to grad_x_kff_multi(u, v) to round-off.  Bitwise repeatable."""
        ut, vt = self._dev(u, self.N), self._dev(v, self.N)
        gx = self._nan_rows()
        _lib.check(self.lib.cglb_grad_x_kff_pair(self._ctx, _ptr(ut), _ptr(vt), _ptr(gx)), self._ctx)
        return gx

    def time_grad_x_kff_pair(self, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_grad_x_kff_pair(self._ctx, int(reps), byref(ms)), self._ctx)
        return ms.value

    def grad_x_kuf(self, G, cvec=None, wvec=None) -> torch.Tensor:
        """gx [N, D] (device): gx[n, k] = sum_m (G[m, n] + cvec[m] wvec[n]) d k(z_m, x_n) / d x_nk with respect to the raw training inputs, at the
        inducing points and hyper-parameters of the last set_hypers (cglb_grad_x_kuf).  G: [M, ldg >= N], row m contiguous (the columns from N on
        are never read); cvec [M] and wvec [N] together or not at all.  Bitwise repeatable."""
        Gt = torch.as_tensor(G, dtype=self.dtype, device=self.device)
        if Gt.dim() != 2 or Gt.shape[0] != self.M or Gt.shape[1] < self.N:
            raise ValueError(f"G must be [{self.M}, ldg >= {self.N}]")
        if (cvec is None) != (wvec is None):
            raise ValueError("cvec and wvec go together")
        Gt = Gt.contiguous()
        ct = None if cvec is None else self._dev(cvec, self.M)
        wt = None if wvec is None else self._dev(wvec, self.N)
        gx = self._nan_rows()
        _lib.check(self.lib.cglb_grad_x_kuf(self._ctx, _ptr(Gt), int(Gt.shape[1]), _ptr(ct), _ptr(wt), _ptr(gx)), self._ctx)
        return gx

    def time_grad_x_kuf(self, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_grad_x_kuf(self._ctx, int(reps), byref(ms)), self._ctx)
        return ms.value

    def set_inputs(self, X):
        """Replaces the training inputs ([N, D], any device) and keeps the targets.  The hyper-parameters of set_hypers AND gpr_set_hypers are void
        afterwards: push them again before the next evaluation (RuntimeError otherwise)."""
        Xd = torch.as_tensor(X, dtype=self.dtype).reshape(-1, self.D).contiguous().to(self.device)
        if Xd.shape[0] != self.N:
            raise ValueError(f"expected {self.N} rows of training inputs, got {Xd.shape[0]}")
        _lib.check(self.lib.cglb_set_inputs(self._ctx, _ptr(Xd)), self._ctx)
        torch.cuda.synchronize(self.device)
        self.state_version += 1

    def _nan_rows(self) -> torch.Tensor:
        """[N, D] device buffer of an input gradient: NaN until the library has written it"""
        return torch.full((self.N, self.D), float("nan"), dtype=torch.float64, device=self.device)

    def get_stat(self, name: str) -> float:
        out = c_double()
        _lib.check(self.lib.cglb_get_stat(self._ctx, name.encode(), byref(out)), self._ctx)
        return out.value

    def time_kernel(self, which: int, reps: int) -> float:
        ms = c_double()
        _lib.check(self.lib.cglb_time_kernel(self._ctx, int(which), int(reps), byref(ms)), self._ctx)
        return ms.value


class _DevPtr:
    """Minimal __cuda_array_interface__ carrier so torch can view library-owned device memory."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def _wrap_device_pointer(ptr, shape, dtype, device) -> torch.Tensor:
    typestr = "<f8" if dtype == torch.float64 else "<f4"
    return torch.as_tensor(_DevPtr(ptr, shape, typestr), device=device)
