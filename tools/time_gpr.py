"""Device time per evaluation of the exact GPR class (cglb_gpr_objective_and_grad) on the HIP backend, against dense torch on the same GPU.

    python tools/time_gpr.py [--reps 2] [--out profiles/gpr_timing.json]

Shapes: N in {5 000, 15 000, 30 000}, D = 8, both kernels, gpr_block in {512, 1024, 2048, 4096}; fp64, trained-like hyper-parameters.
Per (N, kernel, block): ms per evaluation without and with the gradient (HIP events around the call) and the library's own split of the
gradient evaluation into fill | factor | solve | inverse | gradient pass (cglb_get_stat "gpr_*_ms"); the factorisation rate N^3 / 3 / factor
time as a fraction of the 78.6 TF/s fp64 matrix peak of the MI355X.  Yardstick at the two smaller N: the same evaluation written densely in
torch (element-wise kernel matrix, torch.linalg.cholesky, cholesky_inverse, element-wise gradient), value only and with the gradient."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cglb_amd.data import synthetic_problem  # noqa: E402
from cglb_amd.hip_context import HipContext  # noqa: E402

SIZES = [5000, 15000, 30000]
BLOCKS = [512, 1024, 2048, 4096]
KINDS = ["rbf", "matern32"]
TORCH_SIZES = [5000, 15000]
D = 8
FP64_MATRIX_PEAK = 78.6e12
HYPERS = dict(lengthscales=np.full(D, 2.5), variance=1.0, noise=0.05, mean=0.1)
PHASES = ("fill", "factor", "solve", "inverse", "grad")


def _timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps, out


def time_library(X, y, kind, block, reps):
    ctx = HipContext(X, y, 1, kind, dtype=torch.float64, device=torch.device("cuda", 0))
    try:
        ctx.set_option("gpr_block", block)
        ctx.gpr_set_hypers(**HYPERS)
        ctx.gpr_objective_and_grad()                                   # warm-up: allocations, rocBLAS / rocSOLVER kernel selection
        ms_value, _ = _timed(lambda: ctx.gpr_objective_and_grad(with_grad=False), reps)
        ms_grad, res = _timed(ctx.gpr_objective_and_grad, reps)
        split = {p: ctx.get_stat(f"gpr_{p}_ms") for p in PHASES}       # of the last evaluation
        N = X.shape[0]
        rate = (N ** 3 / 3.0) / (split["factor"] * 1e-3)
        return dict(ms_value=round(ms_value, 3), ms_value_and_grad=round(ms_grad, 3), split_ms={k: round(v, 3) for k, v in split.items()},
                    factor_tflops=round(rate / 1e12, 2), factor_share_of_fp64_matrix_peak=round(rate / FP64_MATRIX_PEAK, 3),
                    gpr_bytes=int(ctx.get_stat("gpr_bytes")), lml=res.lml)
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def torch_evaluation(kind, X, y, with_grad):
    """lml (and its gradient) written densely in torch: the yardstick, not the reference of the tests."""
    ls = torch.as_tensor(HYPERS["lengthscales"], dtype=torch.float64, device=X.device)
    f, s, c = HYPERS["variance"], HYPERS["noise"], HYPERS["mean"]
    N = X.shape[0]
    Xs = X / ls
    d2 = torch.zeros((N, N), dtype=torch.float64, device=X.device)
    for d in range(X.shape[1]):
        d2 += (Xs[:, d, None] - Xs[None, :, d]) ** 2
    if kind == "rbf":
        K = f * torch.exp(-0.5 * d2)
        H = K
    else:
        r = math.sqrt(3.0) * torch.sqrt(d2)
        E = torch.exp(-r)
        K, H = f * (1.0 + r) * E, 3.0 * f * E
    L = torch.linalg.cholesky(K + s * torch.eye(N, dtype=torch.float64, device=X.device))
    e = (y - c).reshape(-1, 1)
    alpha = torch.cholesky_solve(e, L)
    lml = -0.5 * (e * alpha).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * N * math.log(2.0 * math.pi)
    if not with_grad:
        return float(lml)
    W = alpha @ alpha.T - torch.cholesky_inverse(L)
    WH = W * H
    g = [0.5 * (WH * (Xs[:, d, None] - Xs[None, :, d]) ** 2).sum() / ls[d] for d in range(X.shape[1])]
    g += [0.5 * (W * K).sum() / f, 0.5 * torch.trace(W), alpha.sum()]
    return float(lml), torch.stack(g).cpu().numpy()


def time_torch(X, y, kind, reps):
    Xd = torch.as_tensor(X, dtype=torch.float64, device="cuda")
    yd = torch.as_tensor(y, dtype=torch.float64, device="cuda")
    torch_evaluation(kind, Xd, yd, True)                               # warm-up
    ms_value, _ = _timed(lambda: torch_evaluation(kind, Xd, yd, False), reps)
    ms_grad, out = _timed(lambda: torch_evaluation(kind, Xd, yd, True), reps)
    torch.cuda.empty_cache()
    return dict(ms_value=round(ms_value, 3), ms_value_and_grad=round(ms_grad, 3), lml=out[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None, help="comma-separated N (default 5000,15000,30000)")
    ap.add_argument("--blocks", default=None, help="comma-separated gpr_block values (default 512,1024,2048,4096)")
    args = ap.parse_args()
    sizes = SIZES if not args.sizes else [int(t) for t in args.sizes.split(",")]
    blocks = BLOCKS if not args.blocks else [int(t) for t in args.blocks.split(",")]
    rows = []
    for N in sizes:
        X, y, _ = synthetic_problem(N, D, 1, seed=0)
        for kind in KINDS:
            row = dict(N=N, D=D, kernel=kind, library={str(b): time_library(X, y, kind, b, args.reps) for b in blocks})
            if N in TORCH_SIZES:
                row["torch"] = time_torch(X, y, kind, args.reps)
                best = min(v["ms_value_and_grad"] for v in row["library"].values())
                row["library_over_torch_value_and_grad"] = round(best / row["torch"]["ms_value_and_grad"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:   # rewritten after every row: a run cut short keeps what it measured
                with open(args.out, "w") as f:
                    json.dump(dict(tool="tools/time_gpr.py", reps=args.reps, hypers={k: np.asarray(v).tolist() for k, v in HYPERS.items()},
                                   fp64_matrix_peak_tflops=FP64_MATRIX_PEAK / 1e12, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
