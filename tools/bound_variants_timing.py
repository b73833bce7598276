"""Device time per evaluation (bound + gradient) of the five model classes of SGPR_CONFIGS on the HIP backend.

    python tools/bound_variants_timing.py [--reps 3] [--out profiles/bound_variants_timing.json]

Shapes: N = 15 000, D = 8, M in {1024, 2048, 4096} (the pol / bike / elevators sizes of the ablation grid) and N = 50 000, D = 8,
M = 1024; fp64, RBF, trained-like hyper-parameters, Z = the first M rows.  The CG classes are timed at a fixed v (one solve first,
then evaluations with run_cg = 0): the step-independent part of an evaluation.  For the N^2M pass the tool reports its time as
t(sgprn2m) - t(sgpr) (the two differ by that pass and the algebra that consumes it) and the rate 3 N^2 M / that time against the
78.6 TF/s fp64 matrix peak of the MI355X.  "k1_launches": launches of the symmetric K_ff pair kernel in one sgpr evaluation (0: no N^2
work)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cglb_amd.data import synthetic_problem  # noqa: E402
from cglb_amd.hip_context import HipContext  # noqa: E402

OPTIONS = {"cglb": (0, 0), "cglbnm2": (1, 0), "cglbn2m": (2, 0), "sgpr": (1, 1), "sgprn2m": (2, 1)}
SHAPES = [(15000, 8, 1024), (15000, 8, 2048), (15000, 8, 4096), (50000, 8, 1024)]
FP64_MATRIX_PEAK = 78.6e12


def time_class(X, y, Z, cls, reps):
    N, M = X.shape[0], Z.shape[0]
    dev = torch.device("cuda", 0)
    ctx = HipContext(X, y, M, "rbf", dtype=torch.float64, device=dev)
    try:
        ld, qt = OPTIONS[cls]
        if cls != "cglb":
            ctx.set_option("logdet_bound", ld)
            ctx.set_option("quad_term", qt)
        ctx.set_hypers(np.full(X.shape[1], 1.5), 1.0, 0.05, 0.0, Z, 1e-6)
        v = torch.zeros(N, dtype=torch.float64, device=dev)
        first = ctx.objective_and_grad(v, run_cg=qt == 0, max_error=1.0)     # warm-up (and the solve of the CG classes)
        ctx.objective_and_grad(v, run_cg=False)
        ctx.set_option("k1_profile", 1)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            res = ctx.objective_and_grad(v, run_cg=False)
        end.record()
        torch.cuda.synchronize()
        ctx.set_option("k1_profile", 0)
        return dict(ms=start.elapsed_time(end) / reps, bound=res.bound, cg_steps=first.steps,
                    k1_launches=int(ctx.get_stat("k1_launches")) // reps)
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="N:D:M,N:D:M,... (default: the four shapes of the docstring)")
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(t) for t in s.split(":")) for s in args.shapes.split(",")]
    rows = []
    for N, D, M in shapes:
        X, y, _ = synthetic_problem(N, D, 1, seed=0)
        Z = X[:M].copy()
        t = {cls: time_class(X, y, Z, cls, args.reps) for cls in OPTIONS}
        n2m_ms = t["sgprn2m"]["ms"] - t["sgpr"]["ms"]
        flop = 3.0 * N * N * M
        row = dict(N=N, D=D, M=M, ms_per_eval={k: round(v["ms"], 3) for k, v in t.items()},
                   cg_steps_of_first_solve={k: t[k]["cg_steps"] for k in ("cglb", "cglbnm2", "cglbn2m")},
                   sgpr_k1_launches=t["sgpr"]["k1_launches"], sgprn2m_k1_launches=t["sgprn2m"]["k1_launches"],
                   n2m_pass_ms=round(n2m_ms, 3), n2m_flop=flop, n2m_tflops=round(flop / (n2m_ms * 1e-3) / 1e12, 2),
                   n2m_share_of_fp64_matrix_peak=round(flop / (n2m_ms * 1e-3) / FP64_MATRIX_PEAK, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/bound_variants_timing.py", reps=args.reps, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
