"""Developer tool: Matern-5/2 against the Matern-3/2 instance timed in the same run (same box): pair kernel, mat-vec, gradient pass and one
cold evaluation, contexts of the two kinds alternating.  Writes profiles/matern52_timing.json.

The instruction model expects pair kernel 29 / 28 issue slots and Gram-form gradient pass 35.2 / 33.2; with one
slot for scheduling the ratios stay below 30 / 28 and 36.2 / 33.2."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext
SHAPES = [(100000, 8, 1024), (60000, 20, 1024), (60000, 27, 1024)]
ROUNDS = 3
if len(sys.argv) > 1 and int(sys.argv[1]) > 0:  # a smaller N for a quick look: python tools/time_matern52.py 20000 [output file]
    SHAPES = [(int(sys.argv[1]), D, M) for _, D, M in SHAPES]
result = {"rounds": ROUNDS, "shapes": []}
for N, D, M in SHAPES:
    X, y, Z = synthetic_problem(N, D, M, 0)
    h = trained_like_hypers(D)
    runs = {"matern32": [], "matern52": []}
    for rnd in range(ROUNDS):
        for kind in ("matern32", "matern52"):
            ctx = HipContext(X, y, M, kind)
            ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], Z, 1e-6)
            v = torch.zeros(N, dtype=torch.float64, device=ctx.device)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = ctx.objective_and_grad(v, True, 1.0, 100, 40)      # cold: the first evaluation of a fresh context
            torch.cuda.synchronize(); cold = 1e3 * (time.perf_counter() - t0)
            runs[kind].append({"pair_kernel_ms": ctx.time_kernel(3, 3), "matvec_ms": ctx.time_kernel(0, 3), "grad_pass_ms": ctx.time_kernel(2, 3),
                               "cold_eval_ms": cold, "steps": r.steps, "bound": r.bound})
            ctx.close()
    entry = {"N": N, "D": D, "M": M, "dtype": "fp64", "runs": runs, "best": {}, "ratio_52_over_32": {}}
    for key in ("pair_kernel_ms", "matvec_ms", "grad_pass_ms", "cold_eval_ms"):
        best = {kind: min(r[key] for r in runs[kind]) for kind in runs}
        entry["best"][key] = best
        entry["ratio_52_over_32"][key] = best["matern52"] / best["matern32"]
    result["shapes"].append(entry)
    print(f"N={N} D={D}: " + ", ".join(f"{k} {entry['best'][k]['matern32']:.3f} -> {entry['best'][k]['matern52']:.3f} ms (x{entry['ratio_52_over_32'][k]:.3f})"
                                        for k in entry["best"]), flush=True)
result["model"] = {"pair_kernel_ratio": [29 / 28, 30 / 28], "grad_pass_ratio": [35.2 / 33.2, 36.2 / 33.2]}
out = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else "profiles/matern52_timing.json")
with open(out, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out)
