"""Timing of the multi-column cross product against S single cross mat-vecs, and of the Lanczos variance cache end to end against the batched
solves it replaces, in one process (profiles/itergp_var_cache_timing.json).

Per kernel (RBF, Matern-3/2) and N at D = 8, fp64, n_new = 4096 new points:
  * cglb_time_cross_matmat with S columns and with -S (S single launches of the plain cross kernel on the same operands), alternated round by
    round: HIP events on the context stream around `--reps` back-to-back products (median, min and max of `--rounds` rounds after a warm-up
    round).  The instruction model per pair and group of 8 columns is k + 8 against 8 (k + 1), k the kernel-value instructions of the plain
    kernel (17 for RBF): printed next to every measured ratio.
  * cache build at rank 100 (the library's "itergp_cache_ms") and the cached predictive of the 4096 points (events around the call, and the
    library's "itergp_var_ms" for the product and the row norms alone), alternated with cglb_itergp_predict on 64 of those points (8 batched
    solves), whose time is scaled by 4096 / 64.  Both predictives start from a converged alpha, so their common first solve takes no step.

    python tools/time_itergp_var.py [--n 20000 100000] [--d 8] [--n-new 4096] [--columns 1 2 8 16 104] [--rank 100] [--reps 3] [--rounds 5]
                                    [--solve-rounds 5] [--append] [--out profiles/itergp_var_cache_timing.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext

K_INSTR = {"rbf": 17, "matern32": 25}   # vector-fp64 instructions of one kernel value at D_p = 8: 8 Gram fma + the profile (DESIGN.md sections 4, 4f)


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def model_ratio(S, k):
    groups = (S + 7) // 8
    return groups * (k + 8) / (S * (k + 1.0))


def timed(fn):
    """ms of fn() by events on the current (= the context's) stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--n-new", type=int, default=4096)
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 2, 8, 16, 104])
    ap.add_argument("--rank", type=int, default=100)
    ap.add_argument("--prec-size", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solve-rounds", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="keep the sizes already in --out")
    ap.add_argument("--out", default=os.path.join("profiles", "itergp_var_cache_timing.json"))
    a = ap.parse_args()
    hyp = trained_like_hypers(a.d)
    out = dict(D=a.d, dtype="fp64", n_new=a.n_new, rank=a.rank, reps=a.reps, device=torch.cuda.get_device_name(0), sizes={})
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            out["sizes"] = json.load(f)["sizes"]

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for n in a.n:
        X, y, Z = synthetic_problem(n, a.d, a.prec_size, seed=0)
        Xnew = np.random.default_rng(1).standard_normal((a.n_new, a.d))
        out["sizes"][str(n)] = {}
        for kind in ("rbf", "matern32"):
            ctx = HipContext(X, y, a.prec_size, kind)
            ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
            rec = dict(rounds=a.rounds, solve_rounds=a.solve_rounds, product={})
            for S in a.columns:
                ctx.time_cross_matmat(a.n_new, S, 1)
                ctx.time_cross_matmat(a.n_new, -S, 1)   # warm-up round of both sides
                multi, single = [], []
                for _ in range(a.rounds):
                    multi.append(ctx.time_cross_matmat(a.n_new, S, a.reps))
                    single.append(ctx.time_cross_matmat(a.n_new, -S, a.reps))
                m, s1 = summary(multi), summary(single)
                rec["product"][str(S)] = dict(multi_ms=m, singles_ms=s1, ratio=m["median"] / s1["median"], model=model_ratio(S, K_INSTR[kind]))
                print(f"N={n} {kind} S={S}: multi {m['median']:.3f} ms ({m['min']:.3f}..{m['max']:.3f}), {S} singles {s1['median']:.3f} ms "
                      f"({s1['min']:.3f}..{s1['max']:.3f}), ratio {m['median'] / s1['median']:.3f} (model {model_ratio(S, K_INSTR[kind]):.3f})", flush=True)
            out["sizes"][str(n)][kind] = rec
            write()
            # end to end
            ctx.itergp_predict(Xnew[:8])                       # preconditioner, alpha, buffers
            builds, cached, var_part, solved = [], [], [], []
            J = 0
            for i in range(max(a.rounds, a.solve_rounds)):
                if i < a.rounds:
                    J = ctx.itergp_var_cache(a.rank)
                    builds.append(ctx.get_stat("itergp_cache_ms"))
                    cached.append(timed(lambda: ctx.itergp_predict_cached(Xnew)))
                    var_part.append(ctx.get_stat("itergp_var_ms"))
                if i < a.solve_rounds:
                    solved.append(timed(lambda: ctx.itergp_predict(Xnew[:64])))
            rec["end_to_end"] = dict(J=J, cache_build_ms=summary(builds), cached_predict_ms=summary(cached), cached_variance_ms=summary(var_part))
            if solved:   # --solve-rounds 0 leaves the parent's side out
                scaled = statistics.median(solved) * a.n_new / 64.0
                rec["end_to_end"].update(solves_64_points_ms=summary(solved), solves_scaled_to_n_new_ms=scaled,
                                         ratio_solves_over_cached=scaled / statistics.median(cached),
                                         ratio_solves_over_build_plus_cached=scaled / (statistics.median(builds) + statistics.median(cached)))
            print(f"N={n} {kind} end to end: {rec['end_to_end']}", flush=True)
            write()
            ctx.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
