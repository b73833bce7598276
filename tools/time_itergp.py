"""Timing of the multi-pair gradient pass against S single passes, and of one iterative exact-GP evaluation by phase, in one process
(profiles/itergp_timing.json).

Per kernel (RBF, Matern-3/2) and N at D = 8, fp64: cglb_time_kernel(which=2) - the single gradient bilinear pass, the code an evaluation would
otherwise run 1 + t times - and cglb_time_grad_kff_multi for S in {1, 2, 4, 8, 11}: both are HIP events on the context stream around `--reps`
back-to-back passes, each pass with its operand prep and fixed-order sum and without a read-back (median, min and max of `--rounds` rounds after
a warm-up round).  Then
one evaluation of cglb_itergp_objective_and_grad (t = 10 probes, rank-100 preconditioner, cold start) split by the library's three phase
statistics.  The instruction model (18 + 4 Dp + 2 S_pad per group of 8) / (S (17 + 2 Dp)) is printed next to every measured ratio.

    python tools/time_itergp.py [--n 20000 100000] [--d 8] [--reps 5] [--rounds 5] [--pairs 1 2 4 8 11] [--out profiles/itergp_timing.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext


def rounds_of(fn, rounds):
    fn()  # warm-up round
    ts = [fn() for _ in range(rounds)]
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def model_ratio(S, dp):
    """Vector-fp64 instructions per pair of the grouped pass (direct differences: 18 + 4 Dp + 2 S_pad per group of up to 8 pairs, padded to
    1, 2, 4 or 8) over those of S single passes in their Gram form (about 15 + 2 Dp + 2: 33 at Dp = 8)."""
    base, cost, rest = 18 + 4 * dp, 0, S
    while rest > 0:
        g = min(8, rest)
        cost += base + 2 * (1 if g == 1 else 2 if g <= 2 else 4 if g <= 4 else 8)
        rest -= g
    return cost / (S * (15.0 + 2 * dp + 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 2, 4, 8, 11])
    ap.add_argument("--probes", type=int, default=10)
    ap.add_argument("--prec-size", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "itergp_timing.json"))
    a = ap.parse_args()
    hyp = trained_like_hypers(a.d)
    out = dict(D=a.d, dtype="fp64", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), sizes={})
    for n in a.n:
        X, y, Z = synthetic_problem(n, a.d, a.prec_size, seed=0)
        out["sizes"][str(n)] = {}
        for kind in ("rbf", "matern32"):
            ctx = HipContext(X, y, a.prec_size, kind)
            ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
            ctx.setup()   # cglb_time_kernel(which=2) asks for the common terms
            rec = dict(single_ms=rounds_of(lambda: ctx.time_kernel(2, a.reps), a.rounds), multi_ms={}, ratio_to_S_singles={}, model={})
            t1 = rec["single_ms"]["median"]
            gen = torch.Generator(device="cpu").manual_seed(0)
            for S in a.pairs:
                r = rounds_of(lambda: ctx.time_grad_kff_multi(S, a.reps), a.rounds)
                rec["multi_ms"][str(S)] = r
                rec["ratio_to_S_singles"][str(S)] = r["median"] / (S * t1)
                rec["model"][str(S)] = model_ratio(S, a.d)
                print(f"N={n} {kind} S={S}: multi {r['median']:.3f} ms ({r['min']:.3f}..{r['max']:.3f}), {S} x single {S * t1:.3f} ms, "
                      f"ratio {rec['ratio_to_S_singles'][str(S)]:.3f} (model {rec['model'][str(S)]:.3f})", flush=True)
            eps = torch.randn(a.probes, a.prec_size + n, dtype=torch.float64, generator=gen)
            phases = []
            for _ in range(2):   # the first evaluation sizes the buffers
                v = torch.zeros(n, dtype=torch.float64, device=ctx.device)
                res = ctx.itergp_objective_and_grad(eps, v)
                phases.append(dict(steps=res.steps, lml=res.lml, select_ms=ctx.get_stat("itergp_select_ms"), solve_ms=ctx.get_stat("itergp_solve_ms"),
                                   grad_ms=ctx.get_stat("itergp_grad_ms")))
            rec["evaluation"] = phases[-1]
            print(f"N={n} {kind} evaluation: {phases[-1]}", flush=True)
            out["sizes"][str(n)][kind] = rec
            ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
