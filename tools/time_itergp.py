"""Timing of the multi-pair gradient pass against S single passes, and of one iterative exact-GP evaluation by phase, in one process
(profiles/itergp_timing.json).

Per kernel (RBF, Matern-3/2) and N at D = 8, fp64: cglb_time_kernel(which=2) - the single gradient bilinear pass, the code an evaluation would
otherwise run 1 + t times - and cglb_time_grad_kff_multi for S in {1, 2, 4, 8, 11}: both are HIP events on the context stream around `--reps`
back-to-back passes, each pass with its operand prep and fixed-order sum and without a read-back (median, min and max of `--rounds` rounds after
a warm-up round).  Then
one evaluation of cglb_itergp_objective_and_grad (t = 10 probes, rank-100 preconditioner, cold start) split by the library's three phase
statistics.  The instruction model (18 + 4 Dp + 2 S_pad per group of 8) / (S (17 + 2 Dp)) is printed next to every measured ratio.

    python tools/time_itergp.py [--n 20000 100000] [--d 8] [--reps 5] [--rounds 5] [--pairs 1 2 4 8 11] [--out profiles/itergp_timing.json]

--ab-grad-multi-mid: inputs of 33 - 96 dimensions (profiles/grad_multi_mid_timing.json).  Per `--dims` D and kind, on ONE context with lengthscales
~ sqrt(D) (unclamped exponent range), cglb_time_grad_kff_multi for every S of `--pairs` with the option "grad_multi_mid" 1 (the shared-weight pass
of kernels_grad_multi_mid.hip) and 0 (S single passes and one product), in alternating rounds after a warm-up round of each, so that a drift of
the clocks hits both.  The instruction model next to every ratio: a pass of a group costs (2 Dh + 38) / 2 + S_pad + 5 lane-instructions per pair
and lane at two lanes per row, a single pass (2 Dh + 38) / 2.

    python tools/time_itergp.py --ab-grad-multi-mid [--n 50000] [--dims 40 64 77 90] --pairs 1 2 3 4 8 11 [--out profiles/grad_multi_mid_timing.json]"""
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


def alternating(fa, fb, rounds):
    """Two timed calls in alternating rounds, after one warm-up round of each."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(fa())
        tb.append(fb())
    return [dict(median=statistics.median(t), min=min(t), max=max(t)) for t in (ta, tb)]


def mid_model_ratio(S, dh):
    """Lane-instructions per pair of the grouped mid-width pass (groups of up to 8 padded to 4 or 8, a single left-over pair through the single
    pass) over those of S single passes."""
    single, cost, rest = (2 * dh + 38) / 2.0, 0.0, S
    while rest > 0:
        g = min(8, rest)
        cost += single if g == 1 else single + (4 if g <= 4 else 8) + 5
        rest -= g
    return cost / (S * single)


def ab_grad_multi_mid(a):
    out = dict(N=a.n[0], dtype="fp64", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), option="grad_multi_mid", shapes=[])
    n = a.n[0]
    for D in a.dims:
        X, y, Z = synthetic_problem(n, D, a.prec_size, seed=0)
        ls = np.random.default_rng(D).uniform(0.8, 1.6, size=D) * np.sqrt(D)
        for kind in ("rbf", "matern32"):
            ctx = HipContext(X, y, a.prec_size, kind)
            ctx.set_hypers(ls, 1.0, 0.05, 0.0, Z)
            Dh = mid_width(D)
            rec = dict(D=D, Dh=Dh, kind=kind, exp_clamp=ctx.get_stat("exp_clamp"), grad_multi_native=ctx.get_stat("grad_multi_native"),
                       matmat_native=ctx.get_stat("matmat_native"), pairs={})

            def timed(opt, S):
                ctx.set_option("grad_multi_mid", opt)
                return ctx.time_grad_kff_multi(S, a.reps)

            for S in a.pairs:
                on, off = alternating(lambda: timed(1, S), lambda: timed(0, S), a.rounds)
                ratio = on["median"] / off["median"]
                rec["pairs"][str(S)] = dict(native_ms=on, fallback_ms=off, ratio=ratio, model=mid_model_ratio(S, Dh))
                print(f"D={D} {kind} S={S}: native {on['median']:.3f} ms ({on['min']:.3f}..{on['max']:.3f}), single passes {off['median']:.3f} ms "
                      f"({off['min']:.3f}..{off['max']:.3f}), ratio {ratio:.3f} (model of the pair kernels alone {rec['pairs'][str(S)]['model']:.3f})", flush=True)
            ctx.set_option("grad_multi_mid", 1)
            out["shapes"].append(rec)
            ctx.close()
    path = a.out or os.path.join("profiles", "grad_multi_mid_timing.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


def mid_width(D):
    """Padded width of the hot operand set of a mid-width fp64 context (0: none)."""
    return 0 if D <= 32 or D > 96 else 48 if D <= 48 else 64 if D <= 64 else 80 if D <= 80 else 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-grad-multi-mid", action="store_true", help="time every S with the option grad_multi_mid 1 and 0 on one context (module docstring)")
    ap.add_argument("--dims", type=int, nargs="+", default=[40, 64, 77, 90], help="--ab-grad-multi-mid: input dimensions")
    ap.add_argument("--n", type=int, nargs="+", default=None, help="default 20000 100000, with --ab-grad-multi-mid 50000")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 2, 4, 8, 11])
    ap.add_argument("--probes", type=int, default=10)
    ap.add_argument("--prec-size", type=int, default=100)
    ap.add_argument("--out", default=None, help="default profiles/itergp_timing.json, with --ab-grad-multi-mid profiles/grad_multi_mid_timing.json")
    a = ap.parse_args()
    if a.ab_grad_multi_mid:
        a.n = a.n or [50000]
        return ab_grad_multi_mid(a)
    a.n = a.n or [20000, 100000]
    a.out = a.out or os.path.join("profiles", "itergp_timing.json")
    hyp = trained_like_hypers(a.d)
    out = dict(D=a.d, dtype="fp64", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), sizes={})
    for n in a.n:
        X, y, Z = synthetic_problem(n, a.d, a.prec_size, seed=0)
        out["sizes"][str(n)] = {}
        for kind in ("rbf", "matern32"):
            ctx = HipContext(X, y, a.prec_size, kind)
            ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
            ctx.setup()   # cglb_time_kernel(which=2) asks for the common terms
            rec = dict(Dh=mid_width(a.d), grad_multi_native=ctx.get_stat("grad_multi_native"), matmat_native=ctx.get_stat("matmat_native"),
                       single_ms=rounds_of(lambda: ctx.time_kernel(2, a.reps), a.rounds), multi_ms={}, ratio_to_S_singles={}, model={})
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
