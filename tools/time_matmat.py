"""Timing of the shared-kernel product K_ff V against S single mat-vecs, in one process (profiles/multi_rhs_timing.json).

Per kernel (RBF, Matern-3/2) at N = 100 000, D = 8, M = 1024, fp64: cglb_time_kernel(which=0) - the single mat-vec, the baseline -
cglb_time_matmat for S in {2, 4, 8}, and a cold cglb_objective_and_grad_multi at P = 4 against four single evaluations.  Each figure is
the median of `--rounds` rounds of `--reps` back-to-back launches after a warm-up round (HIP events on the context stream); min and max
of the rounds are kept as the spread.  The instruction model (18 + 3 S) / (21 S) is printed next to every measured ratio.

    python tools/time_matmat.py [--n 100000] [--d 8] [--m 1024] [--reps 10] [--rounds 7] [--columns 2 4 8] [--no-eval]
                                 [--out profiles/multi_rhs_timing.json]

--mid: the mid-width product (kernels_kff_multi_mid.hip) at the wide shapes of the README instead: N = 50 000, D = 77 and 90 (hot widths
80 and 96), RBF and Matern-3/2, S in {2, 4, 8}, with lengthscales ~ sqrt(D) (unclamped exponent range) and with l = 1 (the reference's
initial values: range-clamped instances).  cglb_time_matmat against S x cglb_time_kernel(which=0) - the unchanged single mat-vec - in the
same process, the two in alternating rounds; instruction model (Dh + 14 + 2 S_pad) / (S (Dh + 17)).  Writes
profiles/multi_rhs_mid_timing.json.

    python tools/time_matmat.py --mid [--n 50000] [--dims 77 90] [--reps 5] [--rounds 5] [--columns 2 4 8]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext


def rounds_of(fn, rounds):
    fn()  # warm-up round
    ts = [fn() for _ in range(rounds)]
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def evaluation_ms(ctx, shape, evals=3):
    ts = []
    for _ in range(evals + 1):  # the first one warms the buffers up
        v = torch.zeros(shape, dtype=torch.float64, device=ctx.device)  # cold start: v = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ctx.objective_and_grad(v, True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=statistics.median(ts[1:]), min=min(ts[1:]), max=max(ts[1:]), steps=res.steps)


def alternating(fa, fb, rounds):
    """Medians of two timed calls taken in alternating rounds (after one warm-up round of each), so that a drift of the clocks hits both."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(fa())
        tb.append(fb())
    return [dict(median=statistics.median(t), min=min(t), max=max(t)) for t in (ta, tb)]


def mid_widths(a):
    out = dict(N=a.n, M=a.m, dtype="fp64", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), shapes=[])
    for D in a.dims:
        X, Y, Z = synthetic_problem(a.n, D, a.m, seed=0)
        Dh = 48 if D <= 48 else 64 if D <= 64 else 80 if D <= 80 else 96
        ranges = (("unclamped", np.random.default_rng(D).uniform(0.8, 1.6, size=D) * np.sqrt(D)), ("clamped", np.ones(D)))
        for kind in ("rbf", "matern32"):
            for name, ls in ranges:
                ctx = HipContext(X, Y.reshape(a.n, -1)[:, 0], a.m, kind)
                ctx.set_hypers(ls, 1.0, 0.05, 0.0, Z)
                rec = dict(D=D, Dh=Dh, kind=kind, range=name, matmat_native=ctx.get_stat("matmat_native"), columns={})
                for S in a.columns:
                    mm, mv = alternating(lambda: ctx.time_matmat(S, a.reps), lambda: ctx.time_kernel(0, a.reps), a.rounds)
                    ratio = mm["median"] / (S * mv["median"])
                    sp = 2 if S <= 2 else 4 if S <= 4 else 8
                    model = (Dh + 14 + 2 * sp) / (S * (Dh + 17.0))
                    rec["columns"][str(S)] = dict(matmat_ms=mm, matvec_ms=mv, ratio_to_S_matvecs=ratio, model=model)
                    print(f"D={D} {kind} {name} S={S}: matmat {mm['median']:.3f} ms ({mm['min']:.3f}..{mm['max']:.3f}), matvec {mv['median']:.3f} ms "
                          f"({mv['min']:.3f}..{mv['max']:.3f}), ratio to {S} mat-vecs {ratio:.3f} (model {model:.3f})", flush=True)
                out["shapes"].append(rec)
                ctx.close()
    path = a.out or os.path.join("profiles", "multi_rhs_mid_timing.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mid", action="store_true", help="the mid-width shapes (module docstring)")
    ap.add_argument("--dims", type=int, nargs="+", default=[77, 90], help="--mid: input dimensions")
    ap.add_argument("--n", type=int, default=None, help="default 100000, with --mid 50000")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=None, help="default 10, with --mid 5")
    ap.add_argument("--rounds", type=int, default=None, help="default 7, with --mid 5")
    ap.add_argument("--columns", type=int, nargs="+", default=[2, 4, 8], help="column counts S of cglb_time_matmat")
    ap.add_argument("--no-eval", action="store_true", help="products only: skip the evaluations at P = 4")
    ap.add_argument("--out", default=None, help="default profiles/multi_rhs_timing.json, with --mid profiles/multi_rhs_mid_timing.json")
    a = ap.parse_args()
    a.n = a.n or (50000 if a.mid else 100000)
    a.reps = a.reps or (5 if a.mid else 10)
    a.rounds = a.rounds or (5 if a.mid else 7)
    if a.mid:
        return mid_widths(a)
    a.out = a.out or os.path.join("profiles", "multi_rhs_timing.json")
    X, Y, Z = synthetic_problem(a.n, a.d, a.m, seed=0, P=4)
    hyp = trained_like_hypers(a.d)
    out = dict(N=a.n, D=a.d, M=a.m, dtype="fp64", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), kernels={})
    for kind in ("rbf", "matern32"):
        ctx = HipContext(X, Y[:, 0], a.m, kind)
        ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
        rec = dict(matvec_ms=rounds_of(lambda: ctx.time_kernel(0, a.reps), a.rounds), matmat_ms={}, ratio_to_S_matvecs={}, model={})
        t1 = rec["matvec_ms"]["median"]
        for S in a.columns:
            r = rounds_of(lambda: ctx.time_matmat(S, a.reps), a.rounds)
            rec["matmat_ms"][str(S)] = r
            rec["ratio_to_S_matvecs"][str(S)] = r["median"] / (S * t1)
            rec["model"][str(S)] = (18 + 3 * S) / (21.0 * S)
            print(f"{kind} S={S}: matmat {r['median']:.3f} ms ({r['min']:.3f}..{r['max']:.3f}), {S} x matvec {S * t1:.3f} ms, "
                  f"ratio {rec['ratio_to_S_matvecs'][str(S)]:.3f} (model {rec['model'][str(S)]:.3f})", flush=True)
        singles = []
        for b in range(0 if a.no_eval else 4):
            ctx.set_targets(torch.from_numpy(Y[:, b].copy()))
            singles.append(evaluation_ms(ctx, (a.n,)))
        if not a.no_eval:
            ctx.set_targets(torch.from_numpy(Y))
            rec["eval_single_ms"] = singles
            rec["eval_multi_p4_ms"] = evaluation_ms(ctx, (a.n, 4))
            rec["eval_ratio_to_4_singles"] = rec["eval_multi_p4_ms"]["median"] / sum(s["median"] for s in singles)
            print(f"{kind} evaluation P=4: {rec['eval_multi_p4_ms']['median']:.1f} ms ({rec['eval_multi_p4_ms']['steps']} steps) against "
                  f"{sum(s['median'] for s in singles):.1f} ms for four single evaluations ({[s['steps'] for s in singles]} steps)", flush=True)
        out["kernels"][kind] = rec
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
