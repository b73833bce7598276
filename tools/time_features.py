"""Timing of the random-feature product (cglb_time_feature_matmat: operand records, kernel and fixed-order sums) beside one K_ff mat-vec of the
same context (cglb_time_kernel, which = 0), in one process (profiles/feature_timing.json).

Shapes: N = 100 000, D = 8 with F in (1024, 4096) and S in (1, 8, 16); N = 50 000, D = 77 (the looping instance) with the same F at S = 8.
fp64, Matern-3/2.  The two sides alternate round by round after a warm-up round of both: HIP events on the context stream around `--reps`
back-to-back calls; median, min and max of `--rounds` rounds.  `ratio` = feature product / one mat-vec, from the medians.

    python tools/time_features.py [--reps 5] [--rounds 5] [--out profiles/feature_timing.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext

SHAPES = ((100000, 8, (1024, 4096), (1, 8, 16)), (50000, 77, (1024, 4096), (8,)))


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prec-size", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "feature_timing.json"))
    a = ap.parse_args()
    out = dict(dtype="fp64", kind="matern32", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), shapes={})
    for n, d, features, columns in SHAPES:
        X, y, Z = synthetic_problem(n, d, a.prec_size, seed=0)
        hyp = trained_like_hypers(d)
        ctx = HipContext(X, y, a.prec_size, "matern32")
        ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
        rec = {}
        for F in features:
            for S in columns:
                ctx.time_feature_matmat(n, F, S, 1)
                ctx.time_kernel(0, 1)   # warm-up round of both sides
                feat, mv = [], []
                for _ in range(a.rounds):
                    feat.append(ctx.time_feature_matmat(n, F, S, a.reps))
                    mv.append(ctx.time_kernel(0, a.reps))
                f, m = summary(feat), summary(mv)
                rec[f"F{F}_S{S}"] = dict(feature_ms=f, matvec_ms=m, ratio=f["median"] / m["median"])
                print(f"N={n} D={d} F={F} S={S}: feature product {f['median']:.3f} ms ({f['min']:.3f}..{f['max']:.3f}), one K_ff mat-vec "
                      f"{m['median']:.3f} ms ({m['min']:.3f}..{m['max']:.3f}), ratio {f['median'] / m['median']:.3f}", flush=True)
        out["shapes"][f"N{n}_D{d}"] = rec
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        ctx.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
