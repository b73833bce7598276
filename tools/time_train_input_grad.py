"""Timing of the pair-weighted training-input gradient pass (cglb_grad_x_kff_multi, csrc/kernels_train_input_grad.hip) beside the composition it
replaces and the lengthscale pass over the same pairs, on the same context and operands, in one process (profiles/train_input_grad_timing.json).

  (a) new_ms          cglb_time_grad_x_kff_multi(S): the new pass over S vector pairs
  (b) composition_ms  cglb_time_cross_grad_matmat(n_new = N, 2 S): the input-gradient cross product with xnew = X over the 2 S columns [V | U], which
                      an elementwise contraction (not timed: the composition is charged less than it costs) would turn into the same gradient
  (c) grad_l_ms       cglb_time_grad_kff_multi(S): the multi-pair lengthscale pass (each unordered pair once)

Shapes: N = 100 000, D = 8 and N = 60 000, D = 20; Matern-3/2 and RBF; S = 1, 8, 11; fp64.  All three are HIP events on the context stream around
`--reps` back-to-back calls.  After a warm-up round of the three, they alternate round by round; median, min and max of `--rounds` rounds.
Bar: (a) below (b) in every cell (`below_composition`, from the medians).  `ratio_to_grad_l` = (a) / (c) is recorded without a bar.

    python tools/time_train_input_grad.py [--reps 3] [--rounds 5] [--out profiles/train_input_grad_timing.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext

SHAPES = ((100000, 8), (60000, 20))
KINDS = ("matern32", "rbf")
PAIRS = (1, 8, 11)
M = 8   # the context's preconditioner rank: not used by any of the three


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "train_input_grad_timing.json"))
    a = ap.parse_args()
    out = dict(dtype="fp64", reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), cells={})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)

    for n, d in SHAPES:
        X, y, Z = synthetic_problem(n, d, M, seed=0)
        hyp = trained_like_hypers(d)
        for kind in KINDS:
            ctx = HipContext(X, y, M, kind)
            ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
            assert ctx.get_stat("train_input_grad_native") == 1.0 and ctx.get_stat("grad_multi_native") == 1.0
            for s in PAIRS:
                sides = (lambda: ctx.time_grad_x_kff_multi(s, a.reps), lambda: ctx.time_cross_grad_matmat(n, 2 * s, a.reps),
                         lambda: ctx.time_grad_kff_multi(s, a.reps))
                for side in sides:   # warm-up round
                    side()
                ts = ([], [], [])
                for _ in range(a.rounds):
                    for t, side in zip(ts, sides):
                        t.append(side())
                new, comp, gl = (summary(t) for t in ts)
                r = dict(new_ms=new, composition_ms=comp, grad_l_ms=gl, speedup_over_composition=comp["median"] / new["median"],
                         below_composition=bool(new["median"] < comp["median"]), ratio_to_grad_l=new["median"] / gl["median"])
                out["cells"][f"N{n}_D{d}_{kind}_S{s}"] = r
                print(f"N={n} D={d} {kind} S={s}: new {new['median']:.3f} ms ({new['min']:.3f}..{new['max']:.3f}), composition {comp['median']:.3f} ms "
                      f"({comp['min']:.3f}..{comp['max']:.3f}), lengthscale pass {gl['median']:.3f} ms; composition / new {r['speedup_over_composition']:.2f}, "
                      f"new / lengthscale pass {r['ratio_to_grad_l']:.2f}", flush=True)
                save()
            ctx.close()
    out["bar_met"] = all(c["below_composition"] for c in out["cells"].values())
    save()
    print("bar met in every cell" if out["bar_met"] else "BAR MISSED in: " + ", ".join(k for k, c in out["cells"].items() if not c["below_composition"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
