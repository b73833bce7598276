"""Timing of the training-input gradient of the CGLB bound (cglb_objective_and_grad_x) and of its two passes, on the same context and operands, in
one process (profiles/bound_input_grad_timing.json).

  pair_ms     cglb_time_grad_x_kff_pair: the single-pair K_ff pass (the kernel's G = 1 instance)
  multi1_ms   cglb_time_grad_x_kff_multi(S = 1): the G-wide instance on the same pair - unchanged by the single-pair instance, so the number the
              library had before it.  Bar: pair_ms below it (`pair_below_multi1`, from the medians).
  kuf_ms      cglb_time_grad_x_kuf: the transposed panel pass; `kuf_bytes_per_s` = M ldg 8 / kuf_ms (ldg = N rounded up to 32), to be read against
              the HBM stream rate of the device.  No bar.
  eval_ms / eval_x_ms   one warm-started evaluation (cglb_objective_and_grad with gradient, v = the solution of a first solve, run_cg on) without /
              with the input gradient, host clock around the blocking call.  Bar: eval_x_ms - eval_ms not above multi1_ms (`eval_extra_within_multi1`).

Shapes: N = 100 000, D = 8 and N = 60 000, D = 20, M = 1024; RBF and Matern-3/2; fp64.  After a warm-up round the sides alternate round by round;
median, min and max of `--rounds` rounds.

    python tools/time_bound_input_grad.py [--reps 3] [--rounds 5] [--out profiles/bound_input_grad_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from cglb_amd.data import synthetic_problem, trained_like_hypers
from cglb_amd.hip_context import HipContext

SHAPES = ((100000, 8), (60000, 20))
KINDS = ("rbf", "matern32")
M = 1024


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first K shapes only")
    ap.add_argument("--out", default=os.path.join("profiles", "bound_input_grad_timing.json"))
    a = ap.parse_args()
    out = dict(dtype="fp64", M=M, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), cells={})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)

    for n, d in SHAPES[:a.shapes]:
        X, y, Z = synthetic_problem(n, d, M, seed=0)
        hyp = trained_like_hypers(d)
        for kind in KINDS:
            ctx = HipContext(X, y, M, kind)
            ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
            assert ctx.get_stat("bound_input_grad_native") == 1.0
            v0 = torch.zeros(n, dtype=torch.float64, device=ctx.device)
            first = ctx.objective_and_grad(v0, run_cg=True, max_error=1.0, with_grad=False)   # the warm start of the timed evaluations

            def evaluation(with_x):
                v = v0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = ctx.objective_and_grad(v, run_cg=True, max_error=1.0, with_grad=True, with_input_grad=with_x)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, res.steps

            sides = (lambda: ctx.time_grad_x_kff_pair(a.reps), lambda: ctx.time_grad_x_kff_multi(1, a.reps), lambda: ctx.time_grad_x_kuf(a.reps),
                     lambda: evaluation(False)[0], lambda: evaluation(True)[0])
            for side in sides:   # warm-up round
                side()
            ts = tuple([] for _ in sides)
            for _ in range(a.rounds):
                for t, side in zip(ts, sides):
                    t.append(side())
            pair, multi1, kuf, ev, evx = (summary(t) for t in ts)
            ldg = (n + 31) // 32 * 32
            extra = evx["median"] - ev["median"]
            r = dict(pair_ms=pair, multi1_ms=multi1, kuf_ms=kuf, eval_ms=ev, eval_x_ms=evx, first_solve_steps=first.steps, warm_steps=evaluation(False)[1],
                     pair_over_multi1=pair["median"] / multi1["median"], pair_below_multi1=bool(pair["median"] < multi1["median"]),
                     kuf_bytes_per_s=M * ldg * 8 / (kuf["median"] * 1e-3), eval_extra_ms=extra, eval_extra_within_multi1=bool(extra <= multi1["median"]))
            out["cells"][f"N{n}_D{d}_{kind}"] = r
            print(f"N={n} D={d} {kind}: pair {pair['median']:.3f} ms ({pair['min']:.3f}..{pair['max']:.3f}), multi(1) {multi1['median']:.3f} ms "
                  f"({multi1['min']:.3f}..{multi1['max']:.3f}), ratio {r['pair_over_multi1']:.3f}; panel pass {kuf['median']:.3f} ms "
                  f"({kuf['min']:.3f}..{kuf['max']:.3f}), {r['kuf_bytes_per_s'] / 1e12:.2f} TB/s; evaluation {ev['median']:.2f} ms "
                  f"({ev['min']:.2f}..{ev['max']:.2f}), with input gradient {evx['median']:.2f} ms ({evx['min']:.2f}..{evx['max']:.2f}), extra {extra:.2f} ms",
                  flush=True)
            save()
            ctx.close()
    out["pair_bar_met"] = all(c["pair_below_multi1"] for c in out["cells"].values())
    out["eval_bar_met"] = all(c["eval_extra_within_multi1"] for c in out["cells"].values())
    save()
    print("pair bar", "met" if out["pair_bar_met"] else "MISSED", "| evaluation bar", "met" if out["eval_bar_met"] else "MISSED")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
