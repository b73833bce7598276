"""Timing of the value-and-input-gradient predictors (cglb_predict_grad, cglb_gpr_predict_grad) beside the value predictors they extend
(cglb_predict, cglb_gpr_predict) on the same context and the same new points, in one process (profiles/predict_grad_timing.json).

Shapes: n_new = 4096 new points; cglb_predict_grad at N = 100 000, D = 8, M = 1024 (headline) and at N = 60 000, D = 20, M = 1024;
cglb_gpr_predict_grad at N = 16 384, D = 8.  fp64, Matern-3/2.  The two sides alternate round by round after a warm-up round of both; the sparse
predictors through cglb_time_predict_grad (HIP events on the context stream around `--reps` back-to-back calls), the exact GP by the host clock
around `--reps` back-to-back calls between device synchronisations; median, min and max of `--rounds` rounds.  `ratio` = value-and-gradient call /
value call, from the medians; `bar` = d + 1, the predictor calls that one-sided finite differences of the same gradients would take;
`below_bar` = ratio < bar.  `kernel_ms`: device time of the row-weighted pair kernel and its slab sums inside one gradient call
("predict_grad_kernel_ms").

`--mid` times the mid-width path instead (option "input_grad_mid", profiles/predict_grad_mid_timing.json): cglb_predict_grad at N = 50 000, D = 77 and
90, M = 1024, Matern-3/2 and RBF; cglb_gpr_predict_grad at N = 16 384, D = 77; lengthscales sqrt(D) on standard-normal inputs (kernel values of order 0.1;
the instruction stream does not depend on them).  The same clocks, the same alternation, the same bar d + 1.

    python tools/time_predict_grad.py [--mid] [--reps 5] [--rounds 7] [--out profiles/predict_grad_timing.json]"""
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

SPARSE_SHAPES = ((100000, 8, 1024), (60000, 20, 1024))
GPR_SHAPE = (16384, 8)
MID_SPARSE_SHAPES = ((50000, 77, 1024), (50000, 90, 1024))
MID_KINDS = ("matern32", "rbf")
MID_GPR_SHAPE = (16384, 77)
N_NEW = 4096


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def compare(grad_side, value_side, rounds, d):
    grad_side()
    value_side()   # warm-up round of both sides
    g, v = [], []
    for _ in range(rounds):
        g.append(grad_side())
        v.append(value_side())
    gs, vs = summary(g), summary(v)
    ratio = gs["median"] / vs["median"]
    return dict(grad_ms=gs, value_ms=vs, ratio=ratio, bar=d + 1, below_bar=bool(ratio < d + 1))


def report(name, r):
    print(f"{name}: value and gradient {r['grad_ms']['median']:.3f} ms ({r['grad_ms']['min']:.3f}..{r['grad_ms']['max']:.3f}), value "
          f"{r['value_ms']['median']:.3f} ms ({r['value_ms']['min']:.3f}..{r['value_ms']['max']:.3f}), ratio {r['ratio']:.3f} against the bar {r['bar']}, "
          f"pair kernel {r['kernel_ms']:.3f} ms", flush=True)


def host_timed(call, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mid", action="store_true", help="the mid-width path (33 - 96 input dimensions, option input_grad_mid)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "predict_grad_mid_timing.json" if a.mid else "predict_grad_timing.json")
    out = dict(dtype="fp64", kind="matern32", n_new=N_NEW, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), shapes={})
    if a.mid:
        out["kind"] = "per shape"

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)

    def hypers(d):
        hyp = trained_like_hypers(d)
        if a.mid:
            hyp["lengthscales"] = [float(d) ** 0.5] * d
        return hyp

    for n, d, m in (MID_SPARSE_SHAPES if a.mid else SPARSE_SHAPES):
        X, y, Z = synthetic_problem(n, d, m, seed=0)
        hyp = hypers(d)
        for kind in (MID_KINDS if a.mid else ("matern32",)):
            ctx = HipContext(X, y, m, kind)
            if a.mid:
                ctx.set_option("input_grad_mid", 1)
                assert ctx.get_stat("predict_grad_native") == 1.0
            ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
            ctx.setup()
            r = compare(lambda: ctx.time_predict_grad(N_NEW, True, a.reps), lambda: ctx.time_predict_grad(N_NEW, False, a.reps), a.rounds, d)
            ctx.time_predict_grad(N_NEW, True, 1)
            r["kernel_ms"] = ctx.get_stat("predict_grad_kernel_ms")
            name = f"cglb_N{n}_D{d}_M{m}" + (f"_{kind}" if a.mid else "")
            out["shapes"][name] = r
            report(f"cglb_predict_grad N={n} D={d} M={m} {kind}", r)
            save()
            ctx.close()
    n, d = MID_GPR_SHAPE if a.mid else GPR_SHAPE
    X, y, _ = synthetic_problem(n, d, 1, seed=0)
    hyp = hypers(d)
    ctx = HipContext(X, y, 1, "matern32")
    if a.mid:
        ctx.set_option("input_grad_mid", 1)
    ctx.gpr_set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"])
    xs = torch.as_tensor(X[:N_NEW], dtype=torch.float64, device=ctx.device)
    ctx.gpr_predict(xs)   # factors
    r = compare(lambda: host_timed(lambda: ctx.gpr_predict_grad(xs), a.reps), lambda: host_timed(lambda: ctx.gpr_predict(xs), a.reps), a.rounds, d)
    ctx.gpr_predict_grad(xs)
    r["kernel_ms"] = ctx.get_stat("predict_grad_kernel_ms")
    out["shapes"][f"gpr_N{n}_D{d}" + ("_matern32" if a.mid else "")] = r
    report(f"cglb_gpr_predict_grad N={n} D={d}", r)
    save()
    ctx.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
