"""Timing of the value-and-input-gradient products (cglb_time_cross_grad_matmat, cglb_time_feature_grad_matmat) beside the value products they
extend (cglb_time_cross_matmat, cglb_time_feature_matmat) on the same context and the same operands, in one process
(profiles/input_grad_timing.json).

Shapes: n_new = 4096 new points at N = 100 000, D = 8 and at N = 60 000, D = 20, S in (1, 8) columns; the feature products at F = 4096 on the
same rows.  fp64, Matern-3/2.  The two sides alternate round by round after a warm-up round of both: HIP events on the context stream around
`--reps` back-to-back calls; median, min and max of `--rounds` rounds.  `ratio` = value-and-gradient product / value product, from the
medians; `bar` = d + 1, the value products that one-sided finite differences of the same gradient would take; `below_bar` = ratio < bar.

    python tools/time_input_grad.py [--reps 20] [--rounds 7] [--out profiles/input_grad_timing.json]

`--mid` times the mid-width path instead (option "input_grad_mid", profiles/input_grad_mid_timing.json): N = 50 000, D = 77 and 90, n_new = 4096,
S in (1, 8), Matern-3/2 and RBF.  The value product that exists at that width is cglb_cross_matvec, one column per call, so both sides are the
public entries on device-resident operands (each returns with the context stream idle) under a host clock: one cross_grad_matmat of S columns
against S cross_matvec calls of the same context, new points and columns.  `ratio` and `bar` as above."""
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
N_NEW, COLUMNS, FEATURES = 4096, (1, 8), 4096


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def compare(grad_side, value_side, rounds, d):
    grad_side(1)
    value_side(1)   # warm-up round of both sides
    g, v = [], []
    for _ in range(rounds):
        g.append(grad_side(None))
        v.append(value_side(None))
    gs, vs = summary(g), summary(v)
    ratio = gs["median"] / vs["median"]
    return dict(grad_ms=gs, value_ms=vs, ratio=ratio, bar=d + 1, below_bar=bool(ratio < d + 1))


MID_N, MID_DIMS, MID_KINDS = 50000, (77, 90), ("matern32", "rbf")


def host_ms(call, reps):
    """ms per call of a public entry that returns with the context stream idle"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main_mid(a):
    out = dict(dtype="fp64", n=MID_N, n_new=N_NEW, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), clock="host, public entries", shapes={})
    for d in MID_DIMS:
        X, y, Z = synthetic_problem(MID_N, d, a.prec_size, seed=0)
        hyp = trained_like_hypers(d)
        ls = [float(d) ** 0.5] * d   # standard-normal inputs: kernel values of order 0.1 (the instruction stream does not depend on them)
        for kind in MID_KINDS:
            ctx = HipContext(X, y, a.prec_size, kind)
            ctx.set_hypers(ls, hyp["variance"], hyp["noise"], hyp["mean"], Z)
            ctx.set_option("input_grad_mid", 1)
            assert ctx.get_stat("input_grad_native") == 1.0
            xnew = torch.as_tensor(X[:N_NEW], dtype=torch.float64, device=ctx.device)
            rec = {}
            for S in COLUMNS:
                V = torch.as_tensor(y, dtype=torch.float64, device=ctx.device).reshape(-1, 1).repeat(1, S).contiguous()
                cols = [V[:, s].contiguous() for s in range(S)]
                o = torch.empty((N_NEW, S), dtype=torch.float64, device=ctx.device)
                g = torch.empty((N_NEW, S, d), dtype=torch.float64, device=ctx.device)

                def values():
                    for v in cols:
                        ctx.cross_matvec(xnew, v)

                r = compare(lambda n: host_ms(lambda: ctx.cross_grad_matmat(xnew, V, out=o, gout=g), n or a.reps), lambda n: host_ms(values, n or a.reps), a.rounds, d)
                rec[f"S{S}"] = dict(cross=r)
                print(f"N={MID_N} D={d} {kind} S={S}: value and gradient {r['grad_ms']['median']:.3f} ms ({r['grad_ms']['min']:.3f}..{r['grad_ms']['max']:.3f}), "
                      f"{S} cross_matvec {r['value_ms']['median']:.3f} ms ({r['value_ms']['min']:.3f}..{r['value_ms']['max']:.3f}), ratio {r['ratio']:.2f} against the "
                      f"bar {d + 1}", flush=True)
            out["shapes"][f"N{MID_N}_D{d}_{kind}"] = rec
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
            ctx.close()
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prec-size", type=int, default=100)
    ap.add_argument("--mid", action="store_true", help="the mid-width path (33 - 96 input dimensions) against cglb_cross_matvec")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "input_grad_mid_timing.json" if a.mid else "input_grad_timing.json")
    if a.mid:
        return main_mid(a)
    out = dict(dtype="fp64", kind="matern32", n_new=N_NEW, features=FEATURES, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), shapes={})
    for n, d in SHAPES:
        X, y, Z = synthetic_problem(n, d, a.prec_size, seed=0)
        hyp = trained_like_hypers(d)
        ctx = HipContext(X, y, a.prec_size, "matern32")
        ctx.set_hypers(hyp["lengthscales"], hyp["variance"], hyp["noise"], hyp["mean"], Z)
        rec = {}
        for S in COLUMNS:
            cross = compare(lambda r: ctx.time_cross_grad_matmat(N_NEW, S, r or a.reps), lambda r: ctx.time_cross_matmat(N_NEW, S, r or a.reps), a.rounds, d)
            feat = compare(lambda r: ctx.time_feature_grad_matmat(N_NEW, FEATURES, S, r or a.reps),
                           lambda r: ctx.time_feature_matmat(N_NEW, FEATURES, S, r or a.reps), a.rounds, d)
            rec[f"S{S}"] = dict(cross=cross, feature=feat)
            for name, r in (("cross", cross), ("feature", feat)):
                print(f"N={n} D={d} S={S} {name}: value and gradient {r['grad_ms']['median']:.3f} ms ({r['grad_ms']['min']:.3f}..{r['grad_ms']['max']:.3f}), value "
                      f"{r['value_ms']['median']:.3f} ms ({r['value_ms']['min']:.3f}..{r['value_ms']['max']:.3f}), ratio {r['ratio']:.2f} against the bar {d + 1}",
                      flush=True)
        out["shapes"][f"N{n}_D{d}"] = rec
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        ctx.close()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
