"""Run the fp32 round-off cases of tests/test_gpu_fp32_parity.py and record max_i |err_i| / s_i per case and quantity
(profiles/fp32_error_ratios.json).  The taus of tests/fp32_error_model.py are set from this file: every ratio <= tau / 4.

    python tools/fp32_error_ratios.py [--out profiles/fp32_error_ratios.json] [--only SUBSTRING]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import fp32_error_model as em  # noqa: E402
import test_gpu_fp32_parity as par  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp32_error_ratios.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--commit", default="", help="commit hash to record when the tree is not a git checkout")
    a = ap.parse_args()
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        pass
    commit = commit or "unknown"
    cases, per_q = {}, {}
    t0 = time.time()
    for name, fn, kw in par.CASES:
        if a.only not in name:
            continue
        r = fn(**kw)
        cases[name] = r
        for q, v in r.items():
            per_q.setdefault(em.quantity(q), []).append(v)
        print(f"{time.time() - t0:7.1f}s {name}: " + " ".join(f"{q}={v:.3g}" for q, v in r.items()), flush=True)
    fmv = {}
    for kind in par.KINDS:
        if a.only and a.only not in "final_matvec":
            break
        fmv[kind] = {str(k): v for k, v in par.final_matvec_case(kind).items()}
        print(f"final_matvec {kind}: {fmv[kind]}", flush=True)
    summary = {q: {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v)), "n": len(v),
                   "tau": em.TAU[q]} for q, v in sorted(per_q.items())}
    doc = {"commit": commit, "note": "max_i |out_i - ref_i| / s_i of the fp32 context against the fp64 reference on float32-rounded "
                                    "inputs (tests/fp32_error_model.py); every ratio must be <= tau / 4",
           "summary": summary, "cases": cases, "final_matvec": fmv}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    for q, s in summary.items():
        print(f"{q:8s} min {s['min']:.3g} median {s['median']:.3g} max {s['max']:.3g} (n {s['n']}, tau {s['tau']})")


if __name__ == "__main__":
    main()
