"""Developer tool: coefficients of the quarter-period cosine polynomial of cos_turns (cglb_amd/csrc/devmath.h).

  C(v) ~ cos(2 pi sqrt(v))  on 0 <= v <= 1/16  (v = a^2, a the phase folded to a quarter turn), C(0) = 1 exactly

Fit: the interpolation at Chebyshev nodes of tools/exp2_poly_fit.py (60-digit arithmetic, constant term fixed), coefficients rounded to
fp64, the error of the rounded polynomial re-measured in exact arithmetic (the approximation error alone: the round-off of the Horner
form and of the fold is measured by tests/test_sample_ref_host.py on the fp64 restatement).

usage: python tools/cos_poly_fit.py [DEGREE ...]     (degree in v; devmath.h uses 8)
"""
import os
import sys

import mpmath as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp2_poly_fit import fit  # noqa: E402

mp.mp.dps = 60


def target(v):
    return mp.cos(2 * mp.pi * mp.sqrt(v))


def max_abs_err(coef, n=4000):
    worst = mp.mpf(0)
    for k in range(n + 1):
        v = mp.mpf(k) / n / 16
        p = sum(mp.mpf(float(c)) * v ** j for j, c in enumerate(coef))
        worst = max(worst, abs(p - target(v)))
    return worst


def main():
    for deg in [int(a) for a in sys.argv[1:]] or [7, 8, 9]:
        c = fit(target, mp.mpf(0), mp.mpf(1) / 16, deg, fixed_c0=1)
        print(f"degree {deg} in v: max abs err {mp.nstr(max_abs_err(c), 3)}")
        print("   ", ", ".join(float(x).hex() for x in c[1:]), " (c1..)")


if __name__ == "__main__":
    main()
