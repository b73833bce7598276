"""Single kernel values against an extended-precision reference (test helper, not a test module; runs on any CPU).

Every N^2 product of the library evaluates its kernel values with the table-driven 2^x of csrc/devmath.h.  The suite's other comparisons are
aggregates (max |K p - ref| / max |ref|, random p), which dilute a defect that touches one table slot, one lane position or only the values
of 2^-300 .. 2^-950.  This module supplies what tests/test_kernel_value_cases_host.py and tests/test_gpu_kernel_values.py need to compare
ONE value at a time:

  * `build_set`: point sets whose pair exponents land on the evaluator's edges (integer hot-unit exponents from both sides, all 256 table
    slots, the largest exponent at the library's own range figure, coincident points), at an N that is no multiple of 16;
  * `regime`: the rule of cglb_set_hypers restated (range figure, integer bound, positivity bias and its cap -> exp_clamp, m32_bias);
  * `exponents`, `profiles`: kappa and the gradient profile h of every pair in np.longdouble from exact coordinate differences and the closed forms of
    include/cglb_hip.h; `certify` holds it to mpmath at 50 digits;
  * `tolerance`: the per-element bound, a sum of derived terms (below);
  * `emulate`: the device's data flow in float64 NumPy (operand scaling, Gram chain, table form), with the DEFECTS the checks must reject;
    `emulate_direct`: the direct form of the input-gradient products (differences, fma chain of d2 - by lane parts at mid width -, sqrt, Horner
    polynomials, the same table step) with its own defects, and `swap_columns` / `multi_pair_model` for the defects of the WEIGHTS a value meets,
    which only a unit-vector read-out in every column slot, pair slot and orientation sees.

Units.  "Hot units": 1/256 octave.  E >= 0 is the exponent magnitude of a pair in hot units, e = 2^(-E/256), s = E ln2 / 256 (= the textbook
argument sqrt(2 nu) r of a Matern kind; RBF: s = d^2 / 2).  d2 is the squared distance of the hot operands: RBF E = d2 / 2 (operands 16 xs),
Matern kinds E = 2 sqrt(d2) (operands 128 xs: half scale, sqrt_hot returns twice the root).  u = 2^-53.

Tolerance of one kernel value, in units of the variance f (`tolerance`; every term is a function of this module):

  (a) level_term        LEVEL[precision] * kappa: the evaluator's relative error as devmath.h states it (EXACT 1.5 ulp for table entry,
                        polynomial and their product; FAST 3.5e-14 and LOW 1.03e-10 for the polynomial alone, to which the table entry's
                        and the product's rounding, 2 u, are added), plus the square root's relative error e_root through the sensitivity
                        of the value to the root AS THE CODE FORMS IT:  hot pair stream (matern_kpoly_hot: the quadratic term of
                        Matern-5/2 comes from d2, not from the root)  Matern-3/2 s^2 e, Matern-5/2 (s^2 + s^3/3) e;  Horner forms of
                        the gradient pass  s^2 e, s^2 (1 + s) e / 3;  h: 3 s e, 5/3 s^2 e.  e_root: 2.1e-14 for the one-step root of
                        FAST and LOW (sqrt_hot), 2 u for the two-step root and for sqrt_pos.  The folded column weight of the
                        unclamped RBF instances is a second 2^x (exp2_neg, 1.8e-16).
  (b) rounding_term     u * kappa for every further rounded operation of the path (`Path.n_round`; counted from the code, listed at `path_for`)
  (c) gram_term         the change of the value when d2 moves by delta_d2, taken on the closed form at both ends of the interval (every
                        profile is monotone in E), delta_d2 = cancellation + operand scaling:
                          Gram form     (5 D + 3) u amax_ij, devmath.h's bound with amax_ij = max(|xh_i|^2, |xh_j|^2) of the pair (its
                                        derivation bounds partial sums of size 1.5 amax; the pair's own norms do).  The mid-width
                                        instances (32 < D <= 96) sum two interleaved chains: three roundings more, 5 D + 6.  The Gram
                                        tiles (rocBLAS GEMM, any summation order) stay inside 5 D + 3 as well
                          direct form   (D + 3) u d2 (D rounded differences, squares and sums; no cancellation).  The mid-width input-gradient
                                        kernel sums four lane parts of two interleaved chains each: a term passes Dh / 8 + 3 <= 15 rounded
                                        sums, fewer than the D of one chain, so the figure holds there
                          scaling       xh = fl(fl(x - c) s_d), s_d = fl(kscale hot / l_d): 3 u relative on s_d (common to both points),
                                        2 u on each operand:  6 u d2 + 8 u sqrt(amax_ij) |xh_i - xh_j|_1  (kernels_prep.hip)
  (d) bias_term         biased instances (Matern kinds, unclamped, FAST and LOW): the documented effect of the positivity bias on a
                        value, 2 (ln2/256)^2 bias for Matern-3/2 and a third of that for Matern-5/2 (devmath.h CGLB_M32_BIAS_*)
  (e) clamp floor       clamped instances, reference below 2^-1000: no relative check.  0 <= value <= floor.  For kappa the hot stream
                        forms its polynomial factor from the UNclamped root, so floor = P(s at the upper end of the interval) 2^-1000;
                        hfac_tab_batch clamps the root first, (1 + 1000 ln2) 2^-1000 - the direct gradient pass takes the same polynomial of
                        the unclamped root as kappa.
  (f) gradient entries  out[k] = f h delta_k^2 / l_k, delta_k = (x_ik - x_jk) / l_k:  f / l_k (tol_h delta_k^2 + h (9 u delta_k^2 +
                        4 u |delta_k| (|z_ik| + |z_jk|))), z = (x - c) / l: the rounded difference and square (3 u), the accumulate, the
                        two scale products and the rounded scale (6 u), and the operands' own rounding.  The moment form of the Gram
                        gradient pass is not reachable through cglb_grad_kff_multi on inputs of up to 32 dimensions (the multi-pair
                        kernel takes direct differences for every S), so no cancellation term is needed for the sets A - E.  Inputs of 33 .. 96
                        dimensions (wide_reg 1) form delta_k^2 from moments: the absolute term of `grad_tolerance(moments=True)`, derived
                        there.  Which kernel runs there depends on S: cglb_grad_kff_multi cuts the pairs into groups of 8 in order; a
                        group of two or more runs grad_kff_multi_mid_kernel (kernels_grad_multi_mid.hip, padded to 4 or 8 pairs), which
                        forms out[D] = kappa itself from P(r) at the exponent's root - path "grad_multi_mid"; a single pair (S = 1, or the one
                        left over after a group of 8) and every pair under the option grad_multi_mid 0 run the single pass of
                        kernels_grad_mid.hip - path "grad_mid" - and take out[D] from one product, bounded by the mat-vec's path.
  (g) input gradients   cross_grad_kernel, weighted_grad_kernel, cross_grad_mid_kernel (paths "cross_grad", "cross_grad_weighted",
                        "cross_grad_mid"): out[i, j] = f kappa_ij by (a) - (e) of the direct form; gout[i, j, k] = -f h_ij delta_k / l_k,
                        delta_k = (x*_ik - x_jk) / l_k:  f / l_k (tol_h |delta_k| + h (c u |delta_k| + 2 u (|z_ik| + |z_jk|))) with c =
                        INPUT_GRAD_ROUNDINGS of the path (`input_grad_tolerance`, derived there); exactly zero where x*_ik == x_jk; under the
                        floor the sign of -delta_k and at most floor_h |delta_k| / l_k.
  Gram tiles (D > 96, or wide_reg 0; the cross mat-vec of every input wider than 32): no table and no precision level - exp2_neg (1.8e-16) and
  sqrt_pos on the scaled operands, the Horner polynomials; same Gram term.  The rectangular tiles of the cross mat-vec take no clamp: the relative
  check reaches down to 2^-1022, below which the value must lie in [0, 2^-1022].
  Not covered: the feature products' cos_turns / sincos_turns, the gradient pass through the Gram tiles (wide_reg 0, D > 96), fp32.

Case table (`case_table`; RBF rows by the range figure oct = 2 s2, Matern rows by s2):
  A    D 1    ordinary range
  B/C  D 2    2 % below / above the clamp switch (RBF oct 931 / 969; Matern s2 at 0.98 / 1.02 of the bias cap)
  C'   D 2    Matern only: 2 % below / above the integer bound s2 = 7629 (both clamped by the bias cap already)
  D    D 3    oct 2400: clamped, values below the floor
  E    D 8, D 12 (padded width 16: column groups of 4 of the input-gradient products), D 32 at the widest unclamped range
  F    D 40 unclamped, D 64 clamped, D 77 clamped, D 90 unclamped: the four hot widths 48, 64, 80, 96 (wide_reg 1: mid-width symmetric
       stream and gradient passes; 0: Gram tiles).  `axis_variants`: the same rows with the sweep on a coordinate of lane part 2 and on the
       last coordinate - the mid-width gradient kernels share a point among four lanes, and the row itself puts every designed exponent
       into the first
  G    D 100  Gram tiles

No term is tuned to the device's output.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TAB = 256
C_HOT = math.log(2.0) / TAB              # ln2 per hot unit
LOG2E = 1.4426950408889634               # the double the device's CGLB_LOG2E rounds to
FLOOR_OCT = 1000                         # CGLB_EXP_FLOOR_OCT
BIAS_FACTOR = 1.5 * 1.1102230246251565e-16  # CGLB_M32_BIAS_FACTOR
BIAS_MAX = 2.0e-8                        # CGLB_M32_BIAS_MAX
KINDS = ("rbf", "matern32", "matern52")
EXACT, FAST, LOW = 0, 1, 2
# devmath.h, precision levels.  Its figures are rounded: each is taken at the upper end of what its last digit covers ("~3e-16 (1.5 ulp)" as
# 1.5 ulp = 3 u, "3.5e-14" as 3.55e-14, "1.03e-10" as 1.035e-10 - the degree-2 fit of tools/exp2_poly_fit.py measures 1.0347e-10)
LEVEL = {EXACT: 3 * U, FAST: 3.55e-14 + 2 * U, LOW: 1.035e-10 + 2 * U}
E_ROOT = {EXACT: 2 * U, FAST: 2.1e-14, LOW: 2.1e-14}                     # sqrt_hot
E_ROOT_POS = 2 * U                                                       # sqrt_pos
LEVEL_EXP2NEG = 1.8e-16                                                  # exp2_neg (the folded column weight)
N_SWEEP = 272
GRID = 2.0 ** 50                         # coordinates are multiples of 2^-50 below 2^13: differences are exact in np.longdouble


def kscale(kind: str) -> float:
    """cglb_kscale_of_kind, in the device's double arithmetic"""
    return math.sqrt(LOG2E) if kind == "rbf" else (1.7320508075688772 if kind == "matern32" else 2.23606797749979) * LOG2E


def hot_scale(kind: str) -> float:
    return 16.0 if kind == "rbf" else 128.0


# ---- the rule of cglb_set_hypers ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Regime:
    s2: float
    oct: float
    int_ok: bool
    exp_clamp: bool
    m32_bias: float


def column_means(X: np.ndarray) -> np.ndarray:
    """cglb_set_data: the rows added in order, then one division"""
    s = np.zeros(X.shape[1])
    for row in X:
        s = s + row
    return s / float(X.shape[0])


def regime_details(kind: str, X: np.ndarray, ls: np.ndarray) -> Regime:
    c = column_means(X)
    dev = X - c
    xrange = np.abs(dev).max(axis=0)
    xradius2 = float((dev * dev).sum(axis=1).max())
    ks = kscale(kind)
    s2 = float(sum((xrange[d] * ks / ls[d]) ** 2 for d in range(X.shape[1])))
    octv = 2.0 * s2 if kind == "rbf" else 2.0 * math.sqrt(s2)
    int_ok = 2.0 * s2 * TAB * (1.0 if kind == "rbf" else TAB) < 1.0e9
    clamp = not (int_ok and octv < 0.95 * FLOOR_OCT)
    bias = 0.0
    if kind != "rbf":
        hs = hot_scale(kind)
        lmin = float(np.min(ls))
        amax = min(s2, ks * ks * xradius2 / (lmin * lmin)) * hs * hs
        bias = max(BIAS_FACTOR * (5.0 * X.shape[1] + 3.0) * amax, 1.0e-200)
        if bias > BIAS_MAX:
            clamp = True
    return Regime(s2, octv, int_ok, clamp, bias)


def regime(kind: str, X: np.ndarray, ls: np.ndarray) -> Tuple[int, float]:
    """(exp_clamp, m32_bias) as cglb_get_stat returns them after cglb_set_hypers"""
    r = regime_details(kind, X, ls)
    return int(r.exp_clamp), r.m32_bias


def bias_cap_s2(D: int) -> float:
    """the s2 at which the positivity bias reaches its cap (box bound of amax)"""
    return BIAS_MAX / (BIAS_FACTOR * (5.0 * D + 3.0) * 128.0 * 128.0)


INT_BOUND_S2 = 1.0e9 / (2.0 * TAB * TAB)   # Matern kinds: 7629.4


# ---- point sets --------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str          # set letter (+ variant)
    kind: str
    D: int
    target: float      # the library's range figure the set is built to: RBF oct, Matern kinds s2
    clamp: int         # the side of the switch the row claims
    note: str
    axis: int = 0      # the coordinate that carries the sweep (and its lengthscale); `axis_variants`


def case_table() -> List[Case]:
    out = []
    out += [Case("A", "rbf", 1, 60.0, 0, "ordinary range"),
            Case("B", "rbf", 2, 931.0, 0, "2 % below the clamp switch"),
            Case("C", "rbf", 2, 969.0, 1, "2 % above it, every value above the floor"),
            Case("D", "rbf", 3, 2400.0, 1, "far inside the clamped regime, values below the floor"),
            Case("E8", "rbf", 8, 200.0, 0, "Gram chain of 8"),
            Case("E12", "rbf", 12, 200.0, 0, "padded width 16: column groups of 4 of the input-gradient products"),
            Case("E32", "rbf", 32, 931.0, 0, "longest narrow Gram chain at the widest unclamped range"),
            Case("F40", "rbf", 40, 200.0, 0, "mid width (wide_reg 1 and 0), unclamped"),
            Case("F64", "rbf", 64, 969.0, 1, "mid width, hot width 64 (no padding), clamped, every value above the floor"),
            Case("F77", "rbf", 77, 1200.0, 1, "mid width (wide_reg 1 and 0), clamped, values below the floor"),
            Case("F90", "rbf", 90, 200.0, 0, "mid width, hot width 96, unclamped"),
            Case("G100", "rbf", 100, 200.0, 0, "Gram tiles")]
    for kind in ("matern32", "matern52"):
        out += [Case("A", kind, 1, 400.0, 0, "ordinary range (oct 40)"),
                Case("B", kind, 2, 0.98 * bias_cap_s2(2), 0, "2 % below the bias cap"),
                Case("C", kind, 2, 1.02 * bias_cap_s2(2), 1, "2 % above the bias cap: clamped for the bias"),
                Case("C'-", kind, 2, 0.98 * INT_BOUND_S2, 1, "2 % below the integer bound (clamped by the bias cap already)"),
                Case("C'+", kind, 2, 1.02 * INT_BOUND_S2, 1, "2 % above the integer bound"),
                Case("D", kind, 3, 1200.0 ** 2, 1, "far inside the clamped regime (oct 2400), values below the floor"),
                Case("E8", kind, 8, 0.9 * bias_cap_s2(8), 0, "Gram chain of 8 at the widest biased range"),
                Case("E12", kind, 12, 0.9 * bias_cap_s2(12), 0, "padded width 16: column groups of 4 of the input-gradient products"),
                Case("E32", kind, 32, 0.9 * bias_cap_s2(32), 0, "longest narrow Gram chain at the widest biased range"),
                Case("F40", kind, 40, 0.9 * bias_cap_s2(40), 0, "mid width (wide_reg 1 and 0), unclamped and biased"),
                Case("F64", kind, 64, 400.0, 1, "mid width, hot width 64 (no padding), clamped for the bias"),
                Case("F77", kind, 77, 400.0, 1, "mid width (wide_reg 1 and 0), clamped for the bias"),
                Case("F90", kind, 90, 0.9 * bias_cap_s2(90), 0, "mid width, hot width 96, unclamped and biased"),
                Case("G100", kind, 100, 100.0, 1, "Gram tiles (the regime figure says clamped; the tiles take no table)")]
    return out


def hot_width(D: int) -> int:
    """padded width of the hot operand set of a mid-width context (33 .. 96 dimensions): the next multiple of 16 from 48 on"""
    return max(48, (D + 15) // 16 * 16)


def axis_variants(case: Case) -> List[Case]:
    """A mid-width row with its sweep on the last coordinate (last lane part of the four a row is shared by; at D = 40 and 77 a part that is partly
    zero padding) and on one coordinate of lane part 2 (coordinates Dh/2 .. 3 Dh/4 - 1).  The row itself (axis 0) carries its designed exponents in
    lane part 0 alone.  Not rows of `case_table`: only the tests of the kernels that split a point over lanes run on them."""
    assert 32 < case.D <= 96 and case.axis == 0
    mid = hot_width(case.D) // 2 + hot_width(case.D) // 8     # the middle of part 2
    assert mid < case.D - 1
    return [Case(f"{case.name}x{a}", case.kind, case.D, case.target, case.clamp, case.note + f", sweep on coordinate {a}", a) for a in (mid, case.D - 1)]


def lane_part(case: Case, k: int) -> int:
    """which of the four lane parts of a mid-width row holds coordinate k"""
    return k // (hot_width(case.D) // 4)


def case_id(c: Case) -> str:
    return f"{c.kind}-{c.name}"


def find_case(kind: str, name: str) -> Case:
    return next(c for c in case_table() if c.kind == kind and c.name == name)


def _quantise(X: np.ndarray) -> np.ndarray:
    return np.round(X * GRID) / GRID


def sweep_exponents() -> np.ndarray:
    """hot-unit exponents of the sweep against the centre: k +- 1e-9, the sign changing every second point, every 16th exactly k"""
    k = np.arange(N_SWEEP, dtype=np.float64)
    eps = np.where((np.arange(N_SWEEP) // 2) % 2 == 0, 1e-9, -1e-9)
    eps[np.arange(N_SWEEP) % 16 == 8] = 0.0
    eps[0] = 1e-9
    return k + eps


@lru_cache(maxsize=None)
def _build(kind: str, D: int, target: float, axis: int = 0):
    ls = 0.8 + 0.1 * (np.arange(D) % 5)
    ks = kscale(kind)
    S = target / 2.0 if kind == "rbf" else target          # sum_d (v_d ks / l_d)^2 of a corner
    E = sweep_exponents()
    z = np.sqrt(E / 128.0) if kind == "rbf" else E / 256.0  # scaled distance from the centre
    sign = np.where(np.arange(N_SWEEP) % 2 == 0, 1.0, -1.0)
    g = 1.0
    for _ in range(4):   # the column means move with the points: fit the corner to the LIBRARY's range figure
        # scaled corner coordinates: an equal share of S per dimension, unless the sweep along its axis would then leave the box - the corner
        # must fix the range in every column
        w = np.full(D, math.sqrt(S / D))
        if D > 1 and w[axis] < 1.15 * z.max():
            w[:] = math.sqrt((S - (1.15 * z.max()) ** 2) / (D - 1))
            w[axis] = 1.15 * z.max()
        v = g * ls / ks * w
        X = np.zeros((4 + N_SWEEP, D))
        X[1], X[2], X[3] = v, -v, v   # two opposite corners and an exact duplicate of the first
        X[4:, axis] = sign * z * ls[axis] / ks
        X = _quantise(X)
        r = regime_details(kind, X, ls)
        have = r.oct if kind == "rbf" else r.s2
        g *= math.sqrt(target / have)
    X.setflags(write=False)
    ls.setflags(write=False)
    return X, ls


def build_set(case: Case) -> Tuple[np.ndarray, np.ndarray]:
    """X [276, D] (row 0 the centre, 1 and 2 opposite corners, 3 a duplicate of row 1, 4.. the sweep along coordinate `case.axis`, sides
    alternating) and the lengthscales.  `check_set` asserts what the layout is for."""
    return _build(case.kind, case.D, case.target, case.axis)


def new_points(case: Case) -> np.ndarray:
    """cross products: the set itself, five points off it and one at 1e3 in every coordinate"""
    X, _ = build_set(case)
    rng = np.random.default_rng(1000 + case.D)
    span = np.abs(X).max(axis=0)
    off = _quantise(rng.uniform(-1.0, 1.0, (5, case.D)) * span)
    far = np.full((1, case.D), 1.0e3)
    return np.concatenate([X, off, far], axis=0)


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
def _ld_consts(kind: str):
    log2e = LD(1) / np.log(LD(2))
    nu2 = {"matern32": LD(3), "matern52": LD(5)}.get(kind)
    return log2e, nu2


def exp2_neg_hot(E):
    """2^(-E/256) in np.longdouble: integer octaves and a fraction in [0, 1), so the argument of exp2l stays small"""
    o = E / LD(TAB)
    n = np.floor(o)
    return np.ldexp(np.exp2(-(o - n)), -n.astype(np.int64))


def profiles(kind: str, E):
    """kappa and h (units of the variance) at the hot-unit exponent E, np.longdouble"""
    E = np.asarray(E, dtype=LD)
    e = exp2_neg_hot(E)
    s = E * (np.log(LD(2)) / LD(TAB))
    if kind == "rbf":
        return e, e
    if kind == "matern32":
        return (LD(1) + s) * e, LD(3) * e
    return (LD(1) + s + s * s / LD(3)) * e, LD(5) / LD(3) * (LD(1) + s) * e


def exponents(kind: str, Xrow: np.ndarray, X: np.ndarray, ls: np.ndarray):
    """E [rows, N] in hot units from exact coordinate differences"""
    log2e, nu2 = _ld_consts(kind)
    q = np.zeros((Xrow.shape[0], X.shape[0]), dtype=LD)
    for d in range(X.shape[1]):
        diff = (Xrow[:, d].astype(LD)[:, None] - X[:, d].astype(LD)[None, :]) / LD(ls[d])
        q += diff * diff
    if kind == "rbf":
        return LD(TAB // 2) * log2e * q
    return LD(TAB) * np.sqrt(nu2) * log2e * np.sqrt(q)


def certify(kind: str, Xrow: np.ndarray, X: np.ndarray, ls: np.ndarray, pairs, E, kap, h):
    """largest relative deviation of the longdouble kappa and h from mpmath at 50 digits over `pairs` [(i, j)]; returns per-pair arrays"""
    import mpmath as mp
    out_k, out_h = [], []
    with mp.workdps(50):
        ln2 = mp.log(2)
        for i, j in pairs:
            q = mp.mpf(0)
            for d in range(X.shape[1]):
                t = (mp.mpf(float(Xrow[i, d])) - mp.mpf(float(X[j, d]))) / mp.mpf(float(ls[d]))
                q += t * t
            if kind == "rbf":
                k_mp = h_mp = mp.exp(-q / 2)
            else:
                s = mp.sqrt((3 if kind == "matern32" else 5) * q)
                k_mp = (1 + s) * mp.exp(-s) if kind == "matern32" else (1 + s + s * s / 3) * mp.exp(-s)
                h_mp = 3 * mp.exp(-s) if kind == "matern32" else mp.mpf(5) / 3 * (1 + s) * mp.exp(-s)
            # longdouble -> mpmath without going through a double: mantissa and exponent
            def to_mp(x):
                m, ex = np.frexp(x)
                hi = float(m)
                lo = float(m - LD(hi))
                return (mp.mpf(hi) + mp.mpf(lo)) * mp.mpf(2) ** int(ex)
            out_k.append(float(abs(to_mp(kap[i, j]) / k_mp - 1)))
            out_h.append(float(abs(to_mp(h[i, j]) / h_mp - 1)))
    return np.array(out_k), np.array(out_h)


# ---- device operands (float64, as kernels_prep.hip forms them) ----------------------------------------------------------------------------
def fma(a, b, c):
    """fused multiply-add of float64 arrays through np.longdouble (the 2^-64 of the product is far below the rounding to double)"""
    return (np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD) + np.asarray(c, dtype=LD)).astype(np.float64)


@dataclass
class Operands:
    xh: np.ndarray     # [n, D] hot operands
    a: np.ndarray      # [n] |xh|^2 (fma chain)
    center: np.ndarray
    scale: np.ndarray


def operands(kind: str, X: np.ndarray, ls: np.ndarray, pts: Optional[np.ndarray] = None) -> Operands:
    c = column_means(X)
    scale = (kscale(kind) * hot_scale(kind)) / ls
    P = X if pts is None else pts
    xh = (P - c) * scale
    a = np.zeros(P.shape[0])
    for d in range(P.shape[1]):
        a = fma(xh[:, d], xh[:, d], a)
    return Operands(xh, a, c, scale)


# ---- tolerance ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Path:
    """The arithmetic one family of instances runs.  n_round / n_round_h: rounded operations beyond the evaluator, counted from the code."""
    name: str
    prec: int
    clamp: bool
    fold: bool       # RBF, unclamped, symmetric kernels: 2^(a_j) folded into the column operand
    biased: bool     # Matern kinds, unclamped, FAST and LOW: positivity bias in the row seeds
    form: str        # "gram" | "direct"
    hot_poly: bool   # matern_kpoly_hot (quadratic term from d2) or the Horner form of the root
    n_round: int
    n_round_h: int = 0
    chain_extra: int = 0   # roundings of the Gram chain beyond devmath.h's D + 1 (mid width: two interleaved chains and their sum)
    tiles: bool = False    # Gram tiles (kernels_wide.hip): exp2_neg and sqrt_pos in scaled units, no table, no precision level


# Rounded operations, per path, beyond LEVEL (table entry, polynomial, their product):
#   pair stream (kappa_hot_*): Matern-3/2 lin = fma(rT, c, 1) [1], P * lin [1];  Matern-5/2 one more fma [3 in all];  every kind: var * sum [1]
#     (kap * p_j with p_j = 1 and the sums of exact zeros are exact);  folded: p_j * w_j with p_j = 1 is exact, the row-side product kap' * pw_j
#     or the column sum times wcol_j [1]
#   multi-pair gradient kernel: RBF kappa none (hv = tab * w, w = 1); Matern kappa: the Horner polynomial [1 | 2] and fma(ew, poly, 0) [1];
#     h: the constant's own rounding, its product(s) with lin and ew [Matern-3/2 1, Matern-5/2 4]
#   input-gradient products (cross_grad_kernel, weighted_grad_kernel, cross_grad_mid_kernel; devmath.h kappa_hfac_hot_from_d2): direct differences, ALWAYS
#     the range-clamped 2^x, never folded or biased, rT = 2 sqrt_pos(d2) (the doubling is exact), the Horner polynomials of that root.
#     kappa: RBF none; matern_kpoly [Matern-3/2 one fma, Matern-5/2 two] and its product with e [1]; then fma(kv, 1, 0) and the sums of exact zeros of the
#     slabs are exact, and the finish kernel's vscale * s [1]:  1 | 3 | 4.
#     h: RBF none; Matern-3/2 3.0 * e [1]; Matern-5/2 5/3 rounded [1], matern52_hlin's fma [1], their product [1], its product with e [1]:  0 | 1 | 4.
#     What follows h on the way to a gradient entry is counted in INPUT_GRAD_ROUNDINGS (`input_grad_tolerance`).
#     Mid width: d2 is the sum of four lane parts, each two interleaved fma chains of Dh / 8 terms, then d2 + d2b, sum_row_pairs, sum_halves: a term
#     passes Dh / 8 + 3 <= 15 rounded sums where the narrow chain's passes up to D, so (D + 3) u d2 of `delta_d2` bounds it and chain_extra stays 0.
#   mid-width multi-pair gradient kernel (kernels_grad_multi_mid.hip; grad_pass.h): Gram form on grad_mid's chain (chain_extra 5), follows exp_clamp, folds
#     and biases as pair_fold / pair_biased say, level 2 runs as level 1, sqrt_hot's root.  With unit vectors the pair weight w (BcastChain2 over the
#     slots, w + w1, sum_halves) is 1 or, folded, the column weight itself: exact.
#     kappa (out[D], unscaled): RBF the sum of S0 = e * w [folded 1]; Matern kinds matern_kpoly of the exponent's root [1 | 2] and fma(ew, poly, acck) [1];
#     block_sum and the finish kernel add exact zeros:  0 (+ 1 folded) | 2 | 3.
#     h: ew [folded 1]; Matern-5/2 matern52_hlin's fma [1] and ew * L [1]; hfac_scale rides in the finish kernel's fac = hscale * var / hot^2: Matern-3/2
#     3 * var [1], Matern-5/2 5/3 rounded [1] and its product with var [1] (RBF: var / hot^2 is the single pass's own factor):  0 (+ 1 folded) | 1 | 4.
INPUT_GRAD_ENTRIES = ("cross_grad", "cross_grad_weighted", "cross_grad_mid")


def path_for(entry: str, kind: str, prec: int, exp_clamp: int) -> Path:
    mat = {"rbf": 0, "matern32": 2, "matern52": 3}[kind]
    if entry in ("matvec_sym", "matmat"):     # kernels_kff_sym.hip, kernels_kff_multi.hip (not native when clamped: single symmetric mat-vecs)
        clamp = bool(exp_clamp)
        fold = kind == "rbf" and not clamp
        return Path(entry, prec, clamp, fold, kind != "rbf" and not clamp and prec != EXACT, "gram", True, mat + 1 + (1 if fold else 0))
    if entry in ("matvec_mid", "matmat_mid"):  # kernels_kff_sym.hip MID / kernels_kff_multi_mid.hip: the symmetric stream, g0 + g1 of two chains
        clamp = bool(exp_clamp)
        fold = kind == "rbf" and not clamp
        return Path(entry, prec, clamp, fold, kind != "rbf" and not clamp and prec != EXACT, "gram", True, mat + 1 + (1 if fold else 0), 0, 3)
    if entry == "grad_mid":   # kernels_grad_mid.hip: Gram form, two chains, their sum and the sum over the lanes sharing a row (5 roundings more);
        # hfac_tab_batch: L = fma [1], (tab * L) [1], * P counted in LEVEL; hscale * u (5/3 rounded [1], product [1]); h * w [1]; level 2 runs as level 1
        clamp = bool(exp_clamp)
        fold = kind == "rbf" and not clamp
        pr = EXACT if prec == EXACT else FAST
        return Path(entry, pr, clamp, fold, kind != "rbf" and not clamp and pr != EXACT, "gram", True, 0,
                    {"rbf": 1, "matern32": 1, "matern52": 5}[kind] + (1 if fold else 0), 5)
    if entry == "tiles":                       # kernels_wide.hip wide_profile: Horner polynomial [1 | 2], its product with 2^-r [1], var [1]
        return Path(entry, EXACT, bool(exp_clamp), False, False, "gram", False, {"rbf": 1, "matern32": 3, "matern52": 4}[kind], 0, 0, True)
    if entry == "matvec_plain":               # kernels_kff.hip kff_matvec_kernel: CLAMP follows exp_clamp, never folded or biased
        return Path(entry, prec, bool(exp_clamp), False, False, "gram", True, mat + 1)
    if entry in ("cross_matvec", "cross_matmat"):   # always the range-clamped 2^x
        return Path(entry, prec, True, False, False, "gram", True, mat + 1)
    if entry == "grad":                        # kernels_grad_multi.hip: direct differences, clamped, sqrt_pos
        return Path(entry, prec, True, False, False, "direct", False, {"rbf": 0, "matern32": 2, "matern52": 3}[kind],
                    {"rbf": 0, "matern32": 1, "matern52": 4}[kind])
    if entry in INPUT_GRAD_ENTRIES:           # kernels_input_grad.hip, kernels_predict_grad.hip, kernels_input_grad_mid.hip
        return Path(entry, prec, True, False, False, "direct", False, {"rbf": 1, "matern32": 3, "matern52": 4}[kind],
                    {"rbf": 0, "matern32": 1, "matern52": 4}[kind], 0)
    if entry == "grad_multi_mid":             # kernels_grad_multi_mid.hip
        clamp = bool(exp_clamp)
        fold = kind == "rbf" and not clamp
        pr = EXACT if prec == EXACT else FAST
        return Path(entry, pr, clamp, fold, kind != "rbf" and not clamp and pr != EXACT, "gram", False,
                    {"rbf": 0, "matern32": 2, "matern52": 3}[kind] + (1 if fold else 0), {"rbf": 0, "matern32": 1, "matern52": 4}[kind] + (1 if fold else 0), 5)
    raise ValueError(entry)


@dataclass
class PairGeometry:
    """What the tolerance needs of a block of pairs (rows x columns)"""
    D: int
    E: np.ndarray        # reference exponent, hot units, longdouble
    amax: np.ndarray     # max(|xh_i|^2, |xh_j|^2), device operands
    l1: np.ndarray       # |xh_i - xh_j|_1 (hot operands)
    kap: np.ndarray
    h: np.ndarray


def pair_geometry(kind: str, X: np.ndarray, ls: np.ndarray, rows: Optional[np.ndarray] = None) -> PairGeometry:
    R = X if rows is None else rows
    E = exponents(kind, R, X, ls)
    kap, h = profiles(kind, E)
    oc, orow = operands(kind, X, ls), operands(kind, X, ls, R)
    amax = np.maximum(orow.a[:, None], oc.a[None, :])
    l1 = np.zeros(E.shape)
    for d in range(X.shape[1]):
        l1 += np.abs(orow.xh[:, d][:, None] - oc.xh[:, d][None, :])
    return PairGeometry(X.shape[1], E, amax, l1, kap, h)


def d2_of_E(kind: str, E):
    return 2 * E if kind == "rbf" else (E / 2) ** 2


def E_of_d2(kind: str, d2):
    return d2 / 2 if kind == "rbf" else 2 * np.sqrt(np.maximum(d2, 0))


def delta_d2(kind: str, g: PairGeometry, form: str, chain_extra: int = 0):
    """(c): bound of |d2 computed - d2 exact| in hot units^2"""
    d2 = d2_of_E(kind, g.E)
    scaling = 6 * U * d2 + 8 * U * np.sqrt(g.amax) * g.l1
    cancel = (5 * g.D + 3 + chain_extra) * U * g.amax if form == "gram" else (g.D + 3 + chain_extra) * U * d2
    return cancel + scaling


def exponent_interval(kind: str, g: PairGeometry, form: str, chain_extra: int = 0, shift: float = 0.0):
    """[E_lo, E_hi] of the computed exponent; `shift`: a one-sided addition to d2 (the positivity bias of a biased instance)"""
    d2 = d2_of_E(kind, g.E)
    dd = delta_d2(kind, g, form, chain_extra).astype(LD)
    lo, hi = d2 - dd, d2 + dd + LD(shift)
    if kind == "rbf":
        return lo / 2, hi / 2     # the RBF exponent may come out a few ulp positive (devmath.h: harmless, no clamp)
    return E_of_d2(kind, lo), E_of_d2(kind, hi)


def gram_term(kind: str, g: PairGeometry, form: str, which: str, chain_extra: int = 0, shift: float = 0.0):
    Elo, Ehi = exponent_interval(kind, g, form, chain_extra, shift)
    k = 0 if which == "kappa" else 1
    f0 = (g.kap, g.h)[k]
    flo, fhi = profiles(kind, Elo)[k], profiles(kind, Ehi)[k]
    return np.maximum(np.abs(flo - f0), np.abs(fhi - f0))


def root_sensitivity(kind: str, E, which: str, hot_poly: bool):
    """|d value / d root| * root, in units of the variance, for the form the code evaluates"""
    if kind == "rbf":
        return np.zeros(np.shape(E), dtype=LD)
    s = np.asarray(E, dtype=LD) * LD(C_HOT)
    e = exp2_neg_hot(np.asarray(E, dtype=LD))
    if which == "h":
        return 3 * s * e if kind == "matern32" else LD(5) / 3 * s * s * e
    if kind == "matern32":
        return s * s * e
    return (s * s + s ** 3 / 3) * e if hot_poly else s * s * (1 + s) / 3 * e


def level_term(kind: str, g: PairGeometry, p: Path, which: str):
    f0 = g.kap if which == "kappa" else g.h
    e_root = E_ROOT[p.prec] if (p.form == "gram" and not p.tiles) else E_ROOT_POS
    t = (LEVEL_EXP2NEG if p.tiles else LEVEL[p.prec]) * f0 + e_root * root_sensitivity(kind, g.E, which, p.hot_poly)
    if p.fold:
        t = t + LEVEL_EXP2NEG * f0
    return t


def rounding_term(g: PairGeometry, p: Path, which: str):
    return (p.n_round if which == "kappa" else p.n_round_h) * U * (g.kap if which == "kappa" else g.h)


def bias_term(kind: str, p: Path, bias: float) -> float:
    if not p.biased:
        return 0.0
    return 2.0 * C_HOT ** 2 * bias / (1.0 if kind == "matern32" else 3.0)


def floor_value(kind: str, g: PairGeometry, p: Path, which: str):
    """(e): what a clamped instance may return at most where the reference is below 2^-1000 (units of the variance)"""
    _, Ehi = exponent_interval(kind, g, p.form, p.chain_extra)
    s = Ehi * LD(C_HOT)
    if kind == "rbf":
        poly = np.ones(np.shape(s), dtype=LD)
    elif which == "kappa":
        poly = 1 + s if kind == "matern32" else 1 + s + s * s / 3
    else:
        poly = LD(3) * np.ones(np.shape(s), dtype=LD) if kind == "matern32" else LD(5) / 3 * (1 + s)
    n = p.n_round if which == "kappa" else p.n_round_h
    return poly * np.ldexp(LD(1), -FLOOR_OCT) * (1 + 2 * LEVEL[p.prec] + (n + 2) * U)


@dataclass
class Bound:
    tol: np.ndarray        # units of the variance
    floored: np.ndarray    # bool: (e) applies
    floor: np.ndarray


def tolerance(kind: str, g: PairGeometry, p: Path, bias: float = 0.0, which: str = "kappa") -> Bound:
    # kappa: the documented effect of the bias, (d).  h has no documented figure (3 e^-s has a square-root singularity at d2 = 0): the bias
    # widens the upper end of the d2 interval of (c) instead
    shift = bias if (which == "h" and p.biased) else 0.0
    tol = (level_term(kind, g, p, which) + rounding_term(g, p, which) + gram_term(kind, g, p.form, which, p.chain_extra, shift)
           + (bias_term(kind, p, bias) if which == "kappa" else 0.0))
    floored = np.logical_and(p.clamp, g.E > LD(FLOOR_OCT * TAB))
    return Bound(tol, floored, floor_value(kind, g, p, which))


def ratios(dev: np.ndarray, ref, b: Bound, scale=1.0, extra=None) -> np.ndarray:
    """error / tolerance of every element (dev and ref in the same units, `scale` times the variance units of the bound); under (e) the value
    over its floor, infinity for a negative or non-finite one.  `extra`: absolute terms already in dev's units (the rounding of the diagonal)"""
    dev = np.asarray(dev, dtype=LD)
    t = b.tol * LD(scale) + (0 if extra is None else extra)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev == ref, LD(0), np.abs(dev - ref) / t)
    with np.errstate(divide="ignore", invalid="ignore"):
        fl = np.where(dev == 0, LD(0), dev / (b.floor * LD(scale)))
    fl = np.where(dev >= 0, fl, np.inf)
    out = np.where(b.floored, fl, r)
    return np.where(np.isfinite(dev), out, np.inf).astype(np.float64)


def grad_tolerance(kind: str, g: PairGeometry, p: Path, X: np.ndarray, ls: np.ndarray, pairs: np.ndarray, variance: float,
                   bias: float = 0.0, kappa_bound: Optional[Bound] = None, moments: bool = False):
    """(f): reference and tolerance of out[0..D-1] (dK_ij / dl_k) and out[D] (kappa_ij) for the probe pairs [(i, j)]: arrays [P, D + 1].
    kappa_bound: the bound of out[D] where it comes from another path (wide inputs: from a product).  moments: the pass forms delta_k^2 as
    x_i (x_i S0 - 2 S1) + S2 from the moments S0 = hv, S1 = hv x_j, S2 = hv x_j^2 - seven rounded operations (x_i S0, hv x_j, their
    difference, its product with x_i, x_j^2, its product with hv, the final sum), each of size <= hv (|x_i| + |x_j|)^2: the absolute term
    7 u h (|z_ik| + |z_jk|)^2 in place of the relative 3 u of a rounded difference and its square."""
    i, j = pairs[:, 0], pairs[:, 1]
    bh = tolerance(kind, g, p, bias, "h")
    bk = tolerance(kind, g, p, bias, "kappa") if kappa_bound is None else kappa_bound
    c = column_means(X)
    D = X.shape[1]
    ref = np.zeros((len(pairs), D + 1), dtype=LD)
    tol = np.zeros((len(pairs), D + 1), dtype=LD)
    floored = np.zeros((len(pairs), D + 1), dtype=bool)
    floor = np.zeros((len(pairs), D + 1), dtype=LD)
    for k in range(D):
        lk = LD(ls[k])
        dk = (X[i, k].astype(LD) - X[j, k].astype(LD)) / lk
        zz = (np.abs(X[i, k] - c[k]) + np.abs(X[j, k] - c[k])) / ls[k]
        ref[:, k] = LD(variance) * g.h[i, j] * dk * dk / lk
        rnd = g.h[i, j] * ((6 if moments else 9) * U * dk * dk + 4 * U * np.abs(dk) * zz + (7 * U * zz * zz if moments else 0))
        tol[:, k] = LD(variance) / lk * (bh.tol[i, j] * dk * dk + rnd)
        floored[:, k] = bh.floored[i, j]
        floor[:, k] = LD(variance) / lk * bh.floor[i, j] * dk * dk * (1 + 12 * U)
    ref[:, D] = g.kap[i, j]
    tol[:, D] = bk.tol[i, j]
    floored[:, D] = bk.floored[i, j]
    floor[:, D] = bk.floor[i, j]
    return ref, Bound(tol, floored, floor)


# Rounded operations between the evaluator's h and a gradient entry of the input-gradient products, and the relative error of the operands' common
# scale - the c of `input_grad_tolerance`.  KSCALE_U: cglb_kscale in double (sqrt(LOG2E), or a rounded sqrt(2 nu) times LOG2E: at most two rounded
# constants and one rounded operation).
#   every entry    df = xi - xj (or the fmac with -1: rounded once) [1];  t = h * 1 exact, fma(t, df, 0) [1];  the finish kernel's scale * s [1];
#                  the operands' common scale s_k = fl(kscale hot / l_k): 3 u (kernels_prep.hip; section (c))
#   narrow, weighted   the scale gs.g[k] = -var / (l_k * (kscale hot)) of row_slab_cross_grad_scale: kscale hot is exact in the power of two, l_k * ks [1],
#                  the division [1], kscale itself [KSCALE_U]; the weighted finish multiplies it by gscale = 1 first: exact
#   mid width      (gfac * scale[k]) * s with gfac = -var / (ks * ks * hot) (ks * ks [1], the division [1], kscale twice [2 KSCALE_U]), scale[k] = ks / l_k
#                  of upload_scales (kscale [KSCALE_U], the division [1]) and their product [1]
# (kscale's error cancels between s_k and the scale, in exact arithmetic; it is counted on both sides as if it did not.)
KSCALE_U = 3
INPUT_GRAD_ROUNDINGS = {"cross_grad": 3 + 3 + (2 + KSCALE_U), "cross_grad_weighted": 3 + 3 + (2 + KSCALE_U),
                        "cross_grad_mid": 3 + 3 + (2 + 2 * KSCALE_U) + (1 + KSCALE_U) + 1}


def input_grad_tolerance(kind: str, g: PairGeometry, p: Path, Xrow: np.ndarray, X: np.ndarray, ls: np.ndarray, k: int, bh: Optional[Bound] = None,
                         idx: Optional[Tuple[np.ndarray, np.ndarray]] = None):
    """Coordinate k of the input gradient of the cross products, in units of the variance f: with delta_k = (x*_ik - x_jk) / l_k
        gout[i, j, k] = -f h_ij delta_k / l_k,     bound   f / l_k (tol_h |delta_k| + h (c u |delta_k| + 2 u (|z_ik| + |z_jk|))),   z = (x - centre) / l:
    the evaluator's bound on h (`tolerance(which="h")` of the path; pass it as `bh` to compute it once for all k) times |delta_k|; c =
    INPUT_GRAD_ROUNDINGS[p.name] rounded operations and the common scale's relative error, each acting on the whole entry; and the operands' own
    rounding xh = fl(fl(x - c) s_k), 2 u |z| each (kernels_prep.hip), which the difference of the two operands inherits absolutely.
    Returns (ref [rows, N], Bound, sign [rows, N]) with sign = -sign(delta_k).  Under the clamp floor (e) the sign is folded into both sides: compare
    sign * device with sign * ref through `ratios`, which then asks 0 <= sign * device <= floor_h |delta_k| / l_k and keeps rejecting a wrong-signed or
    non-finite value.  sign = 0 marks x*_ik == x_jk as doubles: both operands are then the same double, the difference is exactly zero and so must the entry
    be - the caller asserts that on the device value itself.  idx = (rows, columns): those pairs alone, as 1-D arrays (most pairs of a set have
    x*_ik == x_jk off the sweep's coordinate)."""
    bh = tolerance(kind, g, p, 0.0, "h") if bh is None else bh
    c = column_means(X)
    lk = LD(ls[k])
    if idx is None:
        xr, xc = Xrow[:, k][:, None], X[:, k][None, :]
        h, th, fh, flo = g.h, bh.tol, bh.floor, bh.floored
    else:
        xr, xc = Xrow[idx[0], k], X[idx[1], k]
        h, th, fh, flo = g.h[idx], bh.tol[idx], bh.floor[idx], bh.floored[idx]
    dk = (xr.astype(LD) - xc.astype(LD)) / lk
    ad = np.abs(dk)
    zz = (np.abs(xr - c[k]) + np.abs(xc - c[k])) / ls[k]
    cnt = INPUT_GRAD_ROUNDINGS[p.name]
    ref = -h * dk / lk
    tol = (th * ad + h * (cnt * U * ad + 2 * U * zz)) / lk
    # the floor of h times the LARGEST |delta_k| the device can have formed: its c roundings and the operands' own, as in the tolerance
    floor = fh * (ad * (1 + (cnt + 2) * U) + 2 * U * zz) / lk
    return ref, Bound(tol, flo, floor), -np.sign(dk).astype(np.float64)


def input_grad_ratios(kind: str, g: PairGeometry, p: Path, Xrow: np.ndarray, X: np.ndarray, ls: np.ndarray, k: int, bh: Bound, dev: np.ndarray,
                      scale: float = 1.0) -> Tuple[np.ndarray, int]:
    """error / tolerance of coordinate k of a gradient [rows, N] (`scale` times the variance units of the bound) and the number of pairs with
    x*_ik == x_jk, whose entries must be exactly zero (asserted); the reference is formed for the other pairs alone"""
    same = Xrow[:, k][:, None] == X[:, k][None, :]
    assert np.all(dev[same] == 0.0), f"coordinate {k}: a pair of equal coordinates returned a non-zero gradient entry"
    idx = np.nonzero(~same)
    ref, b, sg = input_grad_tolerance(kind, g, p, Xrow, X, ls, k, bh, idx)
    r = np.zeros(dev.shape)
    r[idx] = ratios(dev[idx] * sg, ref * LD(scale) * sg, b, scale=scale)
    return r, int(same.sum())


def floored_cap(case: Case, N: int) -> int:
    """Most elements of a cross matrix (rows: the set and five points off it; the row at 1e3 apart) that may go without a relative check, by the case
    table's own range figures.  A row whose largest exponent stays below 1000 octaves has none: the five off-set points lie inside the box of the
    set.  RBF oct 2400 and 1200 (rows D, F77): centre and sweep are at a quarter of the corners' exponent from a corner, so only the corner pairs
    (1, 2), (3, 2) and their mirrors, and what the five off-set rows add.  Matern oct 2400 (row D; the exponent is linear in the distance): the
    three corner rows and columns against everything, and the off-set rows."""
    if set_statistics(case)["max_oct"] < FLOOR_OCT:
        return 0
    return 4 + 5 * N if case.kind == "rbf" else 6 * N + 5 * N


def probe_pairs(case: Case, n_int=32, n_rand=32, n_near=16, n_same=8, n_far=8) -> np.ndarray:
    """about 96 probe pairs of a set: near-integer exponents, random, nearest neighbours, coincident (i = i), farthest"""
    X, ls = build_set(case)
    N = X.shape[0]
    E = exponents(case.kind, X, X, ls).astype(np.float64)
    rng = np.random.default_rng(7 + case.D)
    frac = np.abs(E - np.rint(E))
    iu = np.triu_indices(N, 1)
    cand = np.flatnonzero((frac[iu] < 1e-6) & (E[iu] > 0.5))
    pick = rng.choice(cand, size=min(n_int, len(cand)), replace=False)
    pairs = [(iu[0][q], iu[1][q]) for q in pick]
    pairs += [tuple(rng.choice(N, size=2, replace=False)) for _ in range(n_rand)]
    Eo = E + np.where(np.eye(N, dtype=bool), np.inf, 0.0)
    near = np.argsort(Eo[iu])[:n_near]
    pairs += [(iu[0][q], iu[1][q]) for q in near]
    pairs += [(q, q) for q in rng.choice(N, size=n_same, replace=False)]
    far = np.argsort(-E[iu])[:n_far]
    pairs += [(iu[0][q], iu[1][q]) for q in far]
    return np.array(pairs, dtype=np.int64)


# ---- checks of the layout ----------------------------------------------------------------------------------------------------------------
def set_statistics(case: Case) -> Dict[str, float]:
    X, ls = build_set(case)
    E = exponents(case.kind, X, X, ls)
    n = np.floor(-E)                       # the device's n = floor(x), x = -E
    idx = (n.astype(np.int64) & (TAB - 1))
    Ef = E.astype(np.float64)
    k = np.rint(Ef)
    off = (E - k.astype(LD)).astype(np.float64)
    r = regime_details(case.kind, X, ls)
    return {"N": X.shape[0], "indices": int(len(np.unique(idx))), "above": int(np.sum((off > 0) & (off < 1e-6) & (k > 0))),
            "below": int(np.sum((off < 0) & (off > -1e-6) & (k > 0))), "exact": int(np.sum((np.abs(off) < 1e-10) & (k > 0))),
            "max_oct": float(E.max() / TAB), "oct": r.oct, "s2": r.s2, "exp_clamp": int(r.exp_clamp), "m32_bias": r.m32_bias,
            "int_ok": int(r.int_ok)}


def check_set(case: Case) -> Dict[str, float]:
    st = set_statistics(case)
    assert st["N"] % 16 != 0, "the ragged tail and every position of the 4/2/1 batches must carry designed pairs"
    assert st["indices"] == TAB, st
    assert st["above"] >= 100 and st["below"] >= 100, st
    assert abs(st["max_oct"] / st["oct"] - 1.0) <= 0.01, st
    assert st["exp_clamp"] == case.clamp, st
    return st


# ---- float64 emulation of the table form, and the defects the checks must reject -----------------------------------------------------------
DEFECTS = ("table_entry", "round_nearest", "octave_shift", "m52_quadratic", "low_tail")


@lru_cache(maxsize=None)
def poly_coefficients(prec: int) -> Tuple[float, ...]:
    """P(s) ~ 2^((s - 1/2)/256) on [0, 1): degree 4 / 3 / 2, fitted by the tool that made devmath.h's constants (ascending)"""
    import mpmath as mp
    from tools.exp2_poly_fit import fit
    deg = {EXACT: 4, FAST: 3, LOW: 2}[prec]
    c = fit(lambda s: mp.mpf(2) ** ((s - mp.mpf(0.5)) / TAB), mp.mpf(0), mp.mpf(1), deg)
    return tuple(float(x) for x in c)


def table() -> np.ndarray:
    return np.exp2((np.arange(TAB) + 0.5) / TAB)


def _poly(prec: int, s: np.ndarray) -> np.ndarray:
    c = poly_coefficients(prec)
    p = np.full(s.shape, c[-1])
    for q in c[-2::-1]:
        p = fma(p, s, q)
    return p


def emulate(kind: str, X: np.ndarray, ls: np.ndarray, p: Path, bias: float = 0.0, defect: Optional[str] = None,
            rows: Optional[np.ndarray] = None, which: str = "kappa") -> np.ndarray:
    """kappa (or h) of every pair [rows, N] in units of the variance as the Gram-form pair stream computes it, in float64 NumPy"""
    assert defect is None or defect in DEFECTS
    oc = operands(kind, X, ls)
    orow = oc if rows is None else operands(kind, X, ls, rows)
    D = X.shape[1]
    mat = kind != "rbf"
    b = bias if p.biased else 0.0
    seed = -0.5 * (orow.a + b) if mat else -0.5 * orow.a
    aj = oc.a if mat else -0.5 * oc.a
    gram = np.repeat(seed[:, None], oc.xh.shape[0], axis=1)
    for d in range(D):
        gram = fma(orow.xh[:, d][:, None], oc.xh[:, d][None, :], gram)
    lin = np.ones(gram.shape)
    if mat:
        d2 = fma(-2.0, gram, aj[None, :])
        x = 2.0 * np.sqrt(np.maximum(d2, 1e-280))           # sqrt_hot: twice the root
        if which == "kappa":
            if kind == "matern32":
                lin = fma(x, C_HOT, 1.0)
            elif defect == "m52_quadratic":
                lin = fma(x, C_HOT, 1.0)
            elif p.hot_poly:
                lin = fma(x, C_HOT, fma(d2, 4.0 * C_HOT * C_HOT / 3.0, 1.0))
            else:   # the Horner form of the exponent's root (matern_kpoly: the mid-width multi-pair gradient pass)
                lin = fma(x, fma(x, C_HOT * C_HOT / 3.0, C_HOT), 1.0)
        else:
            lin = np.full(gram.shape, 3.0) if kind == "matern32" else (5.0 / 3.0) * fma(x, C_HOT, 1.0)
        if p.clamp:
            x = np.minimum(x, float(FLOOR_OCT * TAB))
        x = -x
    else:
        x = gram if p.fold else gram + aj[None, :]
        if p.clamp:
            x = np.maximum(x, -float(FLOOR_OCT * TAB))
    if p.tiles:   # no table: 2^x of the scaled units (np.exp2 stands for exp2_neg), the Horner polynomial of the root
        if mat and which == "kappa":
            r = -x
            lin = fma(r, C_HOT, 1.0) if kind == "matern32" else fma(r, fma(r, C_HOT * C_HOT / 3.0, C_HOT), 1.0)
        return lin * np.exp2(np.minimum(x, 0.0) / TAB) if mat else np.exp2(np.minimum(x, 0.0) / TAB)
    n = np.floor(x)
    s = x - n                                                # v_fract_f64: exact
    if defect == "round_nearest":
        n = np.rint(x)                                       # the fraction still comes from fract
    ni = n.astype(np.int64)
    tab = table()
    if defect == "table_entry":
        tab = tab.copy()
        tab[137] *= 1.0 + 1e-11
    octave = ni >> 8
    if defect == "octave_shift":
        octave = np.trunc(x).astype(np.int64) >> 8
    poly = _poly(p.prec, s)
    if defect == "low_tail":
        N = X.shape[0]
        tail = np.arange(N) >= N - N % 16
        poly = np.where(tail[None, :], _poly(LOW, s), poly)
    val = np.ldexp(tab[ni & (TAB - 1)] * (poly * lin if mat else poly), octave)
    if p.fold:
        val = val * np.exp2(aj / TAB)[None, :]
    return val


def moment_grad_entry(kind: str, X: np.ndarray, ls: np.ndarray, hv: np.ndarray, k: int) -> np.ndarray:
    """out[k] of the mid-width Gram gradient passes for U = e_i, V = e_j, every (i, j) at once, in units of the variance: the moment form
    x_i (x_i S0 - 2 S1) + S2 with S0 = hv, S1 = hv x_j, S2 = hv x_j^2 in the hot operands, then the finish kernel's 1 / hot^2 and 1 / (l_k kscale^2).
    hv: h of `emulate` (which="h") on the pass's path, which carries the kind's constant."""
    oc = operands(kind, X, ls)
    xi, xj = oc.xh[:, k][:, None], oc.xh[:, k][None, :]
    s1 = hv * xj
    s2 = hv * (xj * xj)
    val = xi * (xi * hv - 2.0 * s1) + s2
    ks = kscale(kind)
    return (val * (1.0 / (hot_scale(kind) * hot_scale(kind)))) * (1.0 / (ls[k] * ks * ks))


# ---- the direct form of the input-gradient products (kappa_hfac_hot_from_d2), and the defects only a read-out in every slot and part can see --------
DIRECT_DEFECTS = ("part_dropped", "h_for_kappa")                             # of a pair's value: `emulate_direct`
READOUT_DEFECTS = ("column_swapped", "orientation_dropped", "slot_crosstalk")  # of the weights a value meets: `swap_columns`, `multi_pair_model`


def direct_operands(kind: str, X: np.ndarray, ls: np.ndarray, rows: Optional[np.ndarray] = None) -> Tuple[Operands, Operands]:
    """(row side, column side) of the staged hot operands of a cross product: pass as `ops` to spare their recomputation per coordinate"""
    oc = operands(kind, X, ls)
    return (oc if rows is None else operands(kind, X, ls, rows)), oc


def emulate_direct(kind: str, X: np.ndarray, ls: np.ndarray, p: Path, rows: Optional[np.ndarray] = None, which: str = "kappa", k: int = 0,
                   defect: Optional[str] = None, part: int = 0, ops: Optional[Tuple[Operands, Operands]] = None) -> np.ndarray:
    """kappa, h (which = "kappa" | "h") or coordinate k of the input gradient (which = "grad") of every pair [rows, N], in units of the variance, as
    cross_grad_kernel / weighted_grad_kernel / cross_grad_mid_kernel compute it, in float64 NumPy: differences of the staged hot operands, the fma
    chain of d2 (mid width: four lane parts of Dh / 4 coordinates, each two interleaved chains, then the sums of sum_row_pairs and sum_halves),
    rT = 2 sqrt(d2) (np.sqrt stands for sqrt_pos), the Horner polynomials of that root, the table step of `emulate` on the clamped exponent, and the
    scale of the finish kernel.  Defects: part_dropped - d2 misses the partial of lane part `part`; h_for_kappa - the value takes h's polynomial."""
    assert p.form == "direct" and (defect is None or defect in DIRECT_DEFECTS)
    orow, oc = direct_operands(kind, X, ls, rows) if ops is None else ops
    D = X.shape[1]
    shape = (orow.xh.shape[0], oc.xh.shape[0])
    sq = lambda d, acc: (lambda df: fma(df, df, acc))(orow.xh[:, d][:, None] - oc.xh[:, d][None, :])
    if p.name == "cross_grad_mid":
        hd = hot_width(D) // 4
        parts = []
        for q in range(4):
            a, b = np.zeros(shape), np.zeros(shape)
            for d in range(q * hd, min((q + 1) * hd, D)):   # the zero padding adds exactly zero
                if (d - q * hd) % 2 == 0:
                    a = sq(d, a)
                else:
                    b = sq(d, b)
            parts.append(np.zeros(shape) if (defect == "part_dropped" and q == part) else a + b)
        d2 = (parts[0] + parts[1]) + (parts[2] + parts[3])
    else:
        assert defect != "part_dropped"
        d2 = np.zeros(shape)
        for d in range(D):
            d2 = sq(d, d2)
    if kind == "rbf":
        x = -0.5 * d2
        kp = hp = np.ones(shape)
    else:
        rT = 2.0 * np.sqrt(d2)
        x = -rT
        lin = fma(rT, C_HOT, 1.0)
        kp = lin if kind == "matern32" else fma(rT, fma(rT, C_HOT * C_HOT / 3.0, C_HOT), 1.0)
        hp = np.full(shape, 3.0) if kind == "matern32" else (5.0 / 3.0) * lin
    x = np.maximum(x, -float(FLOOR_OCT * TAB))
    n = np.floor(x)
    ni = n.astype(np.int64)
    e = np.ldexp(table()[ni & (TAB - 1)] * _poly(p.prec, x - n), ni >> 8)
    hv = e if kind == "rbf" else hp * e
    kv = hv if (kind == "rbf" or defect == "h_for_kappa") else kp * e
    if which == "kappa":
        return kv
    if which == "h":
        return hv
    return direct_grad_entry(kind, X, ls, p, rows, hv, k, (orow, oc))


def direct_grad_entry(kind: str, X: np.ndarray, ls: np.ndarray, p: Path, rows: Optional[np.ndarray], hv: np.ndarray, k: int,
                      ops: Optional[Tuple[Operands, Operands]] = None) -> np.ndarray:
    """coordinate k of the input gradient from the h of `emulate_direct` (units of the variance): the rounded difference, its product with h, the scale
    as the finish kernel of the path forms it"""
    orow, oc = direct_operands(kind, X, ls, rows) if ops is None else ops
    ks = kscale(kind)
    acc = hv * (orow.xh[:, k][:, None] - oc.xh[:, k][None, :])
    if p.name == "cross_grad_mid":
        return ((-1.0 / (ks * ks * hot_scale(kind))) * (ks / ls[k])) * acc
    return (-1.0 / (ls[k] * (ks * hot_scale(kind)))) * acc


def group_width(entry: str, D: int) -> int:
    """columns per group of the input-gradient cross products (row_slab.h: input_grad_group_width, input_grad_mid_group)"""
    if entry == "cross_grad_mid":
        return 4 if hot_width(D) <= 64 else 2
    return 8 if D <= 8 else (4 if D <= 16 else 2)   # the padded width passes 8 and 16 where D does


def swap_columns(M: np.ndarray, G: int) -> np.ndarray:
    """column_swapped: what the identity read-out returns when columns b and b ^ 1 of a group of G exchange their weights (a short last group
    keeps an unpaired last column)"""
    out = M.copy()
    n = M.shape[1]
    for j in range(n):
        j1 = j ^ 1
        if G > 1 and j1 < n and j1 // G == j // G:
            out[:, j] = M[:, j1]
    return out


MULTI_S = (1, 2, 4, 5, 8, 9, 10)   # single pass; groups padded to 4 and to 8; 8 + a left-over single pass; 8 + a group of 2


def multi_block_rows(D: int) -> int:
    """rows of a workgroup of the mid-width multi-pair gradient pass (grad_pass.h: 256 / grad_multi_mid_split)"""
    return 64 if hot_width(D) == 96 else 128


def multi_single_slot(S: int, slot: int, native: bool = True) -> bool:
    """whether pair `slot` of S goes through the single pass of kernels_grad_mid.hip (launch_grad_kff_multi: groups of 8 in order, a single left-over
    pair last; S = 1; every pair where the multi-pair instance is switched off)"""
    return (not native) or S == 1 or (S % 8 == 1 and slot == S - 1)


def multi_probe(N: int, S: int, q: int, i: int, j: int, swap: bool) -> Tuple[np.ndarray, np.ndarray, int]:
    """U, V [S, N] of probe q for the pair (i, j): the unit vectors in slot q % S (U = e_i, V = e_j; swap: U = e_j, V = e_i), every other slot a
    non-zero U with V = 0 or the reverse, alternating - all their true terms are exact zeros, cross-talk between slots is not"""
    slot = q % S
    Um, Vm = np.zeros((S, N)), np.zeros((S, N))
    for t in range(S):
        if t != slot:
            (Um if t % 2 == 0 else Vm)[t, :] = 1.0 + 0.25 * (t + 1)
    a, c = (j, i) if swap else (i, j)
    Um[slot, a] = 1.0
    Vm[slot, c] = 1.0
    return Um, Vm, slot


def multi_pair_model(M: np.ndarray, Um: np.ndarray, Vm: np.ndarray, brows: int, defect: Optional[str] = None) -> float:
    """sum_ij M_ij w_ij with the pair weight of kernels_grad_multi_mid.hip: the columns at or right of a row's block are visited; inside the diagonal
    block w_ij = sum_b u_bi v_bj, to its right w_ij = sum_b (u_bi v_bj + v_bi u_bj).  M: any symmetric per-pair quantity (kappa, h delta_k^2).
    Defects: orientation_dropped - the second half is lost; slot_crosstalk - u_b meets v_{b+1} (cyclically) instead of v_b."""
    assert defect is None or defect in READOUT_DEFECTS
    N = M.shape[0]
    blk = np.arange(N) // brows
    Vu = np.roll(Vm, -1, axis=0) if defect == "slot_crosstalk" else Vm
    w1 = Um.T @ Vu
    w2 = np.zeros((N, N)) if defect == "orientation_dropped" else w1.T
    w = np.where(blk[None, :] == blk[:, None], w1, np.where(blk[None, :] > blk[:, None], w1 + w2, 0.0))
    return float((M * w).sum())


def probe_pairs_blocks(case: Case) -> np.ndarray:
    """`probe_pairs`, and pairs inside one row block of 64 of the multi-pair pass and across two, in both orders: the pair weight differs between the
    diagonal block and the blocks to its right"""
    extra = [(5, 60), (60, 5), (70, 120), (130, 200), (10, 70), (70, 10), (63, 64), (64, 63), (127, 128), (128, 127), (6, 270), (270, 6), (200, 259),
             (259, 200), (257, 275), (275, 257)]
    return np.concatenate([probe_pairs(case), np.array(extra, dtype=np.int64)], axis=0)


# ---- shared, read-only pieces of the GPU tests ----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def set_geometry(case: Case, cross: bool = False) -> PairGeometry:
    """reference and geometry of a set (cross: rows = new_points), computed once and shared"""
    X, ls = build_set(case)
    return pair_geometry(case.kind, X, ls, new_points(case) if cross else None)


def locate(case: Case, g: PairGeometry, r: np.ndarray, floored: Optional[np.ndarray] = None) -> str:
    """where the worst error / tolerance occurred: pair, reference exponent in hot units, table index, fractional part; the elements under the
    clamp floor (value / floor, no relative check) are reported on their own"""
    fl = np.zeros(r.shape, dtype=bool) if floored is None else floored
    rr = np.where(fl, 0.0, r)
    w = np.unravel_index(int(np.argmax(rr)), rr.shape)
    E = g.E[w]
    n = np.floor(-E)
    txt = (f"worst error / tolerance {float(rr[w]):.3f} at pair ({int(w[0])}, {int(w[1])}), E = {float(E):.9f} hot units, "
           f"table index {int(n) & (TAB - 1)}, fraction {float(-E - n):.3e}")
    if fl.any():
        txt += f"; {int(fl.sum())} elements under the clamp floor, largest value / floor {float(np.where(fl, r, 0.0).max()):.3f}"
    return txt
