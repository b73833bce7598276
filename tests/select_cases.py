"""Cases and references of the greedy inducing-point selection (test helper, not a test module; runs on any CPU).

`cglb_select_inducing` (csrc/kernels_select.hip) is a pivoted Cholesky of K_ff: a discrete, path-dependent rule.  In fp32, and at near-ties in
fp64, the library's picks legitimately differ from any reference's, so an index comparison says nothing there.  What holds on every path:

  * path follower (`follow`): along the LIBRARY's picks j_0 .. j_{M-1}, recompute in np.longdouble the conditional variances d_ref^(m) before
    every pick.  regret_m = max_i d_ref^(m)[i] - d_ref^(m)[j_m]; a pick is right when regret_m <= tol.  Where the gap to the runner-up exceeds
    tol this is "equals the arg-max"; no step is left out.  sum d_ref after the last step is the reference of the reported trace;
  * working-precision restatement (`restate`): the kernel's data flow in np.float32 / np.float64 - centred, scaled coordinates rounded to the
    working type, differences, d2, the kernel value in the working type, e = (col - C[:m]^T C[:m, j]) / sqrt(d_j), d = max(d - e^2, 0),
    d[j] = 0, lowest index on ties.  fp32 inputs go through fp32_error_model.f32 first.  It supplies the round-off scale and, with one of the
    DEFECTS switched on, the wrong pick sequences the checks have to reject (tests/test_select_cases_host.py).

Tolerance of an instance (case, kind, dtype), `tol(inst)`:

    tol = 4 * E_ref * eps_T * variance  +  kernel-value term

  * E_ref: the largest |d_T - d_longdouble| over all steps and points, restatement in T against the follower on the restatement's own path, in
    units of eps_T * variance.  Stored per instance in `E_REF` (a constant; the host test asserts measurement <= constant <= 2 * measurement).
    THE STORED CONSTANT IS 1.5 TIMES THE MEASUREMENT (`HEADROOM`), the middle of that bracket: the maximum over all steps and points moves with
    the last-bit rounding of the host's exp2 / sqrt, and a constant at the measurement would fall out of the bracket on another CPU.  The
    tolerance is therefore 6 times the measured round-off, not 4; DESIGN.md lists measured and stored values side by side;
    The margin of 4: the kernel sums the dot product in eight interleaved fma chains and rounds sqrt / division differently from numpy - an
    error of the same order, not the same number;
  * kernel-value term, fp64: variance * 1e-13, the relative error include/cglb_hip.h states for the evaluator at the default "precision" level.
    The selection kernel takes direct differences (kappa_from_d2), so the Gram-form term that header adds for the N^2 products does not apply;
  * kernel-value term, fp32: the largest difference between the float32 restatement's kernel columns and the fp64 oracle's on the rounded inputs,
    stored per instance in `KV32` the same way (units of eps_32 * variance, same bracket, the same factor 1.5).

Next to the tolerance, what is exact on the device is asserted exactly (`exact_violations`): the first pick is row 0, duplicate rows are taken
lowest index first, the trace is not negative and is zero once all N rows are picked.  The last two are what rejects a missing clamp and a pivot
that is not zeroed: both stay inside the tolerance on every shape (tests/test_select_cases_host.py has the figures).

The 90 % condition (generic, wide and edge cases: exactly one admissible candidate) is counted over the steps after the first, where all d are
equal on every path.  With lengthscales 0.7 + U(0, 1) it cannot hold for RBF or fp32 at D >= 17 (every step is a many-way near-tie); G4-G6 carry
the kinds and types that keep it, and G2s-G6s run the same shapes with lengthscales sqrt(D) (0.7 + U(0, 1)) - the remedy of the wide cases - in every
kind and both types, so that every padded width is selected on in all six combinations.

Case table (every N <= 3001, M <= 300; `check_geometry` asserts what each row claims):

  G1-G6  seeded normal X, lengthscales 0.7 + U(0, 1), variance 1.7.  D 3 5 9 17 27 32: the padded widths 3 6 10 20 28 32, i.e. both sides of every
         padding rule; N 255 256 257 513 1000 2999: one block less a row, one block, one block and a row, two and a row, a partial fourth, many;
         M 7 8 9 16 17 64: both sides of the 8-step unroll of the dot product; jitter 1e-12 and 1e-6 alternating.  D is paired with N and M as
         (3, 257, 16) (5, 255, 7) (9, 256, 64) (17, 1000, 8) (27, 513, 9) (32, 2999, 17): of all pairings the one that keeps most kinds and types.  All three kinds, both dtypes -
         fp32 only where the float32 path keeps 90 % of its steps at a single admissible candidate (INSTANCES)
  W1-W3  D 33 40 100, N 513, M 16, lengthscales sqrt(D) (0.7 + U(0, 1)): select_impl<T, KIND, 0>, the run-time width on unpadded operands
  E1     a tight cluster plus isolated points planted at rows 0 63 64 255 256 257 N-2 N-1, N = 600 and N = 513 (row 512 alone in the last block), at
         graded radii so that the path visits them in an order that is not the row order
  T1     exact ties: 40 distinct rows, each at i, i + 64, i + 256 and 512 + i (the last, partial block of N = 552): the same lane of other waves
         and blocks.  Rows 0 .. 23 once more at 40 .. 63 and at 296 .. 319, inside a wave that already holds a copy, so that the lowest-index rule of
         the wave shuffle itself sees equal values.  Other rows distinct
  X1     exhaustion (exempt from the 90 % condition): RBF N 300 D 2 M 200 at jitter 1e-6 and 1e-12; Matern-3/2 M = N = 300
  O1     M = N + 5 on a sparse-class context (N 61, M 66): min(M, N) picks, all distinct, nothing left
  J1     jitter 0, 1e-12, 1e-6, 1e-2 on one generic shape
  I1     the iterative exact-GP class re-selects its preconditioner at every evaluation: N 257, D 3, k 9, jitter 1e-6, the same data under two
         sets of hyper-parameters (I1b: lengthscales 0.45 times I1a's, variance 0.8)
  S1, H1 reuse generic shapes; they are GPU-side assertions (tests/test_gpu_select_paths.py)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

import fp32_error_model as em
import matern52_ref as m52
from oracle import cglb_oracle as orc

LD = np.longdouble
KINDS = ("rbf", "matern32", "matern52")
KV64 = 1e-13                         # include/cglb_hip.h, "precision": kernel values to <= ~1e-13 relative at the default level
PAD_SIZES = em.PAD_SIZES             # cglb_internal.h: pad_dim
PLANTED = (0, 63, 64, 255, 256, 257, -2, -1)
HEADROOM = 1.5                       # stored E_REF / KV32 over their measurements (see above)
MIN_SINGLE = 0.9                     # share of steps with exactly one admissible candidate, generic / wide / edge cases


def pad_dim(D: int) -> int:
    return next((p for p in PAD_SIZES if p >= D), D)


def eps_of(dtype) -> float:
    return float(np.finfo(dtype).eps)


# --------------------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    name: str
    data: str            # normal | wide | edges | ties
    N: int
    D: int
    M: int
    jitter: float
    seed: int
    exhaust: bool = False   # exempt from the 90 % condition: regret, range, finiteness and trace only
    ls_scale: float = 1.0   # normal data: the lengthscales are ls_scale (0.7 + U(0, 1)) ...
    var: float = 1.7        # ... and this is the variance
    sqrt_d: bool = False    # normal data: the lengthscales carry sqrt(D) (the remedy of the wide cases, at a padded width)


CASES: Dict[str, Case] = {c.name: c for c in (
    Case("G1", "normal", 257, 3, 16, 1e-12, 1),
    Case("G2", "normal", 255, 5, 7, 1e-6, 2),
    Case("G3", "normal", 256, 9, 64, 1e-12, 3),
    Case("G4", "normal", 1000, 17, 8, 1e-6, 4),
    Case("G5", "normal", 513, 27, 9, 1e-12, 5),
    Case("G6", "normal", 2999, 32, 17, 1e-6, 6),
    Case("G2s", "normal", 255, 5, 7, 1e-6, 2, sqrt_d=True),
    Case("G3s", "normal", 256, 9, 64, 1e-12, 3, sqrt_d=True),
    Case("G4s", "normal", 1000, 17, 8, 1e-6, 4, sqrt_d=True),
    Case("G5s", "normal", 513, 27, 9, 1e-12, 5, sqrt_d=True),
    Case("G6s", "normal", 2999, 32, 17, 1e-6, 6, sqrt_d=True),
    Case("W1", "wide", 513, 33, 16, 1e-12, 11),
    Case("W2", "wide", 513, 40, 16, 1e-6, 12),
    Case("W3", "wide", 513, 100, 16, 1e-12, 13),
    Case("E1a", "edges", 600, 2, 16, 1e-12, 21),
    Case("E1b", "edges", 513, 2, 16, 1e-6, 22),
    Case("T1", "ties", 552, 3, 64, 1e-12, 31),
    Case("X1a", "normal", 300, 2, 200, 1e-6, 41, exhaust=True),
    Case("X1b", "normal", 300, 2, 200, 1e-12, 41, exhaust=True),
    Case("X1c", "normal", 300, 2, 300, 0.0, 41, exhaust=True),
    Case("O1", "normal", 61, 3, 66, 1e-12, 51),
    Case("J1-0", "normal", 513, 3, 17, 0.0, 61),
    Case("J1-12", "normal", 513, 3, 17, 1e-12, 61),
    Case("J1-6", "normal", 513, 3, 17, 1e-6, 61),
    Case("J1-2", "normal", 513, 3, 17, 1e-2, 61),
    Case("I1a", "normal", 257, 3, 9, 1e-6, 71),
    Case("I1b", "normal", 257, 3, 9, 1e-6, 71, ls_scale=0.45, var=0.8),
)}


@dataclass(frozen=True)
class Inst:
    case: str
    kind: str
    dtype: str   # "f64" | "f32"

    @property
    def id(self) -> str:
        return f"{self.case}-{self.kind}-{self.dtype}"

    @property
    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32


def _i(case, kind, dtype):
    return Inst(case, kind, dtype)


# (case, kind, dtype) and the measured constants: E_ref [eps_T variance], KV32 [eps_32 variance] (None for fp64)
_TABLE: List[Tuple[str, str, str, float, Optional[float]]] = [
    ("G1", "rbf", "f64", 4.76, None),
    ("G1", "rbf", "f32", 4.4, 1.45),
    ("G1", "matern32", "f64", 4.25, None),
    ("G1", "matern32", "f32", 3.88, 1.9),
    ("G1", "matern52", "f64", 5.31, None),
    ("G1", "matern52", "f32", 4.49, 1.74),
    ("G2", "rbf", "f64", 2.21, None),
    ("G2", "matern32", "f64", 2.16, None),
    ("G2", "matern32", "f32", 2.11, 1.27),
    ("G2", "matern52", "f64", 2.05, None),
    ("G2", "matern52", "f32", 1.96, 1.24),
    ("G3", "rbf", "f64", 6.55, None),
    ("G3", "matern32", "f64", 6.92, None),
    ("G3", "matern32", "f32", 7.05, 1.06),
    ("G3", "matern52", "f64", 5.43, None),
    ("G3", "matern52", "f32", 6.51, 1.32),
    ("G4", "matern32", "f64", 2.74, None),
    ("G2s", "rbf", "f32", 3.69, 1.41),
    ("G3s", "rbf", "f32", 7.12, 1.59),
    ("G4s", "rbf", "f64", 2.85, None),
    ("G4s", "rbf", "f32", 2.89, 1.54),
    ("G4s", "matern32", "f64", 2.96, None),
    ("G4s", "matern32", "f32", 2.57, 1.65),
    ("G4s", "matern52", "f64", 2.9, None),
    ("G4s", "matern52", "f32", 3.48, 1.64),
    ("G5s", "rbf", "f64", 3.02, None),
    ("G5s", "rbf", "f32", 3.13, 1.55),
    ("G5s", "matern32", "f64", 3.38, None),
    ("G5s", "matern32", "f32", 3.08, 1.74),
    ("G5s", "matern52", "f64", 3.26, None),
    ("G5s", "matern52", "f32", 3.24, 1.68),
    ("G6s", "rbf", "f64", 4.49, None),
    ("G6s", "rbf", "f32", 3.9, 1.76),
    ("G6s", "matern32", "f64", 5.09, None),
    ("G6s", "matern32", "f32", 3.88, 1.64),
    ("G6s", "matern52", "f64", 3.63, None),
    ("G6s", "matern52", "f32", 4.32, 2.05),
    ("G5", "matern32", "f64", 2.52, None),
    ("G5", "matern52", "f64", 2.97, None),
    ("G6", "matern32", "f64", 3.77, None),
    ("W1", "rbf", "f64", 3.46, None),
    ("W1", "rbf", "f32", 3.49, 1.89),
    ("W2", "matern32", "f64", 3.96, None),
    ("W2", "matern32", "f32", 4.25, 1.67),
    ("W3", "matern52", "f64", 3.88, None),
    ("W3", "matern52", "f32", 3.08, 2.95),
    ("E1a", "rbf", "f64", 8.18, None),
    ("E1a", "matern32", "f32", 7.28, 2.43),
    ("E1b", "matern52", "f64", 8.85, None),
    ("E1b", "rbf", "f64", 8.61, None),
    ("E1b", "matern32", "f32", 7.63, 2.64),
    ("T1", "rbf", "f64", 12.5, None),
    ("T1", "rbf", "f32", 9.47, 1.89),
    ("T1", "matern32", "f32", 7.93, 2.12),
    ("T1", "matern52", "f64", 9.02, None),
    ("X1a", "rbf", "f64", 13.8, None),
    ("X1a", "rbf", "f32", 19.5, 2.01),
    ("X1b", "rbf", "f64", 38.7, None),
    ("X1c", "matern32", "f64", 13.9, None),
    ("X1c", "matern32", "f32", 12.8, 2.56),
    ("O1", "matern32", "f64", 4.34, None),
    ("O1", "matern52", "f32", 6.5, 2.23),
    ("J1-0", "rbf", "f64", 3.69, None),
    ("J1-12", "rbf", "f64", 4.65, None),
    ("J1-6", "rbf", "f64", 4.31, None),
    ("J1-6", "matern32", "f32", 4.29, 2),
    ("J1-2", "rbf", "f64", 5.36, None),
    ("J1-2", "matern32", "f32", 4.7, 2),
    ("I1a", "rbf", "f64", 2.99, None),
    ("I1b", "rbf", "f64", 2.48, None),
]
INSTANCES: List[Inst] = [_i(c, k, t) for c, k, t, _, _ in _TABLE]
E_REF: Dict[Inst, float] = {_i(c, k, t): e for c, k, t, e, _ in _TABLE}
KV32: Dict[Inst, Optional[float]] = {_i(c, k, t): v for c, k, t, _, v in _TABLE}


def by_id(ident: str) -> Inst:
    return next(i for i in INSTANCES if i.id == ident)


def tol(inst: Inst, variance: float) -> float:
    e = eps_of(inst.np_dtype)
    kv = KV64 * variance if inst.dtype == "f64" else KV32[inst] * e * variance
    return 4.0 * E_REF[inst] * e * variance + kv


# --------------------------------------------------------------------------- inputs
@dataclass
class Problem:
    X: np.ndarray        # float64 values; already rounded through float32 for an fp32 instance
    ls: np.ndarray
    var: float
    jitter: float
    M: int               # as handed to the context; the selection makes min(M, N) picks
    planted: Tuple[int, ...] = ()

    @property
    def N(self):
        return self.X.shape[0]

    @property
    def picks(self):
        return min(self.M, self.N)


def problem(inst: Inst) -> Problem:
    c = CASES[inst.case]
    rng = np.random.default_rng(1000 * c.seed + c.D)
    planted: Tuple[int, ...] = ()
    if c.data in ("normal", "wide"):
        X = rng.standard_normal((c.N, c.D))
        ls = c.ls_scale * (0.7 + rng.random(c.D))
        if c.data == "wide" or c.sqrt_d:   # with lengthscales of order 1 every kernel value underflows the variance at D >= 33: nothing but exact ties
            ls = math.sqrt(c.D) * ls
        var = c.var
    elif c.data == "edges":
        # cluster of radius ~0.3 at the origin; the planted rows on a circle, radius graded by a fixed order that is not the row order
        X = 0.3 * rng.standard_normal((c.N, c.D))
        planted = tuple(r % c.N for r in PLANTED)
        grade = (5, 2, 7, 0, 3, 6, 1, 4)
        for k, r in enumerate(planted):
            ang = 2.0 * math.pi * k / len(planted)
            X[r] = (3.0 + 0.35 * grade[k]) * np.array([math.cos(ang), math.sin(ang)])
        ls, var = np.array([1.9, 2.3]), 1.3
    elif c.data == "ties":
        X = rng.standard_normal((c.N, c.D))
        base = X[:40].copy()
        for off in (64, 256, 512):
            X[off:off + 40] = base
        for off in (40, 296):            # a further copy of rows 0 .. 23 inside the wave that already holds one (rows 0 .. 63, rows 256 .. 319)
            X[off:off + 24] = base[:24]
        ls, var = 0.7 + rng.random(c.D), 1.7
    else:
        raise KeyError(c.data)
    if inst.dtype == "f32":
        X = em.f32(X)
    return Problem(np.ascontiguousarray(X), ls, var, c.jitter, c.M, planted)


def check_geometry(inst: Inst, p: Problem):
    """What the table says about the case, asserted on the built inputs."""
    c = CASES[inst.case]
    assert p.N == c.N <= 3001 and p.X.shape[1] == c.D and p.picks <= 300
    if c.name.startswith("G"):
        assert c.D <= 32 and (pad_dim(c.D) != c.D) == (c.D in (5, 9, 17, 27))
        assert (p.ls.min() > 0.7 * math.sqrt(c.D)) == c.sqrt_d or c.D < 3
    if c.data == "wide":
        assert c.D > 32 and p.ls.min() > 0.7 * math.sqrt(c.D)
    if c.data == "edges":
        assert p.planted == tuple(r % c.N for r in PLANTED) and len(set(p.planted)) == 8
        assert c.N % 256 != 0 and p.planted[-1] == c.N - 1          # the last row sits in a partial block
        rad = np.linalg.norm(p.X, axis=1)
        others = np.setdiff1d(np.arange(c.N), p.planted)
        assert rad[list(p.planted)].min() > 2.0 * rad[others].max()
        # the reference path (the restatement in the instance's type) contains every planted row, in an order that is not the row order
        order = [int(j) for j in restate(p, inst.kind, inst.np_dtype).picks if int(j) in p.planted]
        assert sorted(order) == sorted(p.planted) and order != sorted(order)
    if c.data == "ties":
        assert c.N == 552 and c.N % 256 == 40
        for off in (64, 256, 512):
            assert np.array_equal(p.X[off:off + 40], p.X[:40])
        for off in (40, 296):
            assert np.array_equal(p.X[off:off + 24], p.X[:24]) and (off + 23) // 64 == (off - 40) // 64   # the same wave as rows off - 40 ...
        rest = np.r_[104:256, 320:512]
        assert len(np.unique(np.concatenate([p.X[:40], p.X[rest]]), axis=0)) == 40 + len(rest)
    if c.name == "O1":
        assert c.M == c.N + 5


# --------------------------------------------------------------------------- the path follower (np.longdouble)
def _kernel_ld(kind, X1, X2, ls, var):
    d2 = orc.scaled_sqdist(X1, X2, ls)
    if kind == "matern52":
        return m52.k52(d2, var)
    return orc.kernel_from_sqdist(kind, d2, var)


@dataclass
class Followed:
    regret: np.ndarray       # [picks]  max_i d_ref - d_ref[j_m] before pick m
    dmax: np.ndarray         # [picks]  max_i d_ref before pick m
    d_hist: np.ndarray       # [picks + 1, N] longdouble: d_ref before every pick and after the last step
    trace: float             # sum d_ref after the last step

    def admissible(self, m: int, tolerance: float) -> np.ndarray:
        return np.flatnonzero(self.d_hist[m] >= self.dmax[m] - tolerance)

    def n_admissible(self, tolerance: float) -> np.ndarray:
        return np.array([(self.d_hist[m] >= self.dmax[m] - tolerance).sum() for m in range(len(self.regret))])


def follow(X, kind, ls, var, jitter, picks) -> Followed:
    X = np.asarray(X, dtype=LD)
    ls = np.asarray(ls, dtype=LD)
    var, jitter = LD(var), LD(jitter)
    N, M = X.shape[0], len(picks)
    d = np.full(N, var + jitter, dtype=LD)
    C = np.zeros((M, N), dtype=LD)
    hist = np.zeros((M + 1, N), dtype=LD)
    regret, dmax = np.zeros(M, dtype=LD), np.zeros(M, dtype=LD)
    for m, j in enumerate(picks):
        j = int(j)
        hist[m] = d
        dmax[m] = d.max()
        regret[m] = dmax[m] - d[j]
        if d[j] > 0:
            col = _kernel_ld(kind, X, X[j:j + 1], ls, var).reshape(-1)
            col[j] += jitter
            e = (col - C[:m].T @ C[:m, j]) / np.sqrt(d[j])
            C[m] = e
            d = np.maximum(d - e * e, LD(0))
        d[j] = 0
    hist[M] = d
    return Followed(regret.astype(np.float64), dmax.astype(np.float64), hist, float(d.sum()))


# --------------------------------------------------------------------------- the working-precision restatement
LOG2E = 1.0 / math.log(2.0)
KSCALE = {"rbf": math.sqrt(LOG2E), "matern32": math.sqrt(3.0) * LOG2E, "matern52": math.sqrt(5.0) * LOG2E}   # devmath.h: cglb_kscale_of_kind
DEFECTS = ("ties_high", "drop_tail", "skip_last_block", "pivot_not_zeroed", "no_init_jitter", "no_clamp", "stale_ls", "m52_as_m32",
           "pad_nonzero", "wide_stride")


def scaled_operand(X, kind, ls, T):
    """kernels_prep.hip: xs = (T)((x - centre) * kscale / l) with the centre and the scale in double; the centre is the running column sum / N."""
    centre = np.cumsum(X, axis=0)[-1] / X.shape[0]
    return ((X - centre) * (KSCALE[kind] / np.asarray(ls, dtype=np.float64))).astype(T)


def _kappa_T(kind, d2, T):
    """devmath.h: kappa_from_d2 in the working type."""
    if kind == "rbf":
        return np.exp2(T(-0.5) * d2)
    r = np.sqrt(d2)
    c = math.log(2.0)
    poly = r * T(c) + T(1) if kind == "matern32" else r * (r * T(c * c / 3.0) + T(c)) + T(1)
    return poly * np.exp2(-r)


@dataclass
class Restated:
    picks: np.ndarray
    trace: float
    d_hist: np.ndarray       # [picks + 1, N] in T
    cols: np.ndarray         # [picks, N] kernel columns (variance included, no jitter) in T


def restate(p: Problem, kind: str, T, defect: Optional[str] = None) -> Restated:
    assert defect is None or defect in DEFECTS
    N, M = p.N, p.picks
    ls = p.ls * 10.0 if defect == "stale_ls" else p.ls
    kkind = "matern32" if (defect == "m52_as_m32" and kind == "matern52") else kind
    Xs = scaled_operand(p.X, kkind, ls, T)
    D = Xs.shape[1]
    if defect == "pad_nonzero":          # one padded column of the scaled operand holds something (here: a copy of column 0)
        assert pad_dim(D) > D
        Xs = np.concatenate([Xs, Xs[:, :1]], axis=1)
    if defect == "wide_stride":          # row i read at i * (D - 1) of the row-major operand
        assert D > 32
        flat = Xs.reshape(-1)
        Xs = np.stack([flat[i * (D - 1): i * (D - 1) + D] for i in range(N)])
    var, jit = T(p.var), T(p.jitter)
    d = np.full(N, var + (T(0) if defect == "no_init_jitter" else jit), dtype=T)
    C = np.zeros((M, N), dtype=T)
    hist = np.zeros((M + 1, N), dtype=T)
    cols = np.zeros((M, N), dtype=T)
    picks = np.zeros(M, dtype=np.int64)
    nfull = (N // 256) * 256
    for m in range(M):
        hist[m] = d
        cand = d[:nfull] if (defect == "skip_last_block" and 0 < nfull < N) else d
        j = int(len(cand) - 1 - np.argmax(cand[::-1])) if defect == "ties_high" else int(np.argmax(cand))
        picks[m] = j
        dj = T(np.sqrt(np.float64(cand[j]))) if cand[j] > 0 else T(1)   # select_pivot_kernel: sqrt in double, 1 once the variance is exhausted
        d2 = np.zeros(N, dtype=T)
        for q in range(Xs.shape[1]):
            df = Xs[:, q] - Xs[j, q]
            d2 += df * df
        col = var * _kappa_T(kkind, d2, T)
        cols[m] = col
        col = col.copy()
        col[j] += jit
        mm = (m // 8) * 8 if defect == "drop_tail" else m
        dot = np.zeros(N, dtype=T)
        for t in range(mm):              # row by row: every point sees the same sequence of roundings, as a thread of the kernel does
            dot += C[t] * C[t, j]
        e = (col - dot) / dj
        C[m] = e
        d = d - e * e
        if defect != "no_clamp":
            d = np.maximum(d, T(0))
        if defect != "pivot_not_zeroed":
            d[j] = 0
    hist[M] = d
    return Restated(picks, float(d.astype(np.float64).sum()), hist, cols)


# --------------------------------------------------------------------------- measurements and checks
def measure(inst: Inst, p: Optional[Problem] = None):
    """(E_ref in eps_T variance, KV32 in eps_32 variance or None, restatement, follower on the restatement's path)."""
    p = problem(inst) if p is None else p
    T = inst.np_dtype
    r = restate(p, inst.kind, T)
    f = follow(p.X, inst.kind, p.ls, p.var, p.jitter, r.picks)
    unit = eps_of(T) * p.var
    e_ref = float(np.abs(r.d_hist.astype(LD) - f.d_hist).max()) / unit
    kv = None
    if inst.dtype == "f32":
        Xp = p.X[r.picks]
        K = m52.k52(orc.scaled_sqdist(Xp, p.X, p.ls), p.var) if inst.kind == "matern52" else orc.kernel_matrix(inst.kind, Xp, p.X, p.ls, p.var)
        kv = float(np.abs(r.cols.astype(np.float64) - K).max()) / unit
    return e_ref, kv, r, f


@dataclass
class Verdict:
    worst_regret: float      # in units of tol
    worst_step: int
    trace_err: float         # |trace - sum d_ref| in units of N tol
    multi: int               # steps with more than one admissible candidate
    unique_ok: bool          # no index repeats while the follower's remaining maximum exceeds tol
    followed: Followed


def judge(inst: Inst, p: Problem, picks, trace) -> Verdict:
    """The checks of one result (the library's, the restatement's or a defect's), in units of the instance's tolerance."""
    t = tol(inst, p.var)
    f = follow(p.X, inst.kind, p.ls, p.var, p.jitter, picks)
    seen, unique_ok = set(), True
    for m, j in enumerate(picks):
        if int(j) in seen and f.dmax[m] > t:
            unique_ok = False
        seen.add(int(j))
    w = int(np.argmax(f.regret))
    return Verdict(float(f.regret[w] / t), w, abs(trace - f.trace) / (p.N * t), int((f.n_admissible(t) > 1).sum()), unique_ok, f)


def tie_rule_violations(p: Problem, picks) -> List[int]:
    """Steps whose pick has an identical row of lower index that is still unpicked (duplicate rows give bitwise equal d on the device)."""
    bad, taken = [], set()
    for m, j in enumerate(picks):
        j = int(j)
        same = np.flatnonzero((p.X[:j] == p.X[j]).all(axis=1))
        if any(int(i) not in taken for i in same):
            bad.append(m)
        taken.add(j)
    return bad


def kernel_fn(kind, ls, var):
    """The callback of orc.greedy_conditional_variance for any of the three kinds."""
    def fn(x1, x2=None, full_cov=False):
        x1 = np.asarray(x1, dtype=np.float64)
        if not full_cov:
            return np.full(x1.shape[0], var)
        x2 = x1 if x2 is None else np.asarray(x2, dtype=np.float64)
        d2 = orc.scaled_sqdist(x1, x2, np.asarray(ls, dtype=np.float64))
        return m52.k52(d2, var) if kind == "matern52" else orc.kernel_from_sqdist(kind, d2, var)
    return fn


def single_share(f: Followed, tolerance: float) -> float:
    """Share of the steps with exactly one admissible candidate.  Step 0 is left out: every d equals variance + jitter there on every path, the
    tie rule alone decides (row 0, asserted exactly), so no case with M < 10 could otherwise reach 90 %."""
    n = f.n_admissible(tolerance)[1:]
    return float((n == 1).mean()) if len(n) else 1.0


def exact_violations(p: Problem, picks, trace) -> List[str]:
    """What holds exactly on the device whatever the round-off: the first pick is row 0 (all d equal); a picked row has no identical unpicked
    row of lower index (bitwise equal d); d is clamped at zero, so the trace is not negative; a pivot's d is set to zero, so once all N rows
    are picked the trace is exactly zero."""
    picks = [int(j) for j in picks]
    out = []
    if picks[0] != 0:
        out.append(f"first pick {picks[0]}")
    ties = tie_rule_violations(p, picks)
    if ties:
        out.append(f"tie rule at steps {ties}")
    if not trace >= 0.0:
        out.append(f"negative trace {trace!r}")
    if len(set(picks)) == p.N and trace != 0.0:
        out.append(f"trace {trace!r} after all rows were picked")
    return out


def intra_wave_tie_steps(p: Problem, picks) -> List[int]:
    """Steps whose pick still has an identical, unpicked row inside its own 64-row wave: the lowest-index rule of the wave shuffle decided."""
    out, taken = [], set()
    for m, j in enumerate(picks):
        j = int(j)
        lo = (j // 64) * 64
        same = lo + np.flatnonzero((p.X[lo:lo + 64] == p.X[j]).all(axis=1))
        if any(int(i) != j and int(i) not in taken for i in same):
            out.append(m)
        taken.add(j)
    return out


def closed_form_trace(p: Problem, kind: str, picks) -> float:
    """tr(K~_ff - K~_fu K~_uu^-1 K~_uf) with K~ = K + jitter I in float64, by a solve: independent of the recurrence the follower runs."""
    picks = np.asarray(picks)
    k = kernel_fn(kind, p.ls, p.var)
    Kuf = k(p.X[picks], p.X, full_cov=True)
    Kuf[np.arange(len(picks)), picks] += p.jitter
    Kuu = Kuf[:, picks]
    return float(p.N * (p.var + p.jitter) - np.trace(Kuf.T @ np.linalg.solve(Kuu, Kuf)))
