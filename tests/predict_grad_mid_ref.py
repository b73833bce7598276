"""The row-weighted gradient product and the cglb / sgpr / gpr gradient predictors at mid widths (33 - 96 input dimensions, option "input_grad_mid":
csrc/kernels_predict_grad_mid.hip): the restated launch geometry, the covering cell table, the float64 restatement of the kernel's arithmetic with
its planted defects, and the predictor cases of tests/test_gpu_predict_grad_mid.py (test helper, not a test module; runs on any CPU).

References and tolerances are the project's own, UNCHANGED: predict_grad_ref.weighted_product (np.longdouble) with weighted_tolerance - 1e-11 of
f sum |w| |h delta / l| per gradient element and of f sum |w kappa| per value, plus the clamp floor - and, at precision level 2, the level term of
input_grad_mid_ref.level_tolerance applied to the same sums; predict_grad_ref.predictor_tolerance (1e-8 max(max |ref|, G_k)) for the predictors.  The
kernel takes direct differences in hot units and accumulates in delta form, in-lane, like cross_grad_mid_kernel, so the product rule applies as it
stands.

Geometry (csrc/row_slab.h: predict_grad_mid_split): a new point is shared by SPLIT = 4 lanes of HD = Dh / 4 coordinates, B = 256 / SPLIT = 64 rows per
workgroup; two weight slots at every width; the point range is split by the kff_jsplit rule with even chunks, capped by the slab of the two-weight
instance whichever weights are given.

Problems: wide_cases.problem (standard normal inputs, lengthscales U(0.8, 1.6) sqrt(D)), so that off-diagonal kernel values are of order 0.1
(`wide_cases.informative` is asserted on every reference by tests/test_predict_grad_mid_ref_host.py).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import input_grad_mid_ref as igm
import input_grad_ref as ig
import kernel_value_cases as kv
import predict_grad_ref as pg
import slab_rules
import wide_cases as wc

LD = np.longdouble
KINDS = wc.KINDS
ROWS = pg.ROWS
FAR = 1e3
JITTER = 1e-4      # predict_ref.JITTER and its reason: cond(K_uu) ~ M f / jitter bounds what the textbook form keeps of its 1e-8


# ---- the launch geometry, restated ----------------------------------------------------------------------------------------------------------------
hot_width, part_width, slice_width = igm.hot_width, igm.part_width, igm.slice_width


def split(d: int) -> int:
    return 4


def rows_per_block(d: int) -> int:
    return 256 // split(d)


def weighted_split(n_rows: int, n_pts: int, d: int, forced: int = 0):
    """(chunks, chunk length) of one launch (n_rows <= ROWS): the kff_jsplit rule with even chunks, capped by the slab of the two-weight instance."""
    B = rows_per_block(d)
    return slab_rules.pair_split(forced, (n_rows + B - 1) // B, n_pts, slab_rules.slot_cap(n_rows, 2 * (hot_width(d) + 1)), even=True)


# ---- the cell table -----------------------------------------------------------------------------------------------------------------------------
DIMS = igm.DIMS                                   # 33, 48, 49, 64, 65, 80, 81, 96: every hot width once padded and once full
N_PTS = (1, 65, 300)
JSPLITS = (1, 3, 7)
SETS = ("train", "inducing")
WEIGHTS = ("uw", "u", "w")                        # the weight combination the host restatement runs (the GPU test runs all three on every cell)
#: cells that also run at precision level 2: one per kind
PRECISION_CELLS = (2, 6, 13)          # 300 points each


def row_counts(d: int):
    B = rows_per_block(d)
    return (1, 2, B - 1, B, B + 1)


def product_cells():
    """dicts (D, n_new, n_pts, set, jsplit, kind, precision, ldw_extra, weights): every D with its five row counts (40 cells) and one cell with more
    rows than a launch takes; the other axes are dealt by cell number with strides that make every value meet every hot width, the way
    tests/geometry_cases.py prunes its crossings (asserted in tests/test_predict_grad_mid_ref_host.py)."""
    cells = []
    for a, d in enumerate(DIMS):
        for q, n in enumerate(row_counts(d)):
            cells.append(dict(D=d, n_new=n, n_pts=N_PTS[(q + a) % 3], set=SETS[(q + a // 2) % 2], jsplit=JSPLITS[(2 * q + a) % 3], kind=KINDS[(q + 2 * a + 1) % 3],
                              precision=(q + a // 3) % 2, ldw_extra=(1, 3, 8)[(q + a) % 3] if n > 1 else 5, weights=WEIGHTS[(q + a // 2) % 3]))
    cells.append(dict(D=77, n_new=4097, n_pts=65, set="inducing", jsplit=3, kind="matern32", precision=1, ldw_extra=7, weights="uw"))
    return cells


def cell_id(c) -> str:
    return "D%d_n%d_P%d_%s_j%d_%s_p%d_ld%d" % (c["D"], c["n_new"], c["n_pts"], c["set"], c["jsplit"], c["kind"], c["precision"], c["ldw_extra"])


def cell_problem(c):
    """(X, y, Z, hypers dict, xnew, u [n_pts], Wt [n_pts, ldw] with NaN in the columns from n_new on) of a cell.  The set the cell multiplies against
    has n_pts rows (the other one 7); new point 0 sits on point min(3, n_pts - 1) of that set and new point 1 (if any) at 10^3."""
    D = c["D"]
    N, M = (c["n_pts"], 7) if c["set"] == "train" else (70, c["n_pts"])
    with np.errstate(invalid="ignore"):              # N = 1: the z-normalised target of one row is 0 / 0
        X, y, _Z, hyp = wc.problem(N, D, 1, seed=D + N)
    y = np.where(np.isfinite(y), y, 0.0)
    rng = np.random.default_rng(1000 * D + 7 * c["n_new"] + c["n_pts"])
    Z = X[:M].copy() if M <= N else rng.standard_normal((M, D))
    P = X if c["set"] == "train" else Z
    xnew = ig.new_points(P, c["n_new"])
    u = rng.standard_normal(len(P))
    Wt = np.full((len(P), c["n_new"] + c["ldw_extra"]), np.nan)
    Wt[:, :c["n_new"]] = rng.standard_normal((len(P), c["n_new"]))
    h = dict(lengthscales=np.asarray(hyp.lengthscales, dtype=np.float64), variance=wc.VARIANCE, noise=wc.NOISE, mean=wc.MEAN)
    return X, y, Z, h, xnew, u, Wt


def weights_of(c, u, Wt):
    """(u, Wt) of the cell's weight combination"""
    return (u if "u" in c["weights"] else None), (Wt if "w" in c["weights"] else None)


def level_tolerance(kind, xnew, P, ls, variance, u=None, Wt=None, precision: int = 1):
    """predict_grad_ref.weighted_tolerance; at precision level 2 the error of that level's 2^x is added to its 1e-11, term by term, and nothing else
    (input_grad_mid_ref.level_tolerance's rule on the row-weighted sums)."""
    tol = list(pg.weighted_tolerance(kind, xnew, P, ls, variance, u, Wt))
    if precision == 2:
        n = len(xnew)
        floors = (None if u is None else ig.FLOOR * variance * np.abs(np.asarray(u, dtype=np.float64)).sum() * np.ones(n),
                  None if Wt is None else ig.FLOOR * variance * np.abs(np.asarray(Wt, dtype=np.float64)[:, :n]).sum(axis=0))
        for x, t in enumerate(tol):
            if t is not None:
                fl = floors[x // 2] if t.ndim == 1 else floors[x // 2][:, None]
                tol[x] = t + (t - fl) * (igm.LEVEL2_KERNEL_ERROR / ig.TOL)
    return tuple(tol)


# ---- float64 restatement of the kernel's arithmetic, with the planted defects ---------------------------------------------------------------------
MID_DEFECTS = ("drop_part", "part_offset", "wt_neighbour", "swap_uw", "ld_wrong", "drop_chunk_last", "pad_nonzero", "set_stale", "const_l")
STALE_FACTOR = 1.25     # "set_stale": the lengthscales the point set was staged with, over the current ones


def restated_weighted(kind, xnew, P, cen, ls, variance, u=None, Wt=None, jsplit: int = 0, wscale: float = 1.0, defect=None):
    """(out_u [n], gout_u [n, D], out_w [n], gout_w [n, D]) in float64 the way the kernel and its finish form them (None for an absent weight): both
    sets centred and scaled to hot units, (x - c) * ((ks / l) * hot), zero-padded to Dh; direct differences; per lane part two interleaved chains of
    squares, the parts summed in pairs; the profiles once per pair; delta-form sums per chunk of points in hot units, the chunks added in order; then
    the finish's constants as it rounds them: f for the values, ((wscale * (-f / (ks ks hot))) * (ks / l_k)) for gradient component k.
    `defect`: one of MID_DEFECTS -
      drop_part        the partial distance of part 1 (coordinates HD .. 2 HD - 1, all real: 2 HD = Dh / 2 < D) is left out of d2;
      part_offset      parts 1 and 2 store their gradient components at each other's offset;
      wt_neighbour     row i reads the weight of row i + 1 (the last row its own);
      swap_uw          the u sums land in the Wt outputs and the reverse (both weights given);
      ld_wrong         the flat Wt array is read with the leading dimension n_new (ldw > n_new: the NaN of the padding columns enter);
      drop_chunk_last  the last point of the first chunk is lost;
      pad_nonzero      the padding coordinates D .. Dh - 1 of the new points hold one hot unit instead of 0 (Dh > D);
      set_stale        the point set was staged at lengthscales STALE_FACTOR times the current ones (the inducing-point operand not refreshed by
                       set_hypers);
      const_l          the gradient constant at l_k in place of l_k^2: the finish multiplies by ks alone in place of ks / l_k, so the entry carries
                       the 1 / l_k of the hot-unit difference only."""
    xnew, P = np.asarray(xnew, dtype=np.float64), np.asarray(P, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    n, npts, D = len(xnew), len(P), P.shape[1]
    Dh, SP, HD = hot_width(D), split(D), part_width(D)
    ks, hot = kv.kscale(kind), kv.hot_scale(kind)
    scale = ks / ls
    za, zb = np.zeros((n, Dh)), np.zeros((npts, Dh))
    za[:, :D] = (xnew - cen) * (scale * hot)
    zb[:, :D] = (P - cen) * ((scale / STALE_FACTOR if defect == "set_stale" else scale) * hot)
    if defect == "pad_nonzero":
        za[:, D:] = 1.0
    W = None
    if Wt is not None:
        Wt = np.asarray(Wt, dtype=np.float64)
        W = Wt.reshape(-1)[:npts * n].reshape(npts, n) if defect == "ld_wrong" else Wt[:, :n]
        if defect == "wt_neighbour":
            W = W[:, np.minimum(np.arange(n) + 1, n - 1)]
    uu = None if u is None else np.asarray(u, dtype=np.float64).reshape(-1)
    nsplit, chunk = weighted_split(min(n, ROWS), npts, D, jsplit)
    sums = [None if uu is None else np.zeros(n), None if uu is None else np.zeros((n, Dh)), None if W is None else np.zeros(n), None if W is None else np.zeros((n, Dh))]
    for a, b in pg._rows(n):
        df = za[a:b, None, :] - zb[None, :, :]                                 # [rows, npts, Dh]
        sq = df * df
        parts = [sq[:, :, p * HD:(p + 1) * HD:2].sum(axis=2) + sq[:, :, p * HD + 1:(p + 1) * HD:2].sum(axis=2) for p in range(SP)]
        if defect == "drop_part":
            parts[1] = np.zeros_like(parts[0])
        d2 = (parts[0] + parts[1]) + (parts[2] + parts[3])
        kap, h = igm._profiles64(kind, d2 / (ks * hot) ** 2)
        if defect == "drop_chunk_last":
            j = min(chunk, npts) - 1
            kap, h = kap.copy(), h.copy()
            kap[:, j], h[:, j] = 0.0, 0.0
        for js in range(nsplit):
            sl = slice(js * chunk, min((js + 1) * chunk, npts))
            if uu is not None:
                sums[0][a:b] += kap[:, sl] @ uu[sl]
                sums[1][a:b] += np.einsum("ij,ijk,j->ik", h[:, sl], df[:, sl, :], uu[sl])
            if W is not None:
                sums[2][a:b] += (kap[:, sl] * W[sl, a:b].T).sum(axis=1)
                sums[3][a:b] += np.einsum("ij,ijk,ji->ik", h[:, sl], df[:, sl, :], W[sl, a:b])
    if defect == "part_offset":
        for x in (1, 3):
            if sums[x] is not None:
                g = sums[x]
                sums[x] = np.concatenate([g[:, :HD], g[:, 2 * HD:3 * HD], g[:, HD:2 * HD], g[:, 3 * HD:]], axis=1)
    gfac = -variance / (ks * ks * hot)
    con = np.full(D, ks) if defect == "const_l" else scale
    out = [None] * 4
    if uu is not None:
        out[0], out[1] = variance * sums[0], (gfac * con) * sums[1][:, :D]
    if W is not None:
        out[2], out[3] = variance * sums[2], ((wscale * gfac) * con) * sums[3][:, :D]
    if defect == "swap_uw" and uu is not None and W is not None:
        out = [out[2], out[3], out[0], out[1]]
    return tuple(out)


def defect_applies(defect, c) -> bool:
    """Whether a cell can show a defect at all, from its shape alone.  The first two new points sit on a point of the set and at 10^3: a pair that is
    neither coincident (gradient 0, d2 = 0) nor out of range needs a second point in the set or a third new point (`live`)."""
    n, npts, w = c["n_new"], c["n_pts"], c["weights"]
    live = npts > 1 or n > 2
    if defect in ("drop_part", "part_offset", "const_l"):
        return live
    if defect == "wt_neighbour":        # row 0 reads row 1's weight
        return "w" in w and n > 1
    if defect == "swap_uw":
        return w == "uw"
    if defect == "ld_wrong":            # row 0 of the flat array is read alike
        return "w" in w and npts > 1
    if defect == "pad_nonzero":
        return hot_width(c["D"]) > c["D"]
    if defect == "set_stale":           # the library's own stale operand can only be the inducing points'
        return c["set"] == "inducing"
    return True                          # drop_chunk_last: with one point everything is lost


def miss(got, want, tol) -> float:
    """max over the outputs present of |got - want| / tolerance; inf for an entry that is not finite."""
    worst = 0.0
    for g, w, t in zip(got, want, tol):
        if w is None:
            assert g is None
            continue
        if not np.all(np.isfinite(g)):
            return float("inf")
        worst = max(worst, float((np.abs(g - w) / t).max()))
    return worst


# ---- single kernel values (tests/kernel_value_cases.py, sets F40 / F64 / F77 / F90) ----------------------------------------------------------------
#: The rounding count of a gradient entry read through weighted_grad_mid_kernel with a unit weight is the c = 19 of the mid-width input-gradient path
#: (kernel_value_cases.INPUT_GRAD_ROUNDINGS["cross_grad_mid"]), operation for operation, counted on the new kernel and its finish:
#:   every entry   df by one fmac with -1 [1]; t = h * 1 exact (u = e_m, Wt = 0 / 1), fma(t, df, 0) [1]; the finish's constant * s [1]; the operands'
#:                 common scale fl(ks hot / l_k) [3 u] - 3 + 3;
#:   mid width     the constant (gfac_b * scale[k]) with gfac = -f / (ks * ks * hot) (ks * ks [1], the division [1], kscale twice [2 KSCALE_U]),
#:                 gfac_b = wscale * gfac with wscale = 1 for cglb_cross_grad_weighted: exact; scale[k] = ks / l_k of upload_scales (kscale [KSCALE_U],
#:                 the division [1]); their product [1] - (2 + 2 KSCALE_U) + (1 + KSCALE_U) + 1.
#: The sums of exact zeros in the accumulators and over the slabs are exact.  The kernel value's own path is that of every input-gradient product
#: (kernel_value_cases.path_for: one kappa_hfac_hot_from_d2 per pair, the clamped 2^x; d2 by four lane parts of two chains: chain_extra 0).
VALUE_ENTRY = "cross_grad_mid"
VALUE_SETS = ("F40", "F64", "F77", "F90")


# ---- the predictors ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    N: int
    D: int
    M: int
    n_new: int
    kind: str

    @property
    def id(self) -> str:
        return f"N{self.N}-D{self.D}-M{self.M}-n{self.n_new}-{self.kind}"


SHAPES = ((300, 40, 33), (300, 77, 33))             # D = 40 and 77: partly padded lane parts (Dh 48: part 3 holds 4 of 12; Dh 80: part 3 holds 17 of 20)
CGLB_CASES = tuple(Case(N, D, M, n, kind) for (N, D, M) in SHAPES for kind in KINDS for n in (1, 65))
LARGE_CASE = Case(300, 40, 33, 4097, "matern32")    # more new points than a launch takes
GPR_CASES = tuple(Case(N, D, 0, 65, KINDS[(x + k) % 3]) for x, (N, D, _M) in enumerate(SHAPES) for k in (0, 1))


@functools.lru_cache(maxsize=None)
def problem(case: Case):
    """(X, y, hypers, v) of a case - shared and read-only: wide_cases.problem with predict_ref's jitter; v any vector of the size of a CG iterate."""
    X, y, _Z, hyp = wc.problem(case.N, case.D, max(case.M, 1), seed=case.N + case.D)
    hyp.jitter = JITTER
    v = 0.05 * np.random.default_rng(case.D).standard_normal(case.N)
    for a in (X, y, v, hyp.Z, hyp.lengthscales):
        a.setflags(write=False)
    return X, y, hyp, v


def xnew(case: Case) -> np.ndarray:
    """training rows, inducing points, random points; the last one (of two or more) at 10^3"""
    X, _, hyp, _ = problem(case)
    n = case.n_new
    rows = [X[:5]] + ([hyp.Z[:3]] if case.M > 0 else []) + [np.random.default_rng(1000 * case.D + n).standard_normal((n, case.D))]
    out = np.concatenate(rows, axis=0)[:n].copy()
    if n >= 2:
        out[-1] = FAR
    return out


def _by_rows(fn, Xnew, rows=512):
    """a predictor reference over blocks of new points (they are independent), so that the dense [n, N, D] terms stay small"""
    parts = [fn(Xnew[a:a + rows]) for a in range(0, len(Xnew), rows)]
    return pg.Grad(*[np.concatenate([getattr(p, name) for p in parts], axis=0) for name in ("mean", "g_mean", "var", "g_var")])


@functools.lru_cache(maxsize=None)
def cglb_reference(case: Case, quad_term: int) -> pg.Grad:
    X, y, hyp, v = problem(case)
    return _by_rows(lambda xs: pg.cglb_predict_grad_autograd(case.kind, X, y, hyp, v, xs, quad_term), xnew(case))


@functools.lru_cache(maxsize=None)
def cglb_analytic(case: Case, quad_term: int) -> pg.Grad:
    X, y, hyp, v = problem(case)
    return _by_rows(lambda xs: pg.cglb_predict_grad_analytic(case.kind, X, y, hyp, v, xs, quad_term), xnew(case))


@functools.lru_cache(maxsize=None)
def gpr_reference(case: Case) -> pg.Grad:
    X, y, hyp, _ = problem(case)
    return pg.gpr_predict_grad_autograd(case.kind, X, y, hyp, xnew(case))
