"""The input-gradient products at mid widths (33 - 96 input dimensions, option "input_grad_mid": csrc/kernels_input_grad_mid.hip): the restated
geometry rule, the covering cell table, the float64 restatements of the two kernels' arithmetic with their planted defects, and the tolerances
of tests/test_gpu_input_grad_mid.py (test helper, not a test module; runs on any CPU).

The references are those of tests/input_grad_ref.py (`cross_grad`, `feature_grad`, np.longdouble) and the tolerances its `cross_tolerance` and
`feature_tolerance`, UNCHANGED: the cross kernel takes direct differences in hot units and accumulates in delta form, in-lane, so neither the
moment-form term nor the Gram-chain term applies; the feature kernel's phase is a sum of D products like the narrow one's (SPLIT partial chains and
three additions in the place of one chain: no more roundings than the d + 3 the tolerance counts), and at the cells' feature counts the feature rule
gives the chunk count input_grad_ref.feature_split states (asserted in tests/test_input_grad_mid_ref_host.py).

Geometry (csrc/row_slab.h: input_grad_mid_split, input_grad_mid_group): a new point is shared by SPLIT = 4 lanes of HD = Dh / 4 coordinates,
the group has G = 4 columns up to Dh = 64 and 2 beyond; B = 256 / SPLIT = 64 rows per workgroup.  A column's coordinates travel in slices of
CH = 8 coordinates per part, or 4 where HD is no multiple of 8 (Dh 48 and 80).
"""
from __future__ import annotations

import numpy as np

import input_grad_ref as ig
import slab_rules
import wide_cases as wc
from input_grad_ref import cross_grad, cross_tolerance, feature_grad, feature_tolerance, predict_grad   # noqa: F401  (the reference and its tolerances)

LD = np.longdouble
KINDS = wc.KINDS
ROWS = 4096


# ---- the geometry rule, restated ---------------------------------------------------------------------------------------------------------------
def hot_width(d: int) -> int:
    assert 32 < d <= 96
    return 48 if d <= 48 else 64 if d <= 64 else 80 if d <= 80 else 96


def split(d: int) -> int:
    return 4


def group_width(d: int) -> int:
    return 4 if hot_width(d) <= 64 else 2


def rows_per_block(d: int) -> int:
    return 256 // split(d)


def part_width(d: int) -> int:
    return hot_width(d) // split(d)


def slice_width(d: int) -> int:
    return 8 if part_width(d) % 8 == 0 else 4


def cross_split(n_rows: int, N: int, d: int, forced: int = 0):
    """(chunks, chunk length) of one launch (n_rows <= ROWS): the kff_jsplit rule, capped by the slab of G (Dh + 1) doubles per row."""
    B = rows_per_block(d)
    return slab_rules.pair_split(forced, (n_rows + B - 1) // B, N, slab_rules.slot_cap(n_rows, group_width(d) * (hot_width(d) + 1)), even=True)


# ---- the cell table ----------------------------------------------------------------------------------------------------------------------------
DIMS = (33, 48, 49, 64, 65, 80, 81, 96)          # every hot width once padded and once full
N_VALUES = (1, 65, 300)
JSPLITS = (1, 3, 7)
F_VALUES = (1, 65)
#: (Dh, SPLIT, G) -> the D of DIMS that reach it
CLASSES = {(48, 4, 4): (33, 48), (64, 4, 4): (49, 64), (80, 4, 2): (65, 80), (96, 4, 2): (81, 96)}
#: cells that also run at the precision levels 0 and 2: one per kind
PRECISION_CELLS = (7, 4, 2)


def s_values(d: int):
    g = group_width(d)
    return (1, g, g + 1, 9)


def row_counts(d: int):
    B = rows_per_block(d)
    return (1, 2, B - 1, B, B + 1)


def product_cells():
    """dicts (D, n_new, N, jsplit, S, kind, F): every D with its five row counts, one cell each (40); N, kff_jsplit, S, the kind and F are dealt
    by cell number with the strides of input_grad_ref.product_cells (tests/geometry_cases.py prunes its crossings the same way)."""
    cells, x = [], 0
    for a, d in enumerate(DIMS):
        for q, n in enumerate(row_counts(d)):
            cells.append(dict(D=d, n_new=n, N=N_VALUES[(x + a) % 3], jsplit=JSPLITS[(x // 3 + a) % 3], S=s_values(d)[(q + a) % 4], kind=KINDS[(q + a) % 3],
                              F=F_VALUES[(x + q // 2) % 2]))
            x += 1
    return cells


def cell_id(c) -> str:
    return "D%d_n%d_N%d_j%d_S%d_%s_F%d" % (c["D"], c["n_new"], c["N"], c["jsplit"], c["S"], c["kind"], c["F"])


def cell_problem(c):
    """(X, y, hypers dict, xnew, V [N, S], omega [F, D], b [F], W [S, F]) of a cell: wide_cases.problem (standard normal inputs, lengthscales U(0.8, 1.6) sqrt(D)) with the middle
    row a duplicate of the row the first new point sits on; new points: that training row first, a point at 10^3 second, the rest random."""
    N, D = c["N"], c["D"]
    with np.errstate(invalid="ignore"):              # N = 1: the z-normalised target of one row is 0 / 0
        X, y, _Z, hyp = wc.problem(N, D, 1, seed=D + N)
    X = X.copy()
    y = np.where(np.isfinite(y), y, 0.0)
    if N > 7:
        X[N // 2] = X[3]
    rng = np.random.default_rng(1000 * D + 7 * c["n_new"] + N + c["S"])
    V = rng.standard_normal((N, c["S"]))
    h = dict(lengthscales=np.asarray(hyp.lengthscales, dtype=np.float64), variance=wc.VARIANCE, noise=wc.NOISE, mean=wc.MEAN)
    import sample_ref as sr
    nu, F = sr.NU[c["kind"]], c["F"]
    omega, b = sr.features_from_draws(c["kind"], rng.standard_normal((F, D)), None if nu is None else rng.chisquare(2 * nu, F), rng.uniform(0, 1, F))
    return X, y, h, ig.new_points(X, c["n_new"]), V, omega, b, rng.standard_normal((c["S"], F))


def feature_split(n_rows: int, F: int, d: int):
    """(chunks, chunk length) of one launch of the feature product (n_rows <= ROWS): the feature rule at 64 rows per block, capped by the slab."""
    return slab_rules.feature_split(rows_per_block(d), n_rows, F, slab_rules.slot_cap(n_rows, group_width(d) * (hot_width(d) + 1)))


# ---- float64 restatement of the kernel's arithmetic, with the planted defects --------------------------------------------------------------------
MID_DEFECTS = ("pad_nonzero", "drop_part", "drop_slice", "clamped_row_stored", "halves_swapped")


def _profiles64(kind, d2):
    k, h = ig.profiles(kind, d2)          # longdouble evaluation of the profiles at the float64 distance: the device's table 2^x is held to 1e-13 elsewhere
    return k.astype(np.float64), h.astype(np.float64)


def restated_cross_grad(kind, xnew, X, ls, variance, V, jsplit: int = 0, defect=None):
    """(out [n, S], gout [n, S, D]) in float64 the way the kernel forms them: centred and scaled coordinates zero-padded to Dh, SPLIT partial
    squared distances from direct differences summed in pairs, the profiles once per pair, delta-form sums per column chunk, the chunks added in
    order, the constants last.  `defect`: one of MID_DEFECTS -
      pad_nonzero          the padding coordinates D .. Dh - 1 of the new points hold 1 instead of 0 (applies where Dh > D);
      drop_part            the partial distance of part 1 (coordinates HD .. 2 HD - 1, all real: 2 HD = Dh / 2 < D) is left out of d2;
      drop_slice           the last slice of part 0 (CH coordinates, all real: HD <= 24 < D) is left out of d2 and of the gradient;
      clamped_row_stored   the lanes past n_new store the last row's sums: in the slab they land on the first rows of the next chunk's slab, modelled
                           as those rows receiving the last row's partial sums of the previous chunk in place of their own (applies with several
                           chunks, n_new > 1 and n_new no multiple of B);
      halves_swapped       the upper half-wave's parts (2, 3) write the components of the lower's (0, 1) and the reverse."""
    X = np.asarray(X, dtype=np.float64)
    xnew = np.asarray(xnew, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    V = np.asarray(V, dtype=np.float64).reshape(len(X), -1)
    n, N, D, S = len(xnew), len(X), X.shape[1], V.shape[1]
    Dh, SP, HD, CH, B = hot_width(D), split(D), part_width(D), slice_width(D), rows_per_block(D)
    cen = X.mean(axis=0)
    za, zb = np.zeros((n, Dh)), np.zeros((N, Dh))
    za[:, :D], zb[:, :D] = (xnew - cen) / ls, (X - cen) / ls
    if defect == "pad_nonzero":
        za[:, D:] = 1.0
    df = za[:, None, :] - zb[None, :, :]                                   # [n, N, Dh]
    live = np.ones(Dh, dtype=bool)
    if defect == "drop_slice":
        live[HD - CH:HD] = False
    parts = [(df[:, :, p * HD:(p + 1) * HD] ** 2 * live[p * HD:(p + 1) * HD]).sum(axis=2) for p in range(SP)]
    if defect == "drop_part":
        parts[1] = np.zeros_like(parts[0])
    d2 = (parts[0] + parts[1]) + (parts[2] + parts[3])
    kap, h = _profiles64(kind, d2)
    nsplit, chunk = cross_split(n, N, D, jsplit)
    out, g = np.zeros((n, S)), np.zeros((n, S, Dh))
    prev = None
    for js in range(nsplit):
        sl = slice(js * chunk, min((js + 1) * chunk, N))
        po = kap[:, sl] @ V[sl]
        pg = np.einsum("ij,ijk,js->isk", h[:, sl], df[:, sl, :] * live, V[sl])
        if defect == "clamped_row_stored" and prev is not None and n % B:
            spill = min(B - n % B, n)
            po[:spill], pg[:spill] = prev[0][-1], prev[1][-1]
        prev = (po.copy(), pg.copy())
        out += po
        g += pg
    if defect == "halves_swapped":
        g = np.concatenate([g[:, :, 2 * HD:], g[:, :, :2 * HD]], axis=2)
    return variance * out, -variance * g[:, :, :D] / ls


def restated_feature_grad(x, cen, ls, variance, omega, b, W, defect=None):
    """(out [n, S], gout [n, S, D]) of the feature product in float64 the way the kernel forms them: the records in turns (omega / (2 pi l),
    b / 2 pi), the centred row zero-padded to Dh, SPLIT partial phases (b in part 0) summed in pairs, input_grad_ref.sincos_turns, the sums per
    feature chunk added in order, -2 pi amp last.  `defect`: one of MID_DEFECTS, as restated_cross_grad (pad_nonzero: the row's padding holds 1
    where the slices re-read the record's last frequency)."""
    x = np.asarray(x, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    W = np.asarray(W, dtype=np.float64)
    n, D = x.shape
    S, F = W.shape
    Dh, SP, HD, CH, B = hot_width(D), split(D), part_width(D), slice_width(D), rows_per_block(D)
    two_pi = 2 * np.arccos(LD(-1))
    inv = (1 / (two_pi * ls.astype(LD))).astype(np.float64)
    om = np.zeros((F, Dh))
    om[:, :D] = np.asarray(omega, dtype=np.float64) * inv
    om[:, D:] = om[:, D - 1:D]                                            # the clamped re-read of the last real frequency
    bt = np.asarray(b, dtype=np.float64) * float(1 / two_pi)
    z = np.zeros((n, Dh))
    z[:, :D] = x - np.asarray(cen, dtype=np.float64)
    if defect == "pad_nonzero":
        z[:, D:] = 1.0
    live = np.ones(Dh, dtype=bool)
    if defect == "drop_slice":
        live[HD - CH:HD] = False
    parts = [(z[:, p * HD:(p + 1) * HD] * live[p * HD:(p + 1) * HD]) @ om[:, p * HD:(p + 1) * HD].T for p in range(SP)]
    if defect == "drop_part":
        parts[1] = np.zeros_like(parts[0])
    ph = ((parts[0] + bt[None, :]) + parts[1]) + (parts[2] + parts[3])
    cv, sv = ig.sincos_turns(ph)
    nsplit, chunk = feature_split(n, F, D)
    out, g = np.zeros((n, S)), np.zeros((n, S, Dh))
    prev = None
    for js in range(nsplit):
        sl = slice(js * chunk, min((js + 1) * chunk, F))
        po = cv[:, sl] @ W[:, sl].T
        pg = np.einsum("ij,sj,jk->isk", sv[:, sl], W[:, sl], om[sl] * live)
        if defect == "clamped_row_stored" and prev is not None and n % B:
            spill = min(B - n % B, n)
            po[:spill], pg[:spill] = prev[0][-1], prev[1][-1]
        prev = (po.copy(), pg.copy())
        out += po
        g += pg
    if defect == "halves_swapped":
        g = np.concatenate([g[:, :, 2 * HD:], g[:, :, :2 * HD]], axis=2)
    amp = np.sqrt(2.0 * variance / F)
    return amp * out, (-float(two_pi) * amp) * g[:, :, :D]


def feature_defect_applies(defect, c) -> bool:
    if defect == "pad_nonzero":
        return hot_width(c["D"]) > c["D"]
    if defect == "clamped_row_stored":
        return c["n_new"] > 1 and c["n_new"] % rows_per_block(c["D"]) != 0 and feature_split(c["n_new"], c["F"], c["D"])[0] > 1
    if defect == "drop_part":      # a lost partial phase shows on a row off the centre: the one training row of N = 1 is the centre itself
        return c["N"] > 1 or c["n_new"] > 1
    return True


def defect_applies(defect, c) -> bool:
    """whether a cell can show a defect at all, from its shape alone: a pair that is neither coincident nor out of range needs a second training
    row or a third new point (the first two new points sit on a training row and at 10^3)"""
    live = c["N"] > 1 or c["n_new"] > 2
    if defect == "pad_nonzero":
        return live and hot_width(c["D"]) > c["D"]
    if defect == "clamped_row_stored":
        return c["N"] > 1 and c["n_new"] > 1 and c["n_new"] % rows_per_block(c["D"]) != 0 and cross_split(c["n_new"], c["N"], c["D"], c["jsplit"])[0] > 1
    return live


# ---- cglb_itergp_predict_grad on wide inputs -----------------------------------------------------------------------------------------------------
PREDICT_RANKS = (8, 33)


def gvar_restatement(kind, N, D, r, wobble: float = 0.0, seed: int = 0):
    """g_var [n, D] = -2 sum_s B G in float64 at love_ref's cache for wide_cases.itergp_case(N, D): B = K_*f R, G its gradient.  Every kernel
    value (love_ref.kernel_matrices) and every gradient term h delta / l^2 is moved by a relative `wobble`."""
    import love_ref
    import matern52_ref as m52
    X, y, h, Xnew = wc.itergp_case(N, D)
    ls, f = np.asarray(h["lengthscales"], dtype=np.float64), h["variance"]
    with m52.oracle_with_matern52():
        Kff, Ksf = love_ref.kernel_matrices(kind, X, Xnew, ls, f, wobble, seed)
    R = love_ref.build(Kff + h["noise"] * np.eye(N), y - h["mean"], r).R
    w = ig.cross_terms(kind, Xnew, X, ls)[1].astype(np.float64)
    if wobble:
        w = w * (1.0 + wobble * np.random.default_rng(seed + 50).uniform(-1.0, 1.0, w.shape))
    B = Ksf @ R
    G = -f * np.einsum("ijk,js->isk", w, R)
    return -2.0 * np.einsum("is,isk->ik", B, G), R


#: tests/test_input_grad_mid_ref_host.py: the largest measured change of g_var under wide_cases.WOBBLE over WOBBLE_SEEDS, in units of
#: f sqrt(C) / l_k, rounded up.  Per case, kind and rank (8 / 33), largest of the three seeds:
#:   (300, 40)  rbf 6.4e-12 2.6e-11 | matern32 2.8e-12 1.4e-11 | matern52 4.0e-12 1.9e-11
#:   (300, 77)  rbf 1.1e-11 3.8e-11 | matern32 4.2e-12 8.78e-11 | matern52 6.2e-12 6.4e-11
GVAR_MEASURED_MAX = 9e-11


def gvar_tolerance(kind, ls, variance):
    """[D]: the larger of 10 x the measured wobble (the margin of wide_cases.cache_tolerance) and the narrow file's 1e-10, of f sqrt(C) / l_k."""
    return max(10.0 * GVAR_MEASURED_MAX, ig.TOL_VAR) * variance * np.sqrt(ig.C_KIND[kind]) / np.asarray(ls, dtype=np.float64).reshape(-1)


#: relative error of the kernel values at precision level 2 (csrc/devmath.h, CGLB_PREC_LOW: a degree-2 table polynomial), as tests/test_gpu_cross_matmat.py
LEVEL2_KERNEL_ERROR = 1.03e-10


def level_tolerance(kind, xnew, X, ls, variance, V, precision: int = 1):
    """input_grad_ref.cross_tolerance; at precision level 2 the error of that level's 2^x is added to its 1e-11, term by term, and nothing else."""
    tv, tg = cross_tolerance(kind, xnew, X, ls, variance, V)
    if precision == 2:
        floor = ig.FLOOR * variance * np.abs(np.asarray(V, dtype=np.float64).reshape(len(X), -1)).sum(axis=0)
        tv = tv + (tv - floor) * (LEVEL2_KERNEL_ERROR / ig.TOL)
        tg = tg + (tg - floor[None, :, None]) * (LEVEL2_KERNEL_ERROR / ig.TOL)
    return tv, tg
