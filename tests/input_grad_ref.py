"""Dense np.longdouble restatement of the input-gradient entries of the iterative exact-GP class (test helper, not a test module; runs on any CPU).

    cross_grad    out[i, s] = f sum_j kappa(x*_i, x_j) V[j, s],   gout[i, s, k] = -f sum_j h(x*_i, x_j) (x*_ik - x_jk) / l_k^2 V[j, s]     (cglb_cross_grad_matmat)
    feature_grad  out[i, s] = amp sum_j W[s, j] cos(phi_ij),       gout[i, s, k] = -amp sum_j W[s, j] sin(phi_ij) omega_jk / l_k            (cglb_feature_grad_matmat)
    predict_grad  mean, grad mean, cache variance f - |R^T k_*|^2 and its gradient -2 sum_s B G                                            (cglb_itergp_predict_grad)
    paths         f_s = m + Phi(x*) w_s + K_*f U_s and its gradient                                                                        (cglb_itergp_paths_eval)

h is the radial derivative factor: RBF kappa; Matern-3/2 3 e^(-sqrt3 r); Matern-5/2 (5/3)(1 + sqrt5 r) e^(-sqrt5 r); amp = sqrt(2 f / F); all gradients
with respect to the raw coordinates of the new point.  The last two take a dense Cholesky solve or given alpha / U / R.  Problems, centre, feature
draws and the cache come from gpr_ref.problem, sample_ref.centre, sample_ref.features_from_draws (through sample_ref.sample_draws) and love_ref.build.
Also here: the float64 restatement of the device sine (`sincos_turns`: csrc/devmath.h), the launcher's geometry rules
(csrc/kernels_input_grad.hip), the case tables of tests/test_gpu_input_grad.py, its tolerances, and the planted defects of
tests/test_input_grad_ref_host.py.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg

import gpr_ref
import love_ref
import sample_ref as sr
import slab_rules

LD = np.longdouble
U = 2.0 ** -53
KINDS = sr.KINDS
#: prior variance of df / dx_k in units of f / l_k^2: -kappa''(0) of the unit-lengthscale profile
C_KIND = {"rbf": 1.0, "matern32": 3.0, "matern52": 5.0 / 3.0}
#: the absolute error bound csrc/devmath.h states for the sine of sincos_turns: the cosine's (the sine adds no rounding to its count)
SIN_TURNS_ERR = sr.COS_TURNS_ERR


# ---- the device sine -----------------------------------------------------------------------------------------------------------------------
def _poly(v):
    p = np.full_like(v, sr.COS_COEF[-1])
    for c in sr.COS_COEF[-2::-1]:
        p = p * v + c
    return p


def sincos_turns(phi):
    """(cos(2 pi phi), sin(2 pi phi)) as the device forms them, operation by operation in float64 (no fused multiply-add in numpy: every Horner
    step rounds twice where the device rounds once): the cosine is sample_ref.cos_turns; the sine is the same polynomial at d = 1/4 - |t|."""
    phi = np.asarray(phi, dtype=np.float64)
    t = phi - np.rint(phi)
    d = 0.25 - np.abs(t)
    a = 0.25 - np.abs(d)
    return np.copysign(_poly(a * a), d), np.copysign(_poly(d * d), t)


# ---- the two products ------------------------------------------------------------------------------------------------------------------------
def profiles(kind, d2):
    """(kappa, h) of the unit-variance kernel at the scaled squared distance d2 (np.longdouble)."""
    d2 = np.asarray(d2, dtype=LD)
    if kind == "rbf":
        k = np.exp(-d2 / 2)
        return k, k
    r = np.sqrt(d2)
    if kind == "matern32":
        s = np.sqrt(LD(3)) * r
        return (1 + s) * np.exp(-s), 3 * np.exp(-s)
    if kind == "matern52":
        s = np.sqrt(LD(5)) * r
        return (1 + s + s * s / 3) * np.exp(-s), LD(5) / 3 * (1 + s) * np.exp(-s)
    raise ValueError(kind)


CROSS_DEFECTS = ("sign", "inv_l", "m32_for_m52", "transposed", "drop_group_last", "drop_chunk_last", "coincident_nonzero")
FEATURE_DEFECTS = ("sign", "transposed", "drop_group_last", "drop_chunk_last", "sin_quarter", "centre_kept")
PREDICT_DEFECTS = ("gvar_factor",)


def _block_defects(g, S, defect, group):
    """the defects of the [s][k] output block, shared by the two products"""
    if defect == "sign":
        g = -g
    if defect == "transposed":      # the [S][d] block of a row written as [d][S]
        g = np.ascontiguousarray(np.swapaxes(g, 1, 2)).reshape(g.shape)
    if defect == "drop_group_last" and S % group:   # the last column of the short last group
        g = g.copy()
        g[:, S - 1, :] = 0
    return g


def cross_terms(kind, xnew, X, ls):
    """(kappa [n, N], w [n, N, d]) with w_ijk = h_ij (x*_ik - x_jk) / l_k^2, np.longdouble."""
    ls = np.asarray(ls, dtype=LD).reshape(-1)
    diff = (np.asarray(xnew, dtype=LD)[:, None, :] - np.asarray(X, dtype=LD)[None, :, :]) / ls
    kap, h = profiles(kind, (diff * diff).sum(axis=2))
    return kap, h[:, :, None] * diff / ls


def cross_grad(kind, xnew, X, ls, variance, V, defect=None, chunk=None, group=8):
    """(out [n, S], gout [n, S, d]) in np.longdouble for V [N, S].  `defect`: one of CROSS_DEFECTS (`chunk`, `group`: the launcher's chunk length
    and group width)."""
    V = np.asarray(V, dtype=LD).reshape(len(X), -1)
    lsd = np.asarray(ls, dtype=LD).reshape(-1)
    kap, w = cross_terms("matern32" if (defect == "m32_for_m52" and kind == "matern52") else kind, xnew, X, ls)
    if defect == "m32_for_m52" and kind == "matern52":   # the factor 3 e^(-s) at Matern-5/2's own s = sqrt5 r
        diff = (np.asarray(xnew, dtype=LD)[:, None, :] - np.asarray(X, dtype=LD)[None, :, :]) / lsd
        s = np.sqrt(LD(5) * (diff * diff).sum(axis=2))
        w = (3 * np.exp(-s))[:, :, None] * diff / lsd
        kap = profiles(kind, (diff * diff).sum(axis=2))[0]
    if defect == "inv_l":
        w = w * lsd
    if defect == "coincident_nonzero":   # delta / r taken as 1 at r = 0
        diff = (np.asarray(xnew, dtype=LD)[:, None, :] - np.asarray(X, dtype=LD)[None, :, :])
        hit = (diff == 0).all(axis=2)
        w = w + np.where(hit, profiles(kind, np.zeros(hit.shape))[1], 0)[:, :, None] / lsd
    if defect == "drop_chunk_last":
        w = w.copy()
        w[:, min(chunk, len(X)) - 1, :] = 0
    f = LD(variance)
    out = f * (kap @ V)
    gout = -f * np.einsum("ijk,js->isk", w, V)
    return out, _block_defects(gout, V.shape[1], defect, group)


def feature_grad(x, c, ls, variance, omega, b, W, defect=None, chunk=None, group=8):
    """(out [n, S], gout [n, S, d]) in np.longdouble.  `defect`: one of FEATURE_DEFECTS."""
    W = np.asarray(W, dtype=LD)
    S, F = W.shape
    ph = sr.phases(x, np.zeros_like(np.asarray(c)) if defect == "centre_kept" else c, ls, omega, b)
    sinv = np.sin(ph)
    if defect == "sin_quarter":   # the quarter 1/4 <= t < 1/2 of the folded phase takes the cosine
        t = ph / (2 * np.arccos(LD(-1)))
        t = t - np.rint(t)
        sinv = np.where((t >= 0.25) & (t < 0.5), np.cos(ph), sinv)
    if defect == "drop_chunk_last":
        sinv = sinv.copy()
        sinv[:, min(chunk, F) - 1] = 0
    amp = np.sqrt(LD(2) * LD(variance) / LD(F))
    ol = np.asarray(omega, dtype=LD) / np.asarray(ls, dtype=LD).reshape(-1)          # [F, d]
    out = amp * (np.cos(ph) @ W.T)
    gout = -amp * np.einsum("ij,sj,jk->isk", sinv, W, ol)
    return out, _block_defects(gout, S, defect, group)


def _unpack(X, y, hypers):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    ls = np.broadcast_to(np.asarray(hypers["lengthscales"], dtype=np.float64).reshape(-1), (X.shape[1],))
    return X, np.asarray(y, dtype=np.float64).reshape(-1), ls, float(hypers["variance"]), float(hypers["noise"]), float(hypers["mean"])


def dense_K(kind, X, ls, f, noise):
    K = sr.kernel(kind, X, X, ls, f)
    K[np.diag_indices_from(K)] += noise
    return K


def predict_grad(kind, X, y, hypers, xnew, alpha=None, R=None, rank=None, defect=None):
    """(mean [n], gmean [n, d], var [n] or None, gvar [n, d] or None) in np.longdouble: at the given alpha [N] (None: the dense Cholesky solve) and
    the given cache factor R [N, r_pad] (None: love_ref.build at `rank`; rank None too: no variances)."""
    X, y, ls, f, noise, m = _unpack(X, y, hypers)
    if alpha is None or (R is None and rank is not None):
        K = dense_K(kind, X, ls, f, noise)
    if alpha is None:
        alpha = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), y - m)
    out, g = cross_grad(kind, xnew, X, ls, f, np.asarray(alpha).reshape(-1, 1))
    mean, gmean = m + out[:, 0], g[:, 0, :]
    if R is None and rank is None:
        return mean, gmean, None, None
    if R is None:
        R = love_ref.build(K, y - m, rank).R
    B, G = cross_grad(kind, xnew, X, ls, f, R)
    return mean, gmean, LD(f) - (B * B).sum(axis=1), (-1 if defect == "gvar_factor" else -2) * np.einsum("is,isk->ik", B, G)


def paths(kind, X, y, hypers, xnew, omega, b, W, eps, U=None):
    """(f [S, n], g [S, n, d], U [S, N]) in np.longdouble at the given solves U, or (U None) at the dense Cholesky solves of sample_ref.sample."""
    X, y, ls, f, noise, m = _unpack(X, y, hypers)
    if U is None:
        U = sr.sample(kind, X, y, hypers, xnew, omega, b, W, eps)[1]
    c = sr.centre(X)
    fo, fg = feature_grad(xnew, c, ls, f, omega, b, W)
    ko, kg = cross_grad(kind, xnew, X, ls, f, np.asarray(U).T)
    return (m + fo + ko).T, np.swapaxes(fg + kg, 0, 1), U


# ---- launch geometry (csrc/kernels_input_grad.hip) ---------------------------------------------------------------------------------------------
ROWS = 4096
pad_dim = sr.pad_dim


def rows_per_lane(d: int) -> int:
    return 2 if pad_dim(d) <= 4 else 1


def group_width(d: int) -> int:
    dp = pad_dim(d)
    return 8 if dp <= 8 else (4 if dp <= 16 else 2)


def rows_per_block(d: int) -> int:
    return 256 * rows_per_lane(d)


def _slot_cap(n_rows: int, d: int) -> int:
    return slab_rules.slot_cap(n_rows, group_width(d) * (pad_dim(d) + 1))


def cross_split(n_rows: int, N: int, d: int, forced: int = 0):
    """(chunks, chunk length) of one launch of the cross product (n_rows <= ROWS): the kff_jsplit rule, capped by the slab."""
    bx = (n_rows + rows_per_block(d) - 1) // rows_per_block(d)
    return slab_rules.pair_split(forced, bx, N, _slot_cap(n_rows, d), even=True)


def feature_split(n_rows: int, F: int, d: int):
    """(chunks, chunk length) of one launch of the feature product (n_rows <= ROWS): the feature rule at this kernel's rows per block, capped by the slab."""
    return slab_rules.feature_split(rows_per_block(d), n_rows, F, _slot_cap(n_rows, d))


# ---- tolerances ---------------------------------------------------------------------------------------------------------------------------
#: tests/test_gpu_cross_matmat.py: the tolerance of a sum of kernel values times columns at the precision levels 0 and 1, and the floor of the
#: range-clamped 2^x (2^-1000 times the largest Matern polynomial; the gradient's factor h (x - x') / l^2 <= (5/3)(1 + s) 1.3e3 / 0.8^2 = 8e7 at
#: s = sqrt(5) 1e3 sqrt(32) / 0.8 stays below the same 1e8)
TOL, FLOOR = 1e-11, 2.0 ** -1000 * 1e8
#: tests/test_gpu_itergp_var_cache.py holds the cached variance to this many f
TOL_VAR = 1e-10
#: tests/test_gpu_itergp_sample.py: re-assembly of a sample, of max(|f|, sqrt f)
TOL_SAMPLE = 1e-10


def cross_tolerance(kind, xnew, X, ls, variance, V):
    """(value [n, S], gradient [n, S, d]) per-element tolerances of the cross product: TOL f sum_j |kappa_ij V_js| and TOL f sum_j |h_ij delta_ijk / l_k V_js|
    (delta_k = (x*_k - x_jk) / l_k; with direct differences the factor is as accurate as the value), each plus FLOOR f sum_j |V_js|."""
    kap, w = cross_terms(kind, xnew, X, ls)
    Va = np.abs(np.asarray(V, dtype=np.float64).reshape(len(X), -1))
    floor = FLOOR * variance * Va.sum(axis=0)
    tv = TOL * variance * (np.abs(kap).astype(np.float64) @ Va) + floor
    tg = TOL * variance * np.einsum("ijk,js->isk", np.abs(w).astype(np.float64), Va) + floor[None, :, None]
    return tv, tg


def feature_tolerance(x, c, ls, variance, omega, b, W):
    """(value [n, S], gradient [n, S, d]) per-element tolerances of the feature product, sample_ref.feature_tolerance extended term by term:
      * value: that function at this kernel's chunk count;
      * gradient: each feature's term is weighted by |omega_jk| / l_k and carries the sine's bound in the cosine's place,
        amp sum_j |W_sj| |omega_jk| / l_k (eps_sin + (d + 3) u absphase_ij), the phase error as derived there (the sine has the same Lipschitz
        constant 1);
      * the fixed-order sums: (F / nsplit + nsplit + 8) u amp sum_j |W_sj omega_jk| / l_k - the value's F / nsplit + nsplit + 2 and six roundings
        the gradient adds: omega / (2 pi l) in the operand record (1 / (2 pi l) once, its product), the product t = sin w ahead of the d fused
        multiply-adds, and the constant -2 pi amp (2 pi, its product with amp, the final multiply)."""
    x = np.asarray(x, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    d, F = x.shape[1], len(b)
    z = np.abs((x - c) / ls)
    om = np.abs(np.asarray(omega, dtype=np.float64))
    absphase = z @ om.T + np.abs(np.asarray(b, dtype=np.float64))[None, :]      # [n, F]
    Wabs = np.abs(np.asarray(W, dtype=np.float64))                               # [S, F]
    amp = math.sqrt(2.0 * variance / F)
    nsplit = feature_split(x.shape[0], F, d)[0]
    per_value = sr.COS_TURNS_ERR + (d + 3) * U * absphase
    per_grad = SIN_TURNS_ERR + (d + 3) * U * absphase
    ol = om / ls                                                                # [F, d]
    tv = amp * (per_value @ Wabs.T) + (F / nsplit + nsplit + 2) * U * amp * Wabs.sum(axis=1)[None, :]
    tg = amp * np.einsum("ij,sj,jk->isk", per_grad, Wabs, ol) + (F / nsplit + nsplit + 8) * U * amp * np.einsum("sj,jk->sk", Wabs, ol)[None, :, :]
    return tv, tg


def solve_bound(kind, ls, variance, max_error):
    """[d]: |grad_k (k_*^T d)| <= sqrt(C f) / l_k sqrt(2 max_error) for the error d of a solve stopped at max_error: the bound of cglb_itergp_sample
    with the prior variance C f / l_k^2 of df / dx_k in the place of f (grad_k k_*^T K^-1 grad_k k_* <= C f / l_k^2: a posterior variance is not negative)."""
    return np.sqrt(C_KIND[kind] * variance) / np.asarray(ls, dtype=np.float64).reshape(-1) * math.sqrt(2.0 * max_error)


def gvar_tolerance(kind, ls, variance):
    """[d]: TOL_VAR f sqrt(C) / l_k."""
    return TOL_VAR * variance * math.sqrt(C_KIND[kind]) / np.asarray(ls, dtype=np.float64).reshape(-1)


# ---- cases of tests/test_gpu_input_grad.py -----------------------------------------------------------------------------------------------
DIMS = (1, 3, 8, 9, 20, 32)
N_VALUES = (1, 65, 300)
JSPLITS = (1, 3, 7)
F_VALUES = (1, 65)
#: (rows per lane, group width) -> the D of DIMS that reach it
CLASSES = {(2, 8): (1, 3), (1, 8): (8,), (1, 4): (9,), (1, 2): (20, 32)}


def s_values(d: int):
    g = group_width(d)
    return (1, g, g + 1, 9)


def row_counts(d: int):
    B = rows_per_block(d)
    return (1, 2, B - 1, B, B + 1)


def product_cells():
    """dicts (D, n_new, N, jsplit, S, kind, F): every D with its five row counts, one cell each (30); N, kff_jsplit, S, the kernel kind and F are
    dealt cyclically over the cells with strides that make every value meet every D (S: all four at every D; the three kinds at D = 3 and at
    every other D), the way tests/geometry_cases.py prunes its crossings."""
    cells, x = [], 0
    for a, d in enumerate(DIMS):
        for q, n in enumerate(row_counts(d)):
            cells.append(dict(D=d, n_new=n, N=N_VALUES[(x + a) % 3], jsplit=JSPLITS[(x // 3 + a) % 3], S=s_values(d)[(q + a) % 4], kind=KINDS[(q + a) % 3],
                              F=F_VALUES[(x + q // 2) % 2]))
            x += 1
    for a, d in enumerate(DIMS):   # the fourth S of every D, the last column chunk at several chunks
        cells.append(dict(D=d, n_new=2, N=300, jsplit=JSPLITS[a % 3], S=s_values(d)[(5 + a) % 4], kind=KINDS[a % 3], F=65))
    return cells


def cell_id(c) -> str:
    return "D%d_n%d_N%d_j%d_S%d_%s_F%d" % (c["D"], c["n_new"], c["N"], c["jsplit"], c["S"], c["kind"], c["F"])


def cell_hypers(D: int) -> dict:
    return dict(lengthscales=np.linspace(0.8, 1.9, D) if D > 1 else np.array([1.3]), variance=1.7, noise=0.3, mean=0.1)


def new_points(X, n_new: int):
    """sample_ref.sample_new_points at any N: a training row first (row 3, or the last one of a shorter set), a point at 10^3 second."""
    out = np.random.default_rng(n_new + X.shape[1]).standard_normal((n_new, X.shape[1]))
    out[0] = X[min(3, len(X) - 1)]
    if n_new > 1:
        out[1] = 1e3
    return out


def cell_problem(c):
    """(X, y, xnew, V [N, S], omega, b, W [S, F]) of a cell: gpr_ref.problem with its middle row a duplicate of the row the first new point sits on
    (the middle row is the last pair of no column chunk of these cells, so the pair a "drop_chunk_last" loses is never this coincident one)."""
    X, y = gpr_ref.problem(c["N"], c["D"])
    X = X.copy()
    if c["N"] > 7:
        X[c["N"] // 2] = X[3]
    rng = np.random.default_rng(1000 * c["D"] + 7 * c["n_new"] + c["N"] + c["S"])
    V = rng.standard_normal((c["N"], c["S"]))
    nu = sr.NU[c["kind"]]
    F = c["F"]
    omega, b = sr.features_from_draws(c["kind"], rng.standard_normal((F, c["D"])), None if nu is None else rng.chisquare(2 * nu, F), rng.uniform(0, 1, F))
    return X, y, new_points(X, c["n_new"]), V, omega, b, rng.standard_normal((c["S"], F))


#: cglb_itergp_predict_grad: sample_ref.SAMPLE_CASES[:4] with the rank-8 and rank-33 caches of love_ref.RANKS
PREDICT_CASES = sr.SAMPLE_CASES[:4]
PREDICT_RANKS = (8, 33)
PREDICT_NEW = 17
