"""Dense numpy restatement of the pathwise posterior samples of the iterative exact-GP class (test helper, not a test module; runs on any CPU).

    Phi(x) w_s = sqrt(2 f / F) sum_{j < F} W[s, j] cos( sum_k omega[j, k] (x_k - c_k) / l_k + b_j )          (cglb_feature_matmat)
    f_s(x*)    = m + Phi(x*) w_s + K_*f U_s,   U_s = K^-1 (y - m - Phi(X) w_s - sqrt(noise) eps_s)            (cglb_itergp_sample)

with K = f kappa(X, X) + noise I, m the constant mean and c the training column means as the context forms them (`centre`).  `features` works
in np.longdouble; `sample` solves densely by Cholesky, or re-assembles the sample at given solves U.  Also here: the float64 restatement of
the device cosine (`cos_turns`: the reduction and coefficients of cglb_amd/csrc/devmath.h), the transformation of `draw_features`
(`features_from_draws`), the launcher's geometry rules (`pad_dim`, `rows_per_block`, `feature_split`), the per-element tolerance of the
feature product (`feature_tolerance`), the case tables of the GPU tests and the planted defects of tests/test_sample_ref_host.py.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg

import slab_rules

U = 2.0 ** -53
#: the absolute error bound cglb_amd/csrc/devmath.h states for cos_turns (CGLB_COS_TURNS_ERR)
COS_TURNS_ERR = 3e-16
#: C(v) ~ cos(2 pi sqrt(v)) on 0 <= v <= 1/16, ascending, as in devmath.h (tools/cos_poly_fit.py, degree 8)
COS_COEF = tuple(float.fromhex(h) for h in (
    "0x1.0p+0", "-0x1.3bd3cc9be45dep+4", "0x1.03c1f081b5a9fp+6", "-0x1.55d3c7e3c9051p+6", "0x1.e1f5068620bcbp+5", "-0x1.a6d1f12b0bef2p+4",
    "0x1.f9d2c1f3b2167p+2", "-0x1.b6a6feabe52e9p+0", "0x1.179a329ef4140p-2"))
KINDS = ("rbf", "matern32", "matern52")


def cos_turns(phi):
    """cos(2 pi phi) as the device forms it, operation by operation in float64 (numpy has no fused multiply-add: every Horner step rounds
    twice where the device rounds once, so this restatement's round-off bounds the device's from above)."""
    phi = np.asarray(phi, dtype=np.float64)
    t = phi - np.rint(phi)
    d = 0.25 - np.abs(t)
    a = 0.25 - np.abs(d)
    v = a * a
    p = np.full_like(v, COS_COEF[-1])
    for c in COS_COEF[-2::-1]:
        p = p * v + c
    return np.copysign(p, d)


def centre(X):
    """The column means the context centres by: a sequential sum in row order, divided by N (cglb_set_data)."""
    X = np.asarray(X, dtype=np.float64)
    return np.cumsum(X, axis=0)[-1] / X.shape[0]


def phases(x, c, ls, omega, b, dtype=np.longdouble):
    """[n, F] phases in radians."""
    z = (np.asarray(x, dtype=dtype) - np.asarray(c, dtype=dtype)) / np.asarray(ls, dtype=dtype)
    return z @ np.asarray(omega, dtype=dtype).T + np.asarray(b, dtype=dtype)[None, :]


def features(x, c, ls, variance, omega, b, W, defect=None, chunk=None):
    """[n, S] feature product in np.longdouble.  `defect`: one of FEATURE_DEFECTS (`chunk`: the launcher's chunk length, for "drop_chunk_last")."""
    ld = np.longdouble
    W = np.asarray(W, dtype=ld)
    F = W.shape[1]
    ph = phases(x, np.zeros_like(np.asarray(c)) if defect == "centre_kept" else c, ls, omega, b)
    cosv = np.cos(ph)
    if defect == "sin_quarter":   # the quarter 1/4 <= t < 1/2 of the folded phase takes the sine
        t = ph / (2 * np.arccos(ld(-1)))
        t = t - np.rint(t)
        cosv = np.where((t >= 0.25) & (t < 0.5), np.sin(ph), cosv)
    if defect == "drop_chunk_last":
        cosv = cosv.copy()
        cosv[:, min(chunk, F) - 1] = 0
    if defect == "ninth_as_first":
        W = W.copy()
        W[8::8] = W[0::8][:W[8::8].shape[0]]
    amp = np.sqrt(ld(1 if defect == "amplitude" else 2) * ld(variance) / ld(F))
    return amp * (cosv @ W.T)


FEATURE_DEFECTS = ("drop_chunk_last", "sin_quarter", "amplitude", "centre_kept", "ninth_as_first")
SAMPLE_DEFECTS = ("noise_unscaled",)


def kernel(kind, A, B, ls, variance):
    ls = np.asarray(ls, dtype=np.float64)
    As, Bs = np.asarray(A, dtype=np.float64) / ls, np.asarray(B, dtype=np.float64) / ls
    d2 = np.zeros((As.shape[0], Bs.shape[0]))
    for k in range(As.shape[1]):
        diff = As[:, k][:, None] - Bs[:, k][None, :]
        d2 += diff * diff
    if kind == "rbf":
        return variance * np.exp(-0.5 * d2)
    r = np.sqrt(d2)
    if kind == "matern32":
        return variance * (1.0 + math.sqrt(3.0) * r) * np.exp(-math.sqrt(3.0) * r)
    if kind == "matern52":
        return variance * (1.0 + math.sqrt(5.0) * r + 5.0 / 3.0 * d2) * np.exp(-math.sqrt(5.0) * r)
    raise ValueError(kind)


def sample(kind, X, y, hypers, xnew, omega, b, W, eps, U=None, defect=None):
    """(f [S, n_new], U [S, N]): the samples at the given solves U, or (U None) at the dense Cholesky solves.  `defect`: a planted defect."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    xnew = np.asarray(xnew, dtype=np.float64).reshape(-1, X.shape[1])
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ls = np.broadcast_to(np.asarray(hypers["lengthscales"], dtype=np.float64).reshape(-1), (X.shape[1],))
    f, noise, m = float(hypers["variance"]), float(hypers["noise"]), float(hypers["mean"])
    c = centre(X)
    fdef = defect if defect in FEATURE_DEFECTS else None
    chunk = feature_split(X.shape[0], len(b), X.shape[1])[1]
    if U is None:
        G = features(X, c, ls, f, omega, b, W, fdef, chunk).astype(np.float64)
        sn = 1.0 if defect == "noise_unscaled" else math.sqrt(noise)
        B = (y - m)[None, :] - G.T - sn * np.asarray(eps, dtype=np.float64)
        K = kernel(kind, X, X, ls, f)
        K[np.diag_indices_from(K)] += noise
        U = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), B.T).T
    U = np.asarray(U, dtype=np.float64)
    Gs = features(xnew, c, ls, f, omega, b, W, fdef, feature_split(xnew.shape[0], len(b), X.shape[1])[1]).astype(np.float64)
    return m + Gs.T + (kernel(kind, xnew, X, ls, f) @ U.T).T, U


# ---- draw_features -------------------------------------------------------------------------------------------------------------------
NU = {"rbf": None, "matern32": 1.5, "matern52": 2.5}


def features_from_draws(kind, z, chi2, u):
    """(omega, b) from z [F, d] standard normal, chi2 [F] chi-square of 2 nu degrees of freedom (unused for RBF) and u [F] uniform on [0, 1)."""
    nu = NU[kind]
    z = np.asarray(z, dtype=np.float64)
    omega = z if nu is None else z * np.sqrt(2.0 * nu / np.asarray(chi2, dtype=np.float64))[:, None]
    return omega, 2.0 * math.pi * np.asarray(u, dtype=np.float64)


# ---- launch geometry (cglb_amd/csrc/kernels_feature_multi.hip, cglb_internal.h) ---------------------------------------------------------
PAD = (1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32)
SP = 8


def pad_dim(d: int) -> int:
    return next((p for p in PAD if d <= p), d)


def rows_per_lane(d: int) -> int:
    dp = pad_dim(d)
    if dp > 32:
        return 1   # the looping instance
    r = 4 if dp <= 8 else (2 if dp <= 16 else 1)
    while r > 1 and r * (dp + SP) > 64:
        r //= 2
    return r


def rows_per_block(d: int) -> int:
    return 256 * rows_per_lane(d)


def feature_split(n_rows: int, F: int, d: int):
    """(chunks, chunk length) of one launch: the feature rule at this kernel's rows per block."""
    return slab_rules.feature_split(rows_per_block(d), n_rows, F)


def feature_tolerance(x, c, ls, variance, omega, b, W):
    """[n, S] tolerance of one element of the feature product, every term derived (u = 2^-53):
      * sqrt(2 f / F) sum_j |W_sj| (eps_cos + 2 pi dphi_ij): the evaluator's stated bound, and the phase error
        2 pi dphi_ij = (d + 3) u (sum_k |omega_jk (x_ik - c_k) / l_k| + |b_j|) - the device forms the phase in turns, from operands rounded as
        kernels_feature_multi.hip states: 1 / (2 pi l_k) once, its product with omega_jk, x_ik - c_k (three roundings of a coordinate term), 1 / 2 pi and
        its product with b_j (two of the phase term), then d fused multiply-adds, each rounding a partial sum that the sum of the absolute
        terms bounds: d + 3 roundings in all, as the count the tolerance was set for;
      * (F / nsplit + nsplit + 2) u sqrt(2 f / F) sum_j |W_sj|: the fixed-order sums - a chunk's fused accumulation, the slabs, the amplitude."""
    x = np.asarray(x, dtype=np.float64)
    d, F = x.shape[1], len(b)
    z = np.abs((x - c) / ls)
    absphase = z @ np.abs(np.asarray(omega, dtype=np.float64)).T + np.abs(np.asarray(b, dtype=np.float64))[None, :]   # [n, F]
    Wabs = np.abs(np.asarray(W, dtype=np.float64))                                                                      # [S, F]
    amp = math.sqrt(2.0 * variance / F)
    nsplit = feature_split(x.shape[0], F, d)[0]
    per_feature = COS_TURNS_ERR + (d + 3) * U * absphase                                                                # [n, F]
    return amp * (per_feature @ Wabs.T) + (F / nsplit + nsplit + 2) * U * amp * Wabs.sum(axis=1)[None, :]


# ---- cases of tests/test_gpu_feature_matmat.py -----------------------------------------------------------------------------------------
DIMS = (1, 3, 8, 17, 32, 40)
F_SMALL = (1, 7, 8, 9, 63, 64, 65, 128, 129)   # 64 | 65 and 128 | 129: the edges between one, two and three chunks at up to 2048 row blocks
F_LARGE = (16384, 16385)                        # 256 chunks of 64 | the slot cap: 253 chunks of 65
COLS = (1, 3, 8, 9, 16, 17)
MODES = ("random", "zero_phase", "zero_w", "eighths", "offset", "far")
N_TRAIN, K_PREC = 70, 4


def row_counts(d: int):
    rb = rows_per_block(d)
    return (1, 255, rb - 1, rb, rb + 1)


def feature_cells():
    """(id, D, n_rows, F, S, mode, training) of the covering table: every D with its five row counts (30 cells, F and S dealt cyclically with
    strides that are coprime to their counts, so that every F and every S meets several D and row counts), the large F at one row, the
    exact and far-data modes, and the training rows themselves (x NULL).  At most 40 cells."""
    out = []
    i = 0
    for a, d in enumerate(DIMS):
        for n in row_counts(d):
            F = F_SMALL[(2 * i + a) % len(F_SMALL)]
            S = COLS[(i + a) % len(COLS)]
            out.append((f"D{d}_n{n}_F{F}_S{S}", d, n, F, S, "random", False))
            i += 1
    out.append(("D3_n1_F16384_S9", 3, 1, 16384, 9, "random", False))
    out.append(("D40_n1_F16385_S1", 40, 1, 16385, 1, "random", False))
    for d, mode in ((3, "zero_phase"), (8, "zero_w"), (3, "eighths"), (17, "offset"), (40, "offset"), (8, "far")):
        out.append((f"D{d}_{mode}", d, 255, 65, 9, mode, False))
    # the instance of two rows per lane (padded widths 10 .. 16), which none of DIMS selects: two ragged row blocks, and the training rows
    out.append(("D12_n513_F129_S9", 12, 513, 129, 9, "random", False))
    out.append(("D12_training_rows", 12, N_TRAIN, 65, 17, "random", True))
    return out


def feature_hypers(d: int) -> dict:
    return dict(lengthscales=np.linspace(0.8, 1.9, d) if d > 1 else np.array([1.3]), variance=1.7, noise=0.3, mean=0.1)


def feature_problem(cell):
    """(X, y, x or None, omega, b, W) of a cell: seeded by its shape."""
    _id, d, n, F, S, mode, training = cell
    rng = np.random.default_rng(1000 * d + 7 * n + F + S)
    X = rng.standard_normal((N_TRAIN, d))
    x = 1.5 * rng.standard_normal((n, d))
    if mode == "offset":   # columns at 10^3 +- 1
        X, x = 1e3 + rng.uniform(-1, 1, (N_TRAIN, d)), 1e3 + rng.uniform(-1, 1, (n, d))
    if mode == "far":      # new points at 10^3 in every coordinate
        x = np.full((n, d), 1e3) + rng.uniform(-1, 1, (n, d)) * 1e-3
        x[0] = 1e3
    y = rng.standard_normal(N_TRAIN)
    omega, b, W = rng.standard_normal((F, d)), rng.uniform(0, 2 * math.pi, F), rng.standard_normal((S, F))
    if mode == "zero_phase":
        omega, b = np.zeros((F, d)), np.zeros(F)
    if mode == "zero_w":
        W = np.zeros((S, F))
    if mode == "eighths":   # phases at exact eighths of a turn (to the rounding of 2 pi k / 8 and of the device's 1 / 2 pi)
        omega, b = np.zeros((F, d)), 2 * math.pi * rng.integers(-16, 17, F) / 8.0
    return X, y, (None if training else x), omega, b, W


# ---- cases of tests/test_gpu_itergp_sample.py ------------------------------------------------------------------------------------------
#: (N, D, kind, k): gpr_ref.problem at (N, D); all three kinds at the first shape, Matern-3/2 at the others
SAMPLE_CASES = ((300, 3, "rbf", 8), (300, 3, "matern32", 8), (300, 3, "matern52", 8), (257, 8, "matern32", 8), (200, 40, "matern32", 8))
SAMPLE_F = 65
SAMPLE_S = (1, 9)
SAMPLE_NEW = (1, 17)


def sample_hypers(D: int) -> dict:
    return dict(lengthscales=np.full(D, 1.5 if D < 8 else 2.5), variance=1.3, noise=0.05, mean=0.1)


def sample_new_points(X, n_new: int):
    """n_new points: a training row first, then (n_new > 1) a point at 10^3 in every coordinate, the rest standard normal."""
    D = X.shape[1]
    out = np.random.default_rng(n_new + D).standard_normal((n_new, D))
    out[0] = X[3]
    if n_new > 1:
        out[1] = 1e3
    return out


def sample_draws(N: int, D: int, kind: str, S: int, F: int = SAMPLE_F):
    """(omega, b, W, eps) from fixed numpy draws through `features_from_draws`."""
    rng = np.random.default_rng(N + D + S)
    nu = NU[kind]
    chi2 = None if nu is None else rng.chisquare(2 * nu, F)
    omega, b = features_from_draws(kind, rng.standard_normal((F, D)), chi2, rng.uniform(0, 1, F))
    return omega, b, rng.standard_normal((S, F)), rng.standard_normal((S, N))
