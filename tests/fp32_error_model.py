"""fp32 round-off model of the HIP kernels (test helper, not a test module; runs on any CPU).

The fp32 path is held to what fp32 arithmetic can deliver on the SAME inputs, entry by entry:

* inputs are rounded first (`f32`, `round_hypers`): X, Z, p, y, v go through float32 and back, so the fp64 reference (the oracle's own
  `dense_cov`, `kernel_matrix`, `common_terms`, `nystrom_precond`, `objective_grad`, `grad_roundoff_spread`) and the fp32
  context see identical values.  Lengthscales, variance, noise and mean are doubles on both sides.  What is left between the two
  is the kernel's arithmetic alone;
* next to every reference value sits an error scale s (same shape).  A test asserts |out - ref| <= tau * s with one named tau per
  quantity (`TAU`).

K_ff mat-vec, row i (the kernels' Gram form: d2_ij = a_i + a_j - 2 x_i.x_j on centred, scaled coordinates, `kernels_prep.hip`):

    s_i = u ||p_j E_ij (1 + 2 (a~_i + a~_j))||_j  +  sqrt(n_acc) u ||k_ij p_j||_j  +  u |sum_j k_ij p_j|  +  u noise |p_i|

    (||.||_j: the 2-norm over the columns j)

    u      = 2^-24;
    a~_i   = |(x_i - xbar) / l|^2 in natural units, xbar = the column means of X32 (cglb_set_data): the Gram-form cancellation
             (d2 = a_i + a_j - 2 g_ij rounds three terms whose magnitudes add up to 2 (a~_i + a~_j) at most);
    E_ij   = |dk/d(d2)|: RBF k_ij / 2, Matern-3/2 3/2 var exp(-sqrt3 r) (dk/dr dr = -3/2 var e^-sqrt3r dd2: the square root
             cancels at r -> 0, where sqrt_pos clamps);
    n_acc  = the kernel's accumulation depth: the column chunk of the symmetric kernel (`sym_chunk`, the launcher's own rule) plus the
             row-sum slabs, the column-sum group slabs and the padded width of the Gram chain.

Choice of the probabilistic form (sqrt n, and 2-norms over j instead of sums of absolute values): the inputs are seeded and of
random sign, so the per-pair errors and the fp32 running sums behave as random walks.  The deterministic form (n u, sums of |.|) sits
sqrt(N) above every observed error (measured with the emulation below: median ratio 0.005 at N = 2999), and a 1e-5 relative
lengthscale error would no longer clear it at any shape.  In the probabilistic form the emulation's median ratio is 0.1-0.2 and its
maximum 0.6-2 over all case shapes, while the planted defects clear tau (`test_fp32_error_model_host.py` checks the margin, the teeth
and that s is not vacuous).  Constant factors (the length of the Gram chain, exp2's ulps) are absorbed in tau.

What the model cannot resolve, by design of fp32 itself: a 1e-5 relative change of ONE of D lengthscales moves d2 by ~1e-5 d2_d,
while the Gram form's own round-off is ~u (a~_i + a~_j) ~ u D, so past D ~ 16 (every wide input) the two are of the same size; and
Matern-3/2's dk/dl ~ r e^(-sqrt3 r) vanishes at r -> 0 where the round-off envelope does not.  Measured on the case shapes: the
lengthscale defect clears tau at every RBF shape with D <= 16 (lowest 7.9 against tau 7.7); for Matern-3/2 it reaches 0.48 - 3 tau
(lowest 3.7 at D = 9, N = 63).  The host test asserts > tau for RBF and > 0.4 tau for Matern-3/2 (`LS_DEFECT_MAX_D`).

The cross mat-vec uses the same form with the new rows' own a~ (the same centre and scale).  The K_ff bilinear gradient form
sum_ij u_i v_j dk_ij/dl_d gets the analogous scale with |u_i||v_j| and the per-dimension factor; the small-M algebra (Cholesky of
K_uu, the Woodbury solve) is covered by `orc.grad_roundoff_spread(delta=2^-23)`, a one-ulp probe of Z and the lengthscales, and by
`algebra_probe`, which perturbs K_uu and K_uf by their fp32 backward errors (cond(K_uu) amplifies these, not a probe of Z).
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import scipy.linalg as sla
from scipy.spatial.distance import cdist
import torch

from oracle import cglb_oracle as orc

U = 2.0 ** -24          # unit round-off of float32
LOG2E = 1.0 / math.log(2.0)
SQRT3 = math.sqrt(3.0)
PAD_SIZES = (1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32)   # cglb_internal.h: pad_dim

# |out - ref| <= TAU[q] * s, set from profiles/fp32_error_ratios.json (every observed ratio <= TAU / 4)
TAU = {
    "matvec": 7.7,     # K_ff mat-vec, row shards, cyclic partials, exponent-range edges (GPU max 1.45; the host emulation's max 1.91)
    "cross": 2.4,      # k(X_new, X) v (0.59)
    "A": 5.3,          # L^-1 K_uf / sigma (1.31)
    "L": 0.6,          # chol(K_uu + jitter I) (0.146)
    "precond": 0.6,    # the Nystrom apply on the context's own A, LB (0.145)
    "grad_ls": 28.5,   # lengthscale gradient at a fixed v (7.08: Matern-3/2, D = 24, M = 32 inducing points from the data; 0.18 - 3.1 elsewhere)
    "grad_Z": 4.05,    # inducing-point gradient at a fixed v (1.01 with M = 32 inducing points from the data, ill-conditioned K_uu; 0.06 at M = 6)
    "f_mean": 1.15,    # predictive mean (0.28)
    "f_var": 0.85,     # predictive variance (0.21)
    "bound": 1.65,     # bound at a fixed v (0.41: the same Matern-3/2 D = 24, M = 32 case; <= 0.16 elsewhere)
}


def f32(a):
    """Round to float32 and return float64 (the values an fp32 context holds)."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def round_hypers(hyp: orc.Hypers) -> orc.Hypers:
    """Z rounded through float32; lengthscales, variance, noise, mean and jitter stay doubles (they reach the library as doubles)."""
    h = hyp.copy()
    h.Z = f32(h.Z)
    return h


# --------------------------------------------------------------------------- the case inputs (shared by the GPU and host tests)
KINDS = ("rbf", "matern32")
# every pad_dim bucket (1 2 3 4 6 8 10 12 16 20 24 28 32), at a bucket top or inside one, then the sgemm Gram tiles (D > 32)
MATVEC_D = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 25, 29, 32, 33, 50, 77, 100)
SHARDS = ((0, 1500), (37, 2999), (1500, 2999))   # row ranges of N = 2999
# RBF, D = 2, l = 1: the fp32 fold / clamp switch (oct = 4 hw^2 log2 e = 200) lies at the half-width hw = 5.89
EDGE_CASES = (("hw5.7", dict(hw=5.7)), ("hw6.1", dict(hw=6.1)), ("hw20", dict(hw=20.0)),
              ("dup-l0.03", dict(ls=0.03, dup=True)), ("offset1e3", dict(offset=1e3)))


def problem(N, D, M=8, seed=0):
    """Rounded inputs (X32, y32, hypers with a rounded Z, p32) of a synthetic case."""
    X, y, Z = orc.synthetic_problem(N, D, M, seed=seed + 1000 * D + N)
    rng = np.random.default_rng(seed + D)
    ls = 0.6 * math.sqrt(D) * (0.8 + 0.4 * rng.random(D))
    hyp = orc.Hypers(ls, 0.7, 0.3, 0.1, f32(Z), 1e-6)
    return f32(X), f32(np.nan_to_num(y)), hyp, f32(rng.standard_normal(N))  # (N = 1: y - mean(y) / std(y) is 0 / 0)


def matvec_shapes():
    """(kind, D, N, forced sym_chunk or 0): per D, N = 1, 63, 64 R -+ 1 (the row-block tail of the instance, kinds alternating) and
    N = 2999 with the chunk forced to 128 (both kinds) so that several chunk and slab edges fall inside N."""
    out = []
    for i, D in enumerate(MATVEC_D):
        R = rows_per_lane(D)
        for j, N in enumerate((1, 63, 64 * R - 1, 64 * R + 1)):
            out.append((KINDS[(i + j) % 2], D, N, 0))
        out += [(kind, D, 2999, 128) for kind in KINDS]
    return out


def edge_problem(hw=None, ls=1.0, offset=0.0, dup=False, N=1500):
    """D = 2 on the box [-hw, hw]^2 with its corners and a near-duplicate of one; dup: 200 near-duplicates (1e-4 apart) at a short
    lengthscale, where the Gram form cancels and sqrt_pos clamps (Matern-3/2); offset: the whole set moved far from the origin."""
    hw = 1.0 if hw is None else hw
    rng = np.random.default_rng(12)
    X = rng.uniform(-hw, hw, size=(N, 2))
    X[0], X[1], X[2] = [hw, hw], [-hw, -hw], [hw, -hw]
    X[3] = X[0] * (1 - 1e-6)
    if dup:
        X[N // 2:N // 2 + 200] = X[:200] + 1e-4 * rng.standard_normal((200, 2))
    X32 = f32(X + offset)
    y32 = f32(rng.standard_normal(N))
    hyp = orc.Hypers(np.full(2, ls), 1.3, 0.2, 0.0, X32[:8].copy(), 1e-6)
    return X32, y32, hyp, f32(rng.standard_normal(N))


# --------------------------------------------------------------------------- dispatch facts (the launchers' own rules)
def pad_dim(D: int) -> int:
    for s in PAD_SIZES:
        if D <= s:
            return s
    return D


def rows_per_lane(D: int, dtype: str = "fp32") -> int:
    """Rows per lane of the symmetric kernel's instances (kernels_kff_sym.hip: kff_sym_generic): fp32 8 / 4 / 2 (the default here), fp64
    8 / 4 (up to the padded width CGLB_SYM_R4_MAX_DP = 12) / 2 / 1 (every wider row, the mid-width instances of D = 33 ... 96 included)."""
    dp = pad_dim(D)
    if dtype == "fp64":
        return 8 if dp <= 4 else (4 if dp <= 12 else (2 if dp <= 16 else 1))
    return 8 if dp <= 4 else (4 if dp <= 16 else 2)


def sym_chunk(n: int, D: int, world: int = 1, opt: int = 0, dtype: str = "fp32") -> int:
    """Column chunk of the symmetric mat-vec (kff_sym_generic: halve 1024 until a rank has >= 16k items; option sym_chunk, rounded up
    to the 16-column batch and clamped to the 1024 columns staged in LDS)."""
    rb = 64 * rows_per_lane(D, dtype)
    chunk = 1024
    nrb_rank = ((n + rb - 1) // rb) / world
    while chunk > 128 and nrb_rank * (n / chunk) * 0.5 < 16384.0:
        chunk //= 2
    if opt > 0:
        chunk = opt
    chunk = (chunk + 15) // 16 * 16
    return min(chunk, 1024)


def n_acc(n: int, D: int, chunk: Optional[int] = None) -> int:
    """Accumulation depth of one output: a column chunk, the row-sum slabs, the column-sum group slabs, the Gram chain."""
    chunk = sym_chunk(n, D) if chunk is None else chunk
    rb = 64 * rows_per_lane(D)
    nrb = (n + rb - 1) // rb
    return min(chunk, n) + (n + chunk - 1) // chunk + (nrb + 3) // 4 + pad_dim(D)


# --------------------------------------------------------------------------- pieces of the scales
def centre(X32):
    return X32.mean(axis=0)


def scaled_norm2(Xq, xbar, ls):
    """a~ = |(x - xbar) / l|^2 (natural units)."""
    return (((Xq - xbar) / np.asarray(ls)) ** 2).sum(axis=1)


def envelope(kind, X1, X2, ls, var):
    """E_ij = |dk/d(d2)|: RBF k_ij / 2, Matern-3/2 3/2 var exp(-sqrt3 r)."""
    d2 = cdist(X1 / np.asarray(ls), X2 / np.asarray(ls), "sqeuclidean")
    if orc.kind_id(kind) == orc.RBF:
        return 0.5 * var * np.exp(-0.5 * d2)
    return 1.5 * var * np.exp(-SQRT3 * np.sqrt(d2))


def _cross_scale(kind, Xr, Xc, xbar, hyp, p, nacc):
    ls = np.asarray(hyp.lengthscales, dtype=np.float64)
    d2 = cdist(Xr / ls, Xc / ls, "sqeuclidean")  # direct differences, as orc.scaled_sqdist (which loops over D in numpy)
    K = orc.kernel_from_sqdist(kind, d2, hyp.variance)
    E = 0.5 * K if orc.kind_id(kind) == orc.RBF else 1.5 * hyp.variance * np.exp(-SQRT3 * np.sqrt(d2))
    ar, ac = scaled_norm2(Xr, xbar, hyp.lengthscales), scaled_norm2(Xc, xbar, hyp.lengthscales)
    KP = K * p[None, :]
    gram = U * np.sqrt(((E * p[None, :] * (1.0 + 2.0 * (ar[:, None] + ac[None, :]))) ** 2).sum(axis=1))
    acc = U * math.sqrt(nacc) * np.sqrt((KP ** 2).sum(axis=1))
    return K, gram + acc + U * np.abs(KP.sum(axis=1))


@dataclass
class MatvecCase:
    ref: np.ndarray      # (K_ff + noise I) p on rows [r0, r1)
    s: np.ndarray        # error scale per row
    K: np.ndarray        # K_ff rows (no noise) - for the planted defects
    chunk: int


def matvec_case(kind, X32, hyp: orc.Hypers, p32, r0=0, r1=None, chunk: Optional[int] = None) -> MatvecCase:
    """fp64 reference and scale of the fp32 mat-vec on the rounded inputs (X32, p32 already rounded)."""
    N, D = X32.shape
    r1 = N if r1 is None else r1
    ch = sym_chunk(N, D) if chunk is None else chunk
    K, s = _cross_scale(kind, X32[r0:r1], X32, centre(X32), hyp, p32, n_acc(N, D, ch))
    ref = K @ p32 + hyp.noise * p32[r0:r1]
    s = s + U * hyp.noise * np.abs(p32[r0:r1])
    return MatvecCase(ref, s, K, ch)


def matvec_rows(kind, X32, hyp: orc.Hypers, p32, r0, r1, block=65536):
    """matvec_case's reference and scale on rows [r0, r1) of a large N, the columns taken in blocks (no N x N matrix)."""
    N, D = X32.shape
    xbar = centre(X32)
    ls = np.asarray(hyp.lengthscales, dtype=np.float64)
    Xr = X32[r0:r1]
    ar = scaled_norm2(Xr, xbar, ls)
    ref, g2, a2 = np.zeros(r1 - r0), np.zeros(r1 - r0), np.zeros(r1 - r0)
    for c0 in range(0, N, block):
        Xc, pc = X32[c0:c0 + block], p32[c0:c0 + block]
        d2 = cdist(Xr / ls, Xc / ls, "sqeuclidean")
        K = orc.kernel_from_sqdist(kind, d2, hyp.variance)
        E = 0.5 * K if orc.kind_id(kind) == orc.RBF else 1.5 * hyp.variance * np.exp(-SQRT3 * np.sqrt(d2))
        KP = K * pc[None, :]
        ref += KP.sum(axis=1)
        g2 += ((E * pc[None, :] * (1.0 + 2.0 * (ar[:, None] + scaled_norm2(Xc, xbar, ls)[None, :]))) ** 2).sum(axis=1)
        a2 += (KP ** 2).sum(axis=1)
    s = U * (np.sqrt(g2) + math.sqrt(n_acc(N, D)) * np.sqrt(a2) + np.abs(ref) + hyp.noise * np.abs(p32[r0:r1]))
    return ref + hyp.noise * p32[r0:r1], s


def cross_case(kind, X32, hyp, Xnew32, v32):
    """k(X_new, X) v and its scale (the plain kernel's column split: depth ~ the 1024-column chunk at most)."""
    N, D = X32.shape
    K, s = _cross_scale(kind, Xnew32, X32, centre(X32), hyp, v32, n_acc(N, D, 1024))
    return K @ v32, s


# --------------------------------------------------------------------------- fp32 emulation (torch CPU float32)
def emulate_matvec(kind, X32, hyp, p32, chunk: int, r0=0, r1=None):
    """What an fp32 kernel computes, in torch float32 on the CPU: centred, scaled coordinates rounded to float32, the Gram form
    a_i + a_j + x_i.x_j (RBF, octaves) / a_i + a_j - 2 x_i.x_j (Matern-3/2), float32 exp2, then the row sum taken sequentially column
    by column inside chunks of `chunk` columns and the chunk sums added in order; var and the noise term last."""
    N, D = X32.shape
    r1 = N if r1 is None else r1
    rbf = orc.kind_id(kind) == orc.RBF
    k = math.sqrt(LOG2E) if rbf else SQRT3 * LOG2E
    xs = torch.from_numpy((X32 - centre(X32)) * (k / np.asarray(hyp.lengthscales))).float()
    a = (xs * xs).sum(1)
    g = xs[r0:r1] @ xs.T
    if rbf:
        kap = torch.exp2((-0.5 * a[r0:r1])[:, None] + (-0.5 * a)[None, :] + g)
    else:
        r = torch.sqrt(torch.clamp(a[r0:r1][:, None] + a[None, :] - 2.0 * g, min=0.0))
        kap = (1.0 + r * float(math.log(2.0))) * torch.exp2(-r)
    p = torch.from_numpy(p32).float()
    nch = (N + chunk - 1) // chunk
    terms = torch.zeros((r1 - r0, nch * chunk), dtype=torch.float32)
    terms[:, :N] = kap * p[None, :]
    terms = terms.reshape(r1 - r0, nch, chunk)
    acc = torch.zeros((r1 - r0, nch), dtype=torch.float32)
    for j in range(chunk):           # sequential inside every chunk (all chunks side by side)
        acc = acc + terms[:, :, j]
    total = torch.zeros(r1 - r0, dtype=torch.float32)
    for c in range(nch):             # the chunk sums in order
        total = total + acc[:, c]
    out = torch.tensor(hyp.variance, dtype=torch.float32) * total + torch.tensor(hyp.noise, dtype=torch.float32) * p[r0:r1]
    return out.double().numpy()


# --------------------------------------------------------------------------- planted defects (what a plausible kernel bug does)
def defect_drop_last_column(case: MatvecCase, p32, r0=0, col=-1):
    """Column `col` (default: the last one) missing from every row sum."""
    return case.ref - case.K[:, col] * p32[col]


def defect_drop_pair(case: MatvecCase, p32, i, j, r0=0):
    """One kernel pair missing: row i (local) loses k_ij p_j."""
    out = case.ref.copy()
    out[i] -= case.K[i, j] * p32[j]
    return out


def defect_drop_tail_row(case: MatvecCase, p32, r0=0):
    """The first row of the last 64-row group loses its kernel sum (noise term kept)."""
    out = case.ref.copy()
    n = len(out)
    i = ((n - 1) // 64) * 64
    out[i] -= case.K[i] @ p32
    return out


LS_DEFECT_MAX_D = 16


def defect_lengthscale(kind, X32, hyp, p32, r0=0, r1=None, rel=1e-5):
    """Lengthscale 0 off by `rel` relative."""
    h = hyp.copy()
    h.lengthscales = np.array(h.lengthscales, dtype=np.float64)
    h.lengthscales[0] *= 1.0 + rel
    N = X32.shape[0]
    r1 = N if r1 is None else r1
    return orc.kernel_matrix(kind, X32[r0:r1], X32, h.lengthscales, h.variance) @ p32 + h.noise * p32[r0:r1]


def defect_shard_noise(case: MatvecCase, p32, r0=0, noise=0.0):
    out = case.ref.copy()
    out[0] -= noise * p32[r0]
    return out


def defect_double_column(case: MatvecCase, p32, r0=0):
    """Column `chunk` (the first of the second chunk; the last column if there is one chunk) counted twice."""
    j = min(case.chunk, len(p32) - 1)
    return case.ref + case.K[:, j] * p32[j]


def ratio(out, ref, s) -> float:
    """max_i |out_i - ref_i| / s_i (entries with s_i = 0, such as the zero upper triangle of L, must match exactly)."""
    err = np.abs(np.asarray(out, dtype=np.float64) - ref)
    s = np.broadcast_to(s, err.shape)
    if np.any(err[s == 0] > 0):
        return math.inf
    return float(np.max(err[s > 0] / s[s > 0])) if np.any(s > 0) else 0.0


def quantity(key: str) -> str:
    """The TAU entry of a ratio key: matvec_v2 -> matvec, cross_n77 -> cross."""
    return re.sub(r"_[vn][0-9]+$", "", key)


# --------------------------------------------------------------------------- setup products, preconditioner
def setup_case(kind, X32, hyp):
    """A = L^-1 K_uf / sigma and L = chol(K_uu + jitter I) from the rounded Z, with per-entry scales: a one-ulp probe (2^-23
    relative on Z and the lengthscales, three draws) plus the direct round-off of forming K_uf / K_uu in fp32."""
    terms = orc.common_terms(kind, X32, hyp)
    M = hyp.Z.shape[0]
    xbar = centre(X32)
    sA, sL = np.zeros_like(terms.A), np.zeros_like(terms.L)
    rng = np.random.default_rng(0)
    for _ in range(3):
        hp = hyp.copy()
        hp.Z = hp.Z * (1.0 + 2.0 ** -23 * rng.uniform(-1, 1, hp.Z.shape))
        hp.lengthscales = np.asarray(hp.lengthscales) * (1.0 + 2.0 ** -23 * rng.uniform(-1, 1, len(hp.lengthscales)))
        t = orc.common_terms(kind, X32, hp)
        sA = np.maximum(sA, np.abs(t.A - terms.A))
        sL = np.maximum(sL, np.abs(t.L - terms.L))
    Ekuf = envelope(kind, hyp.Z, X32, hyp.lengthscales, hyp.variance)
    az, ax = scaled_norm2(hyp.Z, xbar, hyp.lengthscales), scaled_norm2(X32, xbar, hyp.lengthscales)
    dKuf = U * (Ekuf * (1.0 + az[:, None] + ax[None, :]) + np.abs(orc.kernel_matrix(kind, hyp.Z, X32, hyp.lengthscales, hyp.variance)))
    Linv = np.abs(sla.solve_triangular(terms.L, np.eye(M), lower=True))
    sA = sA + (Linv @ dKuf) / math.sqrt(hyp.noise) + U * M * (Linv @ np.abs(terms.L)) @ np.abs(terms.A)
    sL = sL + U * (M + 2) * (np.abs(terms.L) @ np.abs(terms.L).T).diagonal()[:, None] ** 0.5 * np.tril(np.ones((M, M)))
    return terms, sA, sL


def precond_case(A, LB, noise, r):
    """z = (r - A^T LB^-T LB^-1 A r) / noise (orc.nystrom_precond on the given A, LB) and its per-entry scale."""
    z, _ = orc.nystrom_precond(A, LB, noise, r)
    N, M = A.shape[1], A.shape[0]
    LBi = np.abs(sla.solve_triangular(LB, np.eye(M), lower=True))
    t = LBi.T @ (LBi @ (np.abs(A) @ np.abs(r)))
    s = U * (np.abs(r) + (math.sqrt(N) + M) * (np.abs(A).T @ t)) / noise
    return z, s


# --------------------------------------------------------------------------- gradient at a fixed v
def algebra_probe(kind, X32, hyp, terms, v32, w, probes=3) -> Dict[str, np.ndarray]:
    """The small-M algebra's own round-off, which a probe of Z alone misses when K_uu is ill-conditioned: a Cholesky factor computed in
    fp32 is the exact factor of K_uu + dK with |dK| <= M u |L||L^T| (backward stability; sqrt(M) here, the probabilistic form of the
    mat-vec scale), and K_uf / K_uu are formed with the Gram-form error of the mat-vec scale.  Each probe factors the perturbed K_uu, rebuilds A and LB in fp64 and takes the gradient at
    the same (v, w); returned: the largest change of each block per entry."""
    M = hyp.Z.shape[0]
    sigma = math.sqrt(hyp.noise)
    ls = np.asarray(hyp.lengthscales, dtype=np.float64)
    xbar = centre(X32)
    az, ax = scaled_norm2(hyp.Z, xbar, ls), scaled_norm2(X32, xbar, ls)
    kuu = orc.kernel_matrix(kind, hyp.Z, hyp.Z, ls, hyp.variance) + hyp.jitter * np.eye(M)
    kuf = orc.kernel_matrix(kind, hyp.Z, X32, ls, hyp.variance)
    aL = np.abs(terms.L)
    duu = U * (math.sqrt(M) * (aL @ aL.T) + envelope(kind, hyp.Z, hyp.Z, ls, hyp.variance) * (1.0 + 2.0 * (az[:, None] + az[None, :])) + np.abs(kuu))
    duf = U * (envelope(kind, hyp.Z, X32, ls, hyp.variance) * (1.0 + 2.0 * (az[:, None] + ax[None, :])) + np.abs(kuf))
    base = orc.objective_grad(kind, X32, hyp, terms, v32, w)
    out = {k: np.zeros_like(np.asarray(base[k], dtype=np.float64)) for k in ("lengthscales", "Z")}
    rng = np.random.default_rng(3)
    for _ in range(probes):
        e = rng.uniform(-1.0, 1.0, (M, M))
        L = np.linalg.cholesky(kuu + duu * np.triu(e) + (duu * np.triu(e, 1)).T)
        A = sla.solve_triangular(L, kuf + duf * rng.uniform(-1.0, 1.0, kuf.shape), lower=True) / sigma
        AAt = A @ A.T
        t = orc.CommonTerms(A=A, LB=np.linalg.cholesky(AAt + np.eye(M)), AAt_diag_sum=float(np.trace(AAt)), L=L)
        g = orc.objective_grad(kind, X32, hyp, t, v32, w)
        for k in out:
            out[k] = np.maximum(out[k], np.abs(np.asarray(g[k]) - np.asarray(base[k])))
    return out


def panel_scale(kind, X32, hyp, terms, w) -> Dict[str, np.ndarray]:
    """Round-off of the inducing-point derivative sums themselves: with the adjoints G_uf, G_uu of the bound (orc.kernel_adjoints) the
    Z gradient is sum_n G_mn h_mn delta_mnd / l_d over the N data points (and sum_m' over the inducing points, twice), the lengthscale
    gradient the same with delta^2.  Each term carries the Gram-form error of its pair, each sum the sqrt-depth accumulation error:
    u (sqrt(n) ||t||_2 + ||t (1 + 2 (a~ + a~'))||_2) per output, as in the mat-vec scale."""
    N, D = X32.shape
    ls = np.asarray(hyp.lengthscales, dtype=np.float64)
    xbar = centre(X32)
    az, ax = scaled_norm2(hyp.Z, xbar, ls), scaled_norm2(X32, xbar, ls)
    Guu, Guf, _, _ = orc.kernel_adjoints(hyp, terms, w, N)
    out = {"lengthscales": np.zeros(D), "Z": np.zeros_like(hyp.Z, dtype=np.float64)}
    for Xc, ac, G, mult in ((X32, ax, Guf, 1.0), (hyp.Z, az, Guu, 2.0)):
        W = orc.kernel_grad_factor(kind, cdist(hyp.Z / ls, Xc / ls, "sqeuclidean"), hyp.variance) * G
        gf = 1.0 + 2.0 * (az[:, None] + ac[None, :])
        n = Xc.shape[0]
        for d in range(D):
            delta = (hyp.Z[:, d][:, None] - Xc[:, d][None, :]) / ls[d]
            tz, tl = W * delta / ls[d], W * delta * delta / ls[d]
            out["Z"][:, d] += mult * U * (math.sqrt(n) * np.sqrt((tz ** 2).sum(axis=1)) + np.sqrt(((tz * gf) ** 2).sum(axis=1)))
            out["lengthscales"][d] += U * (math.sqrt(n * len(az)) * np.sqrt((tl ** 2).sum()) + np.sqrt(((tl * gf) ** 2).sum()))
    return out


def grad_case(kind, X32, y32, hyp, v32):
    """Gradient reference at the fixed v (w = P r from the fp64 preconditioner on the rounded data) and scales for the lengthscale
    and Z blocks: the K_ff bilinear form sum_ij |u_i||v_j||dk_ij/dl_d| (1 + a~_i + a~_j + sqrt n) u, the propagation of the fp32
    mat-vec's error through w (|P^-1| <= 1 / noise), the inducing-point derivative sums (`panel_scale`), the one-ulp spread of Z and
    the lengthscales and `algebra_probe`."""
    N, D = X32.shape
    terms = orc.common_terms(kind, X32, hyp)
    cov = orc.dense_cov(kind, X32, hyp)
    r = (y32 - hyp.mean) - cov @ v32
    w, _ = orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r)
    g = orc.objective_grad(kind, X32, hyp, terms, v32, w)
    ls = np.asarray(hyp.lengthscales, dtype=np.float64)
    uu = np.abs(w + 0.5 * v32)
    av = np.abs(v32)
    xbar = centre(X32)
    a = scaled_norm2(X32, xbar, ls)
    d2 = orc.scaled_sqdist(X32, X32, ls)
    H = orc.kernel_grad_factor(kind, d2, hyp.variance)
    mv = matvec_case(kind, X32, hyp, v32)
    nn = math.sqrt(n_acc(N, D))
    UV = uu[:, None] * av[None, :]
    s_ls = np.zeros(D)
    for d in range(D):
        xd = (X32[:, d] - xbar[d]) / ls[d]
        delta2 = (xd[:, None] - xd[None, :]) ** 2
        gram = H * (delta2 * (1.0 + 2.0 * (a[:, None] + a[None, :])) + (xd ** 2)[:, None] + (xd ** 2)[None, :]) / ls[d]
        s_ls[d] = U * (np.sqrt(((UV * gram) ** 2).sum()) + nn * np.sqrt(((UV * H * delta2 / ls[d]) ** 2).sum()))
    spread = orc.grad_roundoff_spread(kind, X32, hyp, v32, w, probes=3, delta=2.0 ** -23)
    # w = P r carries the fp32 mat-vec's error (|P^-1| <= 1 / noise): probe the gradient with w moved by that bound, random signs
    rng = np.random.default_rng(1)
    gw = orc.objective_grad(kind, X32, hyp, terms, v32, w + mv.s / hyp.noise * rng.choice([-1.0, 1.0], N))
    alg = algebra_probe(kind, X32, hyp, terms, v32, w)
    pan = panel_scale(kind, X32, hyp, terms, w)
    s_Z = pan["Z"] + spread["Z"] + alg["Z"] + np.abs(gw["Z"] - g["Z"]) + U * math.sqrt(N) * np.abs(g["Z"])
    s_ls = s_ls + pan["lengthscales"] + spread["lengthscales"] + alg["lengthscales"] + np.abs(gw["lengthscales"] - g["lengthscales"])
    return g, {"lengthscales": s_ls, "Z": s_Z}, w


# --------------------------------------------------------------------------- prediction at a fixed v
def predict_case(kind, X32, y32, hyp, v32, Xnew32):
    """f_mean, f_var of PredictCG (models.py:334-351) at the given v - the oracle's pieces, without its solve - and their scales.
    f_var = var + |tmp2|^2 - |tmp1|^2 cancels: its scale is u (var + |tmp1|^2 + |tmp2|^2) (times M for the triangular solves),
    absolute, never relative."""
    terms = orc.common_terms(kind, X32, hyp)
    cov = orc.dense_cov(kind, X32, hyp)
    err = y32 - hyp.mean
    res = err - cov @ v32
    cg_mean, s_cross = cross_case(kind, X32, hyp, Xnew32, v32)
    kus = orc.kernel_matrix(kind, hyp.Z, Xnew32, hyp.lengthscales, hyp.variance)
    sigma = math.sqrt(hyp.noise)
    M = hyp.Z.shape[0]
    c = sla.solve_triangular(terms.LB, terms.A @ res, lower=True) / sigma
    tmp1 = sla.solve_triangular(terms.L, kus, lower=True)
    tmp2 = sla.solve_triangular(terms.LB, tmp1, lower=True)
    f_mean = tmp2.T @ c + cg_mean + hyp.mean
    f_var = hyp.variance + (tmp2 ** 2).sum(0) - (tmp1 ** 2).sum(0)
    # res carries the fp32 mat-vec's error: move it by that bound and see the SGPR part move
    mv = matvec_case(kind, X32, hyp, v32)
    rng = np.random.default_rng(2)
    c2 = sla.solve_triangular(terms.LB, terms.A @ (res + mv.s * rng.choice([-1.0, 1.0], len(res))), lower=True) / sigma
    s_mean = s_cross + np.abs(tmp2.T @ (c2 - c)) + U * (M + math.sqrt(len(v32))) * (np.abs(tmp2).T @ np.abs(c) + abs(hyp.mean))
    s_var = U * (M + 2) * (hyp.variance + (tmp1 ** 2).sum(0) + (tmp2 ** 2).sum(0))
    return f_mean, f_var, s_mean, s_var


def bound_scale(kind, X32, y32, hyp, v32, w) -> float:
    """Scale of the bound at a fixed v: the fp32 mat-vec's error through lower = v^T (r + K v / 2) and the error term r^T w / 2, the
    fp32 dot products of the quadratic term (sqrt N deep) and the trace of A A^T in the Jensen log-det term (2-norms over the rows,
    as in the mat-vec scale)."""
    N = X32.shape[0]
    mv = matvec_case(kind, X32, hyp, v32)
    e = y32 - hyp.mean
    r = e - mv.ref
    terms = orc.common_terms(kind, X32, hyp)
    T = terms.AAt_diag_sum
    t = N * hyp.variance / hyp.noise - T
    M = hyp.Z.shape[0]
    nrm = np.linalg.norm
    quad = nrm(v32 * mv.s) + nrm(w * mv.s) + U * math.sqrt(N) * (nrm(v32 * r) + nrm(v32 * mv.ref) + nrm(w * r))
    logdet = U * (M * np.abs(np.log(np.diag(terms.LB))).sum() + math.sqrt(N * M) * T * 0.5 / (1.0 + t / N) + N)
    return float(quad + logdet)
