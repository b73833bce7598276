"""References, tolerances and the case table of the predictive paths (test helper, not a test module; runs on any CPU).

Shared by tests/test_gpu_predict_geometry.py (the GPU checks) and tests/test_predict_ref_host.py (the references against each other,
the planted defects, the coverage of the table).

References (numpy, fp64, direct differences):
* `cross`         k(X_new, X) v from oracle.cglb_oracle.kernel_matrix;
* `cglb_predict`  the oracle's `predict` with max_error = 1e300: no CG step, the predictor at exactly the given v;
* `sgpr_predict`  Titsias' predictive in its textbook form (Sigma = K_uu + K_uf K_fu / s), NOT the tmp1 / tmp2 algebra the library and the
                  oracle share;
* the dense exact-GP predictive is tests/gpr_ref.py's.

Inputs: `fp32_error_model.problem` (float32-representable values, lengthscales ~ 0.6 sqrt(D): kernel values 0.01 ... 1 over the whole
matrix) with one of two sets of (variance, noise, mean): `init` (0.7, 0.3, 0.1 - the generator's own) and `trained` (1.0, 0.05, -0.2).
The mean is never 0, so that the fp32 scale of the predictive mean does not vanish where every kernel value underflows.  Jitter 1e-4 and
the generator seed are conditions of the host test (`JITTER`, `SEED`).

New points (`xnew`), in this order: the first min(5, N) training rows, the first min(3, M) inducing points, standard-normal rows and, as
the last row, a point at 1e3 in every coordinate, where every kernel value underflows: mean = mu and variance = f there.  n_new = 1
keeps the first training row and not the far point: at a lone far point every output is mu / f / 0 whatever the kernels read, and no
planted defect (nor any real one) could show.

Tolerances (`cross_ref`, `predict_ref`, `exact_ref`): what the project already holds the same quantities to - fp64 cross mat-vec geometry_cases.ATOL64 max|ref| (narrow),
1e-11 max|ref| (wide, tests/test_gpu_wide.py); fp64 predictor mean and variance 1e-8 of the largest reference entry (predict goldens,
tests/test_gpu_gpr.py, tests/test_gpu_multi_output.py); fp32 the fp32_error_model scale times its TAU with the accumulation depth of the
actual launch; the iterative class sqrt(variance 2e-12) + 1e-9 (tests/test_gpu_itergp.py).  One addition, from the number format alone:
the fp32 cross mat-vec scale gets the floor N max|v| f 2^-126 - at the far point the model's scale is exactly 0 (every k_ij underflows
in fp64 too), while an fp32 kernel value that underflows may come back as anything below the smallest normal float32.

The table (`CASES`).  The two-valued axes (kernel kind, init / trained hyper-parameters, precision level 0 / 1) are not crossed with the
cells; they are dealt by cell number x: kind = x % 2, trained = (x // 2) % 2, precision = (x // 4) % 2.
* A  cross mat-vec, narrow.  B = 256 R (`rows_per_thread`).  Every class (fp64 D = 3, 8, 12, 16, 20, 32; fp32 D = 3, 16, 24) with every
     n_new of (1, 2, 63, 65, B - 1, B, B + 1, 2 B + 17); cell (class c, size j) has x = c + j and takes N = (1, 65, 129, 1100)[x % 4]: the
     eight cells of a class have eight consecutive x, so every class meets every N twice and both values of the three dealt axes.
     Options: kff_rows 1 and 2 on fp64 D = 3 (n_new = B and B + 1 of the changed B), kff_jsplit 1, 3, 7 on fp64 D = 16 (N = 1100).
* B  cglb_predict, narrow: M (1, 31, 32, 33, 65) x n_new (1, 7, 8, 9, 255, 256, 257), N = 130; cell (i, j) takes the class
     ((fp64 | fp32) x D (3, 16, 20))[(i + j) % 6] and x = 7 i + j.  Each cell runs quad_term 0 and 1.  One predict_multi cell (P = 3).
* C  wide: fp64 D = 40 (wide_reg 0 and 1), fp64 D = 100, fp32 D = 40; N = 130, M = 33, n_new (1, 57, 4097); x = 3 c + j.
* D  cglb_gpr_predict: D (1, 8, 20) x n_new (1, 4095, 4096, 4097, 8193); x = 5 i + j, N = (65, 300)[x % 2], kind = (x // 2) % 2,
     trained = (x // 4) % 2 (one precision level: the class has its own kernels).
* E  cglb_itergp_predict: D (3, 20) x n_new (1, 8, 9, 17), N = 257, k = 8, trained hyper-parameters.
* F  three ranks: n_new (1, 2, 4, 10), N = 130, M = 33, D = 3, fp64.

Planted defects (`defects`) - what a plausible index bug does to the outputs, applied to the reference arrays; see each one below.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import scipy.linalg as sla

import fp32_error_model as em
import geometry_cases as gc
import gpr_ref
import slab_rules
from oracle import cglb_oracle as orc

FAR = 1e3
F32_TINY = 2.0 ** -126
HYPER_SETS = {False: (0.7, 0.3, 0.1), True: (1.0, 0.05, -0.2)}   # (variance, noise, mean): init, trained
SEED = 0       # of seeds 0 ... 7 the one whose weakest planted defect is largest (586 x the tolerance: the inducing rows m >= 32 lost at M = 33, fp32)
JITTER = 1e-4   # with 1e-6 the textbook SGPR form loses its 1e-10 at M = 65, D = 3 (RBF): cond(K_uu) ~ M f / jitter

A_CLASSES = (("fp64", 3), ("fp64", 8), ("fp64", 12), ("fp64", 16), ("fp64", 20), ("fp64", 32), ("fp32", 3), ("fp32", 16), ("fp32", 24))
A_N = (1, 65, 129, 1100)
B_CLASSES = (("fp64", 3), ("fp64", 16), ("fp64", 20), ("fp32", 3), ("fp32", 16), ("fp32", 20))
B_M = (1, 31, 32, 33, 65)
B_NNEW = (1, 7, 8, 9, 255, 256, 257)
C_CLASSES = (("fp64", 40, (("wide_reg", 0),)), ("fp64", 40, (("wide_reg", 1),)), ("fp64", 100, ()), ("fp32", 40, ()))
C_NNEW = (1, 57, 4097)
D_N, D_D, D_NNEW = (65, 300), (1, 8, 20), (1, 4095, 4096, 4097, 8193)
E_D, E_NNEW = (3, 20), (1, 8, 9, 17)
F_NNEW = (1, 2, 4, 10)
WIDE_TILE, GPR_BATCH, ITERGP_GROUP, FINISH_BLOCK = 4096, 4096, 8, 256


def rows_per_thread(D: int, kff_rows: int = 4) -> int:
    """kernels_kff.hip: rows_per_thread - whatever the dtype."""
    dp, r = em.pad_dim(D), kff_rows
    if dp > 16:
        r = 1
    elif dp > 8 and r > 2:
        r = 2
    return r if r in (1, 2, 4) else 4


def cross_slabs(n_new: int, N: int, R: int, jsplit_opt: int = 0) -> Tuple[int, int]:
    """(jchunk, slab count) of kff_pairs_range for n_new rows against N columns."""
    count, jchunk = slab_rules.pair_split(jsplit_opt, (n_new + 256 * R - 1) // (256 * R), N, 512, even=True)   # 512: the slots of kff_generic
    return jchunk, count


@dataclass(frozen=True)
class Case:
    group: str
    dtype: str
    D: int
    N: int
    M: int
    n_new: int
    kind: str
    trained: bool
    precision: int
    options: tuple = ()
    block: int = FINISH_BLOCK     # rows of one block / tile / batch / group of the path's output

    @property
    def id(self) -> str:
        opt = "".join(f"-{k}{v}" for k, v in self.options)
        return f"{self.group}-{self.dtype}-D{self.D}-N{self.N}-M{self.M}-n{self.n_new}-{self.kind}-{'tr' if self.trained else 'in'}-p{self.precision}{opt}"

    @property
    def wide(self) -> bool:
        return self.D > 32

    def opt(self, name, default=0):
        return dict(self.options).get(name, default)


def _dealt(x: int):
    return em.KINDS[x % 2], bool((x // 2) % 2), (x // 4) % 2


def _cases():
    out = []
    for c, (dtype, D) in enumerate(A_CLASSES):
        B = 256 * rows_per_thread(D)
        for j, n_new in enumerate((1, 2, 63, 65, B - 1, B, B + 1, 2 * B + 17)):
            x = c + j
            out.append(Case("A", dtype, D, A_N[x % 4], 1, n_new, *_dealt(x), block=B))
    for x, rows in enumerate((1, 2)):
        for k, n_new in enumerate((256 * rows, 256 * rows + 1)):
            out.append(Case("A", "fp64", 3, 1100, 1, n_new, *_dealt(2 * x + k), options=(("kff_rows", rows),), block=256 * rows))
    for x, js in enumerate((1, 3, 7)):
        out.append(Case("A", "fp64", 16, 1100, 1, 65, *_dealt(x + 1), options=(("kff_jsplit", js),), block=512))
    for i, M in enumerate(B_M):
        for j, n_new in enumerate(B_NNEW):
            dtype, D = B_CLASSES[(i + j) % 6]
            out.append(Case("B", dtype, D, 130, M, n_new, *_dealt(7 * i + j)))
    out.append(Case("Bmulti", "fp64", 3, 130, 33, 9, "matern32", True, 1))
    for c, (dtype, D, options) in enumerate(C_CLASSES):
        for j, n_new in enumerate(C_NNEW):
            out.append(Case("C", dtype, D, 130, 33, n_new, *_dealt(3 * c + j), options=options, block=WIDE_TILE))
    for i, D in enumerate(D_D):
        for j, n_new in enumerate(D_NNEW):
            x = 5 * i + j
            out.append(Case("D", "fp64", D, D_N[x % 2], 0, n_new, em.KINDS[(x // 2) % 2], bool((x // 4) % 2), 1, block=GPR_BATCH))
    for i, D in enumerate(E_D):
        for j, n_new in enumerate(E_NNEW):
            out.append(Case("E", "fp64", D, 257, 0, n_new, em.KINDS[(i + j) % 2], True, 1, block=ITERGP_GROUP))
    for j, n_new in enumerate(F_NNEW):
        out.append(Case("F", "fp64", 3, 130, 33, n_new, em.KINDS[j % 2], bool((j // 2) % 2), 1))
    return tuple(out)


CASES = _cases()


def cases(*groups):
    return [c for c in CASES if c.group in groups]


# --------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _problem(N, D, M, trained):
    X, y, hyp, v = em.problem(N, D, M=max(M, 1), seed=SEED)
    hyp.variance, hyp.noise, hyp.mean = HYPER_SETS[trained]
    hyp.jitter = JITTER
    for a in (X, y, v, hyp.Z, hyp.lengthscales):
        a.setflags(write=False)
    return X, y, hyp, v


def problem(case: Case):
    """(X, y, hypers, v) of a case - shared and read-only.  Groups D and E have no inducing points (Z is a placeholder of one row / k rows)."""
    return _problem(case.N, case.D, 8 if case.group == "E" else case.M, case.trained)


def xnew(case: Case) -> np.ndarray:
    X, _, hyp, _ = problem(case)
    n, D = case.n_new, case.D
    rng = np.random.default_rng(1000 * D + n)
    rows = [X[:min(5, case.N)]]
    if case.M > 0:
        rows.append(hyp.Z[:min(3, case.M)])
    rows.append(em.f32(rng.standard_normal((n, D))))
    out = np.concatenate(rows, axis=0)[:n].copy()
    if n >= 2:
        out[-1] = FAR
    return out


# --------------------------------------------------------------------------- references
def cross(kind, X, hyp, v, Xnew):
    return orc.kernel_matrix(kind, Xnew, X, hyp.lengthscales, hyp.variance) @ v


def cglb_predict(kind, X, y, hyp, v, Xnew):
    m, s, _, _ = orc.predict(kind, X, y, hyp, np.asarray(v, dtype=np.float64), Xnew, max_error=1e300)
    return m, s


def sgpr_predict(kind, X, y, hyp, Xnew):
    """Titsias' predictive, textbook form: Sigma = K_uu + jitter I + K_uf K_fu / s; mean = mu + K_*u Sigma^-1 K_uf (y - mu) / s;
    var = k_** - K_*u (K_uu + jitter I)^-1 K_u* + K_*u Sigma^-1 K_u*."""
    ls, f, s = hyp.lengthscales, hyp.variance, hyp.noise
    M = hyp.Z.shape[0]
    Kuu = orc.kernel_matrix(kind, hyp.Z, hyp.Z, ls, f) + hyp.jitter * np.eye(M)
    Kuf = orc.kernel_matrix(kind, hyp.Z, X, ls, f)
    Kus = orc.kernel_matrix(kind, hyp.Z, Xnew, ls, f)
    Sigma = sla.cho_factor(Kuu + Kuf @ Kuf.T / s, lower=True)
    mean = hyp.mean + Kus.T @ sla.cho_solve(Sigma, Kuf @ (y - hyp.mean)) / s
    var = f - (Kus * sla.cho_solve(sla.cho_factor(Kuu, lower=True), Kus)).sum(0) + (Kus * sla.cho_solve(Sigma, Kus)).sum(0)
    return mean, var


@dataclass
class Pieces:
    """The terms of PredictCG.forward (models.py:334-351) at a fixed v, for the planted defects."""
    cg_mean: np.ndarray
    tmp1: np.ndarray   # [M, n_new]
    tmp2: np.ndarray
    c: np.ndarray

    def outputs(self, hyp):
        return self.cg_mean + self.tmp2.T @ self.c + hyp.mean, hyp.variance + (self.tmp2 ** 2).sum(0) - (self.tmp1 ** 2).sum(0)


def predict_pieces(kind, X, y, hyp, v, Xnew) -> Pieces:
    terms = orc.common_terms(kind, X, hyp)
    res = (y - hyp.mean) - orc.dense_cov(kind, X, hyp) @ v
    c = sla.solve_triangular(terms.LB, terms.A @ res, lower=True) / math.sqrt(hyp.noise)
    tmp1 = sla.solve_triangular(terms.L, orc.kernel_matrix(kind, hyp.Z, Xnew, hyp.lengthscales, hyp.variance), lower=True)
    return Pieces(cross(kind, X, hyp, v, Xnew), tmp1, sla.solve_triangular(terms.LB, tmp1, lower=True), c)


@functools.lru_cache(maxsize=None)
def gpr_factor(case: Case):
    X, y, hyp, _ = problem(case)
    return gpr_ref.evaluate(case.kind, X, y, hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, with_grad=False)


# --------------------------------------------------------------------------- tolerances
@dataclass
class Ref:
    ref: np.ndarray
    s: np.ndarray       # per-entry scale
    bound: float        # admissible max |out - ref| / s


def _const(ref, rel):
    return np.full(ref.shape, rel * np.abs(ref).max())


def cross_depth(case: Case) -> int:
    """Accumulation depth of one output of the cross mat-vec: a slab's columns, the slabs, the Gram chain (wide: all columns of one tile)."""
    if case.wide:
        return case.N + case.D
    jchunk, jsplit = cross_slabs(case.n_new, case.N, rows_per_thread(case.D, case.opt("kff_rows", 4)), case.opt("kff_jsplit"))
    return min(jchunk, case.N) + jsplit + em.pad_dim(case.D)


def cross_ref(case: Case, v=None) -> Ref:
    X, _, hyp, p = problem(case)
    v = p if v is None else v
    Xn = xnew(case)
    if case.dtype == "fp32":
        K, s = em._cross_scale(case.kind, Xn, X, em.centre(X), hyp, v, cross_depth(case))
        return Ref(K @ v, s + case.N * np.abs(v).max() * hyp.variance * F32_TINY, em.TAU["cross"])
    ref = cross(case.kind, X, hyp, v, Xn)
    return Ref(ref, _const(ref, 1e-11 if case.wide else gc.ATOL64), 1.0)


def predict_ref(case: Case, quad_term: int, v=None) -> Dict[str, Ref]:
    """{"mean", "var"} of cglb_predict: quad_term 0 at v (default: the case's own) against `cglb_predict`; 1 against `sgpr_predict`."""
    X, y, hyp, p = problem(case)
    v = (np.zeros(case.N) if quad_term else p) if v is None else v
    Xn = xnew(case)
    m, s2 = sgpr_predict(case.kind, X, y, hyp, Xn) if quad_term else cglb_predict(case.kind, X, y, hyp, v, Xn)
    if case.dtype == "fp32":
        _, _, sm, sv = em.predict_case(case.kind, X, y, hyp, v, Xn)
        return {"mean": Ref(m, sm, em.TAU["f_mean"]), "var": Ref(s2, sv, em.TAU["f_var"])}
    return {"mean": Ref(m, _const(m, 1e-8), 1.0), "var": Ref(s2, _const(s2, 1e-8), 1.0)}


def exact_ref(case: Case) -> Dict[str, Ref]:
    """Groups D and E against the dense exact-GP predictive."""
    X, _, hyp, _ = problem(case)
    m, s2 = gpr_ref.predict(case.kind, X, gpr_factor(case), hyp.lengthscales, hyp.variance, hyp.mean, xnew(case))
    if case.group == "E":
        s = np.full(m.shape, math.sqrt(hyp.variance * 2e-12) + 1e-9)
        return {"mean": Ref(m, s, 1.0), "var": Ref(s2, s, 1.0)}
    return {"mean": Ref(m, _const(m, 1e-8), 1.0), "var": Ref(s2, _const(s2, 1e-8), 1.0)}


@functools.lru_cache(maxsize=None)
def references(case: Case) -> Dict[str, Ref]:
    """Every reference of a case, keyed by output: "cross", "mean0" / "var0" (quad_term 0), "mean1" / "var1" (quad_term 1), "mean" / "var"."""
    if case.group == "A":
        return {"cross": cross_ref(case)}
    if case.group in ("D", "E"):
        return exact_ref(case)
    if case.group in ("F", "Bmulti"):
        r = predict_ref(case, 0)
        return {"mean0": r["mean"], "var0": r["var"]}
    out = {"cross": cross_ref(case)} if case.group == "C" else {}
    for q in (0, 1):
        r = predict_ref(case, q)
        out[f"mean{q}"], out[f"var{q}"] = r["mean"], r["var"]
    return out


def far_point(case: Case, refs: Dict[str, Ref]):
    """What the far last row must hold, per output: 0 (cross), mu (mean), f (variance); None for n_new = 1 (no far point)."""
    if case.n_new < 2:
        return None
    _, _, hyp, _ = problem(case)
    return {k: 0.0 if k == "cross" else (hyp.mean if k.startswith("mean") else hyp.variance) for k in refs}


def miss(outs: Dict[str, np.ndarray], refs: Dict[str, Ref]) -> float:
    """max over the outputs of (max_i |out_i - ref_i| / s_i) / bound; inf for an entry that is not finite."""
    worst = 0.0
    for k, out in outs.items():
        if not np.all(np.isfinite(out)):
            return math.inf
        worst = max(worst, em.ratio(out, refs[k].ref, refs[k].s) / refs[k].bound)
    return worst


# --------------------------------------------------------------------------- planted defects
def _edge(case: Case) -> int:
    """Last row of the first block of the output (of the ragged only block)."""
    return min(case.block, case.n_new) - 1


def _arrays(refs):
    return {k: r.ref.copy() for k, r in refs.items()}


def defects(case: Case):
    """(name, damaged outputs) of every planted defect that applies to the case:
    * stale_edge_row      the last row of a row block keeps the value of the row before it (n_new >= 2);
    * unwritten_edge_row  that row is left unwritten (NaN);
    * offset_off_by_one   the second batch / tile / group starts one new point early (GPR batch, wide tile, itergp group; n_new > block);
    * padded_column       column ld - 1 of the tmp1 / tmp2 panels is read for the last new point, ld = (n_new + 7) & ~7 (n_new % 8 != 0).  What
                          the padding holds is undefined; zeros would reproduce the far point's own values, so the model is the realistic
                          stale content: the panel column of training row (ld - 1) % N, left behind by a prediction at the training inputs
                          (the metrics predict there first);
    * lost_inducing_rows  the inducing rows m >= 32 floor((M - 1) / 32) are missing from tmp1 and tmp2;
    * lost_column_slab    the last column slab of the cross mat-vec is dropped (wide: the one column tile);
    * stale_rank_slice    N ranks: the last non-empty slice of new points is filled from the slice before it (n_new >= 2)."""
    refs = references(case)
    X, y, hyp, p = problem(case)
    Xn = xnew(case)
    e, n = _edge(case), case.n_new
    if n >= 2:
        d = _arrays(refs)
        for a in d.values():
            a[e] = a[e - 1]
        yield "stale_edge_row", d
    d = _arrays(refs)
    for a in d.values():
        a[e] = np.nan
    yield "unwritten_edge_row", d
    if case.group in ("C", "D", "E") and n > case.block:
        d = _arrays(refs)
        for k, a in d.items():
            a[case.block:] = refs[k].ref[case.block - 1:-1]
        yield "offset_off_by_one", d
    if case.group in ("B", "Bmulti", "C", "F"):
        M = case.M
        for q in (0, 1):
            if f"mean{q}" not in refs:
                continue
            pc = predict_pieces(case.kind, X, y, hyp, np.zeros(case.N) if q else p, Xn)
            if n % 8:
                ld = (n + 7) & ~7
                stale = predict_pieces(case.kind, X, y, hyp, np.zeros(case.N), X[(ld - 1) % case.N][None, :])
                bad = Pieces(pc.cg_mean, pc.tmp1.copy(), pc.tmp2.copy(), pc.c)
                bad.tmp1[:, -1], bad.tmp2[:, -1] = stale.tmp1[:, 0], stale.tmp2[:, 0]
                yield f"padded_column_q{q}", dict(zip((f"mean{q}", f"var{q}"), bad.outputs(hyp)))
            m0 = 32 * ((M - 1) // 32)
            bad = Pieces(pc.cg_mean, pc.tmp1.copy(), pc.tmp2.copy(), pc.c)
            bad.tmp1[m0:], bad.tmp2[m0:] = 0.0, 0.0
            yield f"lost_inducing_rows_q{q}", dict(zip((f"mean{q}", f"var{q}"), bad.outputs(hyp)))
    if "cross" in refs:
        if case.wide:
            j0 = 0
        else:
            jchunk, jsplit = cross_slabs(n, case.N, rows_per_thread(case.D, case.opt("kff_rows", 4)), case.opt("kff_jsplit"))
            j0 = (jsplit - 1) * jchunk
        K = orc.kernel_matrix(case.kind, Xn, X[j0:], hyp.lengthscales, hyp.variance)
        yield "lost_column_slab", {"cross": refs["cross"].ref - K @ p[j0:]}
    if case.group == "F" and n >= 2:
        pern = (n + 2) // 3
        a = ((n - 1) // pern) * pern            # first row of the last non-empty slice
        d = _arrays(refs)
        for k, arr in d.items():
            arr[a:] = refs[k].ref[a - pern:a - pern + (n - a)]
        yield "stale_rank_slice", d


# --------------------------------------------------------------------------- GPU side (imported lazily: the module itself needs no GPU)
def make_ctx(case: Case, M=None, device=None):
    """Context of a case with its options and hyper-parameters set (no common terms yet)."""
    import torch
    from cglb_amd.hip_context import HipContext
    X, y, hyp, _ = problem(case)
    ctx = HipContext(X, y, hyp.Z.shape[0] if M is None else M, case.kind, dtype=torch.float64 if case.dtype == "fp64" else torch.float32, device=device)
    try:
        ctx.set_option("precision", case.precision)
        for k, v in case.options:
            ctx.set_option(k, v)
        ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _poisoned(ctx, *shape):
    import torch
    return torch.full(shape, float("nan"), dtype=ctx.dtype, device=ctx.device)


def _host(t, what):
    a = t.double().cpu().numpy()
    assert np.all(np.isfinite(a)), f"{what}: {int((~np.isfinite(a)).sum())} of {a.size} entries were never written (first at {np.argwhere(~np.isfinite(a))[0].tolist()})"
    return a


def _p(t):
    from ctypes import c_void_p
    return c_void_p(t.data_ptr())


def cross_matvec(ctx, Xnew, v):
    """cglb_cross_matvec into an output pre-filled with NaN."""
    from cglb_amd import _lib
    xn, vd = ctx._xnew(Xnew), ctx._dev(v, ctx.N)
    out = _poisoned(ctx, xn.shape[0])
    _lib.check(ctx.lib.cglb_cross_matvec(ctx._ctx, _p(xn), xn.shape[0], _p(vd), _p(out)), ctx._ctx)
    return _host(out, "cross mat-vec")


def _two(ctx, entry, what, n, *args):
    from cglb_amd import _lib
    mean, var = _poisoned(ctx, n), _poisoned(ctx, n)
    _lib.check(entry(ctx._ctx, *args, _p(mean), _p(var)), ctx._ctx)
    return _host(mean, what + " mean"), _host(var, what + " variance")


def predict(ctx, v, Xnew):
    """cglb_predict into outputs pre-filled with NaN; v may hold NaN (quad_term 1 must not read it)."""
    xn, vd = ctx._xnew(Xnew), ctx._dev(v, ctx.N)
    return _two(ctx, ctx.lib.cglb_predict, "cglb_predict", xn.shape[0], _p(vd), _p(xn), xn.shape[0])


def dist_predict(ctx, v, Xnew):
    """cglb_dist_predict (a DistHipContext) into outputs pre-filled with NaN."""
    xn, vd = ctx._xnew(Xnew), ctx._dev(v, ctx.N)
    return _two(ctx, ctx.lib.cglb_dist_predict, "cglb_dist_predict", xn.shape[0], _p(vd), _p(xn), xn.shape[0])


def predict_multi(ctx, V, Xnew):
    """cglb_predict_multi: (mean [P, n_new], var [n_new]) from V [N, P]."""
    from cglb_amd import _lib
    xn, Vt = ctx._xnew(Xnew), ctx._cols(V, ctx.P)
    n = xn.shape[0]
    mean, var = _poisoned(ctx, ctx.P, n), _poisoned(ctx, n)
    _lib.check(ctx.lib.cglb_predict_multi(ctx._ctx, _p(Vt), _p(xn), n, _p(mean), _p(var)), ctx._ctx)
    return _host(mean, "cglb_predict_multi mean"), _host(var, "cglb_predict_multi variance")


def gpr_predict(ctx, Xnew):
    xn = ctx._xnew(Xnew)
    return _two(ctx, ctx.lib.cglb_gpr_predict, "cglb_gpr_predict", xn.shape[0], _p(xn), xn.shape[0])


def itergp_predict(ctx, Xnew, max_error, max_cg_iter=1000):
    from cglb_amd import _lib
    xn = ctx._xnew(Xnew)
    n = xn.shape[0]
    mean, var = _poisoned(ctx, n), _poisoned(ctx, n)
    _lib.check(ctx.lib.cglb_itergp_predict(ctx._ctx, _p(xn), n, float(max_error), int(max_cg_iter), _p(mean), _p(var)), ctx._ctx)
    return _host(mean, "cglb_itergp_predict mean"), _host(var, "cglb_itergp_predict variance")


def check(case: Case, outs: Dict[str, np.ndarray], refs: Dict[str, Ref], what="") -> float:
    """Every output against its reference and, at the far point, against mu / f / 0; prints the worst ratio (in units of the bound)."""
    far = far_point(case, refs)
    worst = 0.0
    for k, out in outs.items():
        r = refs[k]
        assert out.shape == r.ref.shape, (k, out.shape, r.ref.shape)
        ratio = em.ratio(out, r.ref, r.s) / r.bound
        line = f"{case.id} {what}{k}: max |out - ref| / (bound s) = {ratio:.3g}"
        if far is not None:
            fr = abs(out[-1] - far[k]) / (r.s[-1] * r.bound)
            line += f", far point {fr:.3g}"
            ratio = max(ratio, fr)
        print(line)
        worst = max(worst, ratio)
    assert worst <= 1.0, f"{case.id} {what}: {worst:.3g} times the tolerance"
    return worst
