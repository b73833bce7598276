"""Per-rank cases of the multi-GPU entry points (test helper, not a test module; runs on any CPU).

One process holds the `world` contexts of a case, each with `row_range=parts[g]`, next to the `world` oracle-backed local ops of
tests/sharded_oracle_ops.py.  There is no process group: an all-reduce is a plain sum in rank order, an all-gather a plain concatenation
into a buffer of world * (per + 1) elements.  The same seeded input goes into the HIP op and the oracle op of every rank, so a rank's partial
is compared on its own, before any sum can hide it (tests/test_gpu_shard_ops.py); tests/test_shard_cases_host.py shows on the CPU that the
table selects what it says, that the reference agrees with itself and that each planted defect is told apart.

The table (every case fp64; `fp32`: also run in fp32; `full`: the objective phases run, i.e. an N x N reference may be built):

  P1  N 1029 w 2 D 3  M 7  matern52  per 515: rank 1 starts at an odd row (an fp64 view is at 8 mod 16: scalar body of gemv_u_kernel); nloc 515 / 514:
                                     rank 0 has a vector-body tail; M % 4 = 3 (GU_ROWS clamp)
  P2  N 1030 w 4 D 8  M 33 rbf       per 258, shards 258 / 258 / 258 / 256: row 258 misaligns an fp32 view and aligns an fp64 one; RBF in the unclamped exponent
                                     range: the fused weighted operand.  fp32 too
  P3  N 5    w 4 D 2  M 3  matern52  shards 2, 2, 1, 0: an empty rank and a one-row rank; N below one 256-row block
  P4  N 600  w 3 D 12 M 65 matern52  per 200 against the 256-row cyclic blocks (a block spans two shards); M = 65: two 64-row chunks of gemv_t_kernel, the
                                     second with one row; GU_ROWS tail of 1; padded width <= 16: the 2-rows-per-thread class of the gradient pass
  P6  N 16391 w 2 D 3 M 9  rbf       nloc 8196 / 8195: launch_gemv_u takes nsplit = 2 with chunk 4104; rank 1 starts at row 8196.  Vector and preconditioner
                                     ops only (nothing N x N), fp32 too
  P7  N 300  w 2 D 3  M 6  matern32  the third kernel kind through every per-rank op (P1 ... P6 hold RBF and Matern-5/2 only)

`check_geometry` asserts these claims with the launchers' own rules restated here, so a later change of a threshold fails the table instead of
silently leaving a path unvisited.

Tolerances (functions below; each is one the suite already holds the quantity to, or a round-off bound):
  * elementwise vector primitives: 2 eps_T * (sum of the magnitudes of the terms) - the factor is rounded once to T, the fma once, and the
    reference (np.longdouble, rounded once to T) once: 3 * eps_T / 2 in all;
  * dot: 1e-11 * sum |a_i b_i| in both dtypes (double accumulation) - the bound of the fused PCG tests;
  * u = A r: 1e-11 * sum_ij |A_ij r_j| (one number per u, see tol_u); in fp32 additionally one rounding of the result to float, em.U |u_i| (the kernel accumulates in double);
  * z and r^T z: 1e-9 max |z| and 1e-9 relative (tests/test_gpu_pair_geometry.py); a rank's partial of r^T z takes the scale of the sum;
  * cyclic mat-vec partial: geometry_cases.ATOL64 of max |(K_ff + noise I) p|, fp32 through fp32_error_model.matvec_case and TAU['matvec'];
  * gradient blocks: 1e-8 of the largest entry of the summed reference block; the variance, noise and mean scalars rel 1e-7 + 1e-8 |bound|;
    bound, lower, upper, logdet rel 1e-10.  A rank's partial takes the scale of the sum (partials may cancel).
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import torch

import fp32_error_model as em
import matern52_ref as m52
from cglb_amd.distributed import row_partition
from oracle import cglb_oracle as orc
from sharded_oracle_ops import OracleLocalOps, OracleSymLocalOps

LD = np.longdouble


@dataclass(frozen=True)
class Case:
    name: str
    N: int
    world: int
    D: int
    M: int
    kind: str
    full: bool = True     # objective phases (an N x N reference) are run
    fp32: bool = False    # also run in fp32
    seed: int = 0


CASES: Dict[str, Case] = {c.name: c for c in (
    Case("P1", 1029, 2, 3, 7, "matern52", seed=1),
    Case("P2", 1030, 4, 8, 33, "rbf", fp32=True, seed=2),
    Case("P3", 5, 4, 2, 3, "matern52", seed=3),
    Case("P4", 600, 3, 12, 65, "matern52", seed=4),
    Case("P6", 16391, 2, 3, 9, "rbf", full=False, fp32=True, seed=6),
    Case("P7", 300, 2, 3, 6, "matern32", seed=7),
)}
FULL = [n for n, c in CASES.items() if c.full]
FP32 = [n for n, c in CASES.items() if c.fp32]

# what each case claims (asserted by check_geometry): shard sizes, nsplit of launch_gemv_u per rank, 64-row chunks of gemv_t_kernel
CLAIMS = {
    "P1": dict(per=515, shards=(515, 514), nsplit=(1, 1), tchunks=1),
    "P2": dict(per=258, shards=(258, 258, 258, 256), nsplit=(1, 1, 1, 1), tchunks=1),
    "P3": dict(per=2, shards=(2, 2, 1, 0), nsplit=(1, 1, 1, 1), tchunks=1),
    "P4": dict(per=200, shards=(200, 200, 200), nsplit=(1, 1, 1), tchunks=2),
    "P6": dict(per=8196, shards=(8196, 8195), nsplit=(2, 2), tchunks=1),
    "P7": dict(per=150, shards=(150, 150), nsplit=(1, 1), tchunks=1),
}

SEG_SHAPES = ((1, 600, 600), (3, 200, 600), (4, 258, 1030), (4, 2, 5))   # (world, per, n) of the segmented update; (4, 2, 5): a short and an empty slice
GU_ROWS = 4        # kernels_vec.hip
T_MCHUNK = 64      # launch_precond_z
RB = 256           # row block of the cyclic mat-vec
VEC_CAP = 2048     # vec_grid


def gemv_u_split(M: int, nloc: int):
    """(nsplit, chunk) by the rule of launch_gemv_u."""
    nsplit = 1
    while (M // GU_ROWS) * nsplit < 2048 and nsplit < 64 and nloc // (nsplit * 2) >= 4096:
        nsplit *= 2
    chunk = (nloc + nsplit - 1) // nsplit
    chunk = (chunk + 7) & ~7
    if chunk == 0:
        chunk = 8
    return max((nloc + chunk - 1) // chunk, 1), chunk


def grad_block_rows(D: int, dtype="fp64") -> int:
    """Row-block size of the cyclic K_ff gradient pass (launch_grad_kff_cyclic, narrow inputs, default options): 256 threads x R rows.  fp64 runs the
    Gram-form kernel, R = 4 / 2 / 1 for padded widths <= 4 / <= 12 / wider; fp32 the direct-difference one, R = 2 up to padded width 16, else 1.  Rank r owns the
    blocks b = r (mod world) of the global upper triangle: this decides which rank's partial holds which share of the lengthscale gradient."""
    dp = em.pad_dim(D)
    assert dp <= 32, "the wide path deals its tiles by another rule"
    if dtype in (torch.float32, np.float32, "fp32"):
        return 256 * (2 if dp <= 16 else 1)
    return 256 * (4 if dp <= 4 else (2 if dp <= 12 else 1))


def view_aligned(r0: int, esz: int) -> bool:
    """Whether full[r0:] of a 16-byte aligned allocation is 16-byte aligned (the vector body of gemv_u_kernel)."""
    return (r0 * esz) % 16 == 0


def check_geometry(case: Case):
    per, parts = row_partition(case.N, case.world)
    claim = CLAIMS[case.name]
    assert per == claim["per"], (case.name, per)
    assert tuple(b - a for a, b in parts) == claim["shards"], (case.name, parts)
    assert tuple(gemv_u_split(case.M, b - a)[0] for a, b in parts) == claim["nsplit"], case.name
    assert (case.M + T_MCHUNK - 1) // T_MCHUNK == claim["tchunks"], case.name
    if case.name == "P1":
        assert parts[1][0] % 2 == 1 and not view_aligned(parts[1][0], 8)          # fp64 view at 8 mod 16
        assert (parts[0][1] - parts[0][0]) % 2 == 1                               # vector body (rank 0 is aligned) with a tail of one
        assert case.M % GU_ROWS == 3
    if case.name == "P2":
        assert parts[1][0] % 4 != 0 and not view_aligned(parts[1][0], 4) and view_aligned(parts[1][0], 8)
        assert (parts[0][1] - parts[0][0]) % 4 != 0                               # fp32 vector body with a tail on rank 0
    if case.name == "P3":
        assert case.N < RB
    if case.name == "P4":
        assert per < RB and case.N > 2 * RB and any(a < RB < b for a, b in parts)  # a 256-row block spans two shards
        assert case.M % T_MCHUNK == 1 and case.M % GU_ROWS == 1
        assert 8 < em.pad_dim(case.D) <= 16                                       # padded width 12 or 16
    if case.name == "P6":
        assert all(gemv_u_split(case.M, b - a) == (2, 4104) for a, b in parts) and parts[1][0] == 8196
    return per, parts


# --------------------------------------------------------------------------- inputs
def inputs(case: Case):
    """X, y, hypers of a case: fp32_error_model.problem (float32-representable values, so an fp32 and an fp64 context hold the same numbers)."""
    X, y, hyp, _ = em.problem(case.N, case.D, M=case.M, seed=case.seed)
    return X, y, hyp


def rand(seed, n, scale=1.0):
    """Seeded standard normal (times scale), float32-representable."""
    return em.f32(scale * np.random.default_rng(seed).standard_normal(n))


def rand_v(case: Case):
    return rand(1000 + case.seed, case.N, 0.3)


# --------------------------------------------------------------------------- the emulated world
class World:
    def __init__(self, case, dtype, X, y, hyp, per, parts):
        self.case, self.dtype, self.X, self.y, self.hyp, self.per, self.parts = case, dtype, X, y, hyp, per, parts
        self.N, self.D, self.M, self.W, self.kind = case.N, case.D, case.M, case.world, case.kind
        self.oracle: List[OracleSymLocalOps] = []
        self.ctx, self.hip = [], []
        self.device = None

    # tensors for the HIP ops: device, context dtype (scalars float64); at least one element so that the pointer is never NULL
    def dev(self, a, scalar=False):
        a = np.atleast_1d(np.asarray(a, dtype=np.float64))
        if a.size == 0:
            a = np.full(1, np.nan)
        return torch.from_numpy(a).to(torch.float64 if scalar else self.dtype).to(self.device)

    def nan(self, n, scalar=False):
        return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float64 if scalar else self.dtype, device=self.device)

    def setup(self, hip=True):
        """setup_local on every rank, the host sum of the A A^T partials in rank order, setup_finish."""
        for ops in ([self.oracle, self.hip] if hip and self.hip else [self.oracle]):
            for o in ops:
                o.setup_local()
            total = sum(o.aat_tensor().double().cpu().numpy() for o in ops)
            for o in ops:
                t = o.aat_tensor()
                t.copy_(torch.from_numpy(total).to(t.dtype))
                o.setup_finish()


@contextlib.contextmanager
def emulated_world(case: Case, dtype=torch.float64, gpu=True, profile=m52.k52, grad_factor=m52.h52, world=None):
    """The W oracle ops (and, gpu=True, the W HipContexts / HipSymLocalOps) of a case inside matern52_ref.oracle_with_matern52(); every context is
    closed on exit.  profile / grad_factor: what the oracle uses for kind 2 (the Matern-3/2 ones are a reference-side defect).  world: another world
    size on the same inputs (the hand-off test runs P2 at world 1 and 2)."""
    if world is None:
        per, parts = check_geometry(case)
    else:
        case = Case(case.name, case.N, world, case.D, case.M, case.kind, case.full, case.fp32, case.seed)
        per, parts = row_partition(case.N, world)
    X, y, hyp = inputs(case)
    w = World(case, dtype, X, y, hyp, per, parts)
    with m52.oracle_with_matern52(profile, grad_factor):
        try:
            for g, (r0, r1) in enumerate(parts):
                o = OracleSymLocalOps(case.kind, X, y, hyp.copy(), r0, r1)
                o.set_parallel(case.world, g)
                o.GB = grad_block_rows(case.D, dtype)          # the library's placement of the cyclic N^2 gradient share for this width and dtype
                w.oracle.append(o)
            if gpu:
                from cglb_amd.distributed import HipSymLocalOps
                from cglb_amd.hip_context import HipContext
                for g, (r0, r1) in enumerate(parts):
                    ctx = HipContext(X, y, case.M, case.kind, dtype=dtype, row_range=(r0, r1))
                    w.ctx.append(ctx)
                    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, hyp.Z, hyp.jitter)
                    ops = HipSymLocalOps(ctx)
                    ops.set_parallel(case.world, g)
                    w.hip.append(ops)
                w.device = w.ctx[0].device
            yield w
        finally:
            for ctx in w.ctx:
                ctx.close()


# --------------------------------------------------------------------------- the objective phases with host "collectives"
def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, copy=True).reshape(-1))


def run_objective(w: World, v, hip: bool, cyclic: bool, Kv_locals=None):
    """obj_phase1 (or phase1_kv fed Kv_locals) -> sum u -> phase2 -> sum sc, aw -> obj_w -> phase3 (or phase3_cyclic with u_full = w + v/2 gathered) ->
    finish, on the HIP ops or the oracle ops.  Every output buffer starts as NaN.  Returns per-rank numpy partials and the sums."""
    ops = w.hip if hip else w.oracle
    M, D, N = w.M, w.D, w.N
    glen = D + 3 + M * D
    if hip:
        mk, nan, back = w.dev, w.nan, (lambda t, n=None: t.double().cpu().numpy()[:n])
    else:
        mk = lambda a, scalar=False: _t64(a)
        nan = lambda n, scalar=False: torch.full((int(n),), float("nan"), dtype=torch.float64)
        back = lambda t, n=None: t.numpy().copy()[:n]
    vt = mk(v)
    out = dict(u=[], sc=[], aw=[], w=[], grad=[], fin=[], Kv=[])
    for g, o in enumerate(ops):
        u = nan(M)
        if cyclic:
            o.obj_phase1_kv(mk(Kv_locals[g]), u)
        else:
            o.obj_phase1(vt, u)
        out["u"].append(back(u, M))
    u_sum = sum(out["u"])
    for o in ops:
        sc, aw = nan(8, True), nan(M)
        o.obj_phase2(vt, mk(u_sum), sc, aw)
        out["sc"].append(back(sc, 8))
        out["aw"].append(back(aw, M))
    sc_sum, aw_sum = sum(out["sc"]), sum(out["aw"])
    u_full = np.zeros(N)
    for o, (r0, r1) in zip(ops, w.parts):
        wt = nan(r1 - r0)
        o.obj_w(wt)
        out["w"].append(back(wt, r1 - r0))
        u_full[r0:r1] = out["w"][-1] + 0.5 * v[r0:r1]
    for o in ops:
        grad = nan(glen, True)
        if cyclic:
            o.obj_phase3_cyclic(vt, mk(u_full), mk(sc_sum, True), mk(aw_sum), grad)
        else:
            o.obj_phase3(vt, mk(sc_sum, True), mk(aw_sum), grad)
        out["grad"].append(back(grad, glen))
        out["fin"].append(tuple(float(x) for x in o.obj_finish(mk(sc_sum, True))))
    if not hip:
        out["Kv"] = [o.Kv.copy() for o in ops]
    out.update(u_sum=u_sum, sc_sum=sc_sum, aw_sum=aw_sum, grad_sum=sum(out["grad"]), u_full=u_full)
    return out


def pack_grad(g: dict) -> np.ndarray:
    return np.concatenate([np.asarray(g["lengthscales"], dtype=np.float64).reshape(-1), [g["variance"], g["noise"], g["mean"]],
                           np.asarray(g["Z"], dtype=np.float64).reshape(-1)])


def reference_objective(w: World, v):
    """orc.objective(run_cg=False, with_grad=True) at v on the whole problem (inside the world's oracle patch)."""
    return orc.objective(w.kind, w.X, w.y, w.hyp, v, run_cg=False, with_grad=True)


def run_precond(w: World, r_full, hip=False):
    """precond_u per rank -> sum -> precond_z per rank on the oracle ops: (u partials, u, z partials, rz partials)."""
    us, zs, rzs = [], [], []
    for o, (r0, r1) in zip(w.oracle, w.parts):
        u = torch.zeros(w.M, dtype=torch.float64)
        o.precond_u(_t64(r_full[r0:r1]), u)
        us.append(u.numpy().copy())
    u = sum(us)
    for o, (r0, r1) in zip(w.oracle, w.parts):
        z, rz = torch.zeros(r1 - r0, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        o.precond_z(_t64(r_full[r0:r1]), _t64(u), z, rz)
        zs.append(z.numpy().copy())
        rzs.append(float(rz[0]))
    return us, u, zs, rzs


# --------------------------------------------------------------------------- tolerances
def eps_of(dtype) -> float:
    return float(np.finfo(np.float32 if dtype in (torch.float32, np.float32, "fp32") else np.float64).eps)


def tol_elementwise(dtype, *terms):
    """2 units in the last place of the element type on the sum of the magnitudes of the terms."""
    return 2.0 * eps_of(dtype) * sum(np.abs(np.asarray(t, dtype=np.float64)) for t in terms)


def tol_dot(a, b) -> float:
    return 1e-11 * float(np.abs(np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)).sum())


def tol_u(A, r, dtype=torch.float64, u_ref=None):
    """1e-11 sum_ij |A_ij r_j|, one number for the whole of u (+ one rounding of each entry to float in fp32).  Not per row i: the panel
    A = L^-1 K_uf / sigma comes out of a triangular solve, whose error - in the library and in the oracle alike - is relative to the column, so
    an entry that is small by cancellation is not known to 1e-11 of itself (P3, the one-row rank: 1.4e-16 on an entry of 4e-7 next to one of 2)."""
    t = np.full(A.shape[0], 1e-11 * float((np.abs(A) @ np.abs(r)).sum()))
    if eps_of(dtype) > 1e-10:
        t = t + em.U * np.abs(u_ref)
    return t


def tol_z(z_full) -> float:
    return 1e-9 * float(np.abs(z_full).max()) if len(z_full) else 0.0


TOL_RZ = 1e-9          # relative, on the scale of the summed r^T z
TOL_VALUE = 1e-10      # bound, lower, upper, logdet: relative


def tol_grad(ref_sum: np.ndarray, bound: float, D: int) -> np.ndarray:
    """Per-entry tolerance of a packed gradient (a partial or the sum) from the SUMMED reference."""
    t = np.empty_like(ref_sum)
    t[:D] = 1e-8 * np.abs(ref_sum[:D]).max()
    t[D:D + 3] = 1e-7 * np.abs(ref_sum[D:D + 3]) + 1e-8 * abs(bound)
    t[D + 3:] = 1e-8 * np.abs(ref_sum[D + 3:]).max()
    return t


def worst(err, tol) -> float:
    """max err / tol (0 / 0 counts as 0, err > 0 at tol 0 as inf)."""
    err, tol = np.atleast_1d(np.abs(np.asarray(err, dtype=np.float64))), np.broadcast_to(np.atleast_1d(np.asarray(tol, dtype=np.float64)), np.shape(np.atleast_1d(err)))
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def report(what, err, tol):
    """Print the largest observed error next to its tolerance and assert."""
    r = worst(err, tol)
    e = np.atleast_1d(np.abs(np.asarray(err, dtype=np.float64)))
    print(f"{what}: max |err| = {e.max() if e.size else 0.0:.3g}, max |err| / tol = {r:.3g} (tol up to {np.max(tol) if np.size(tol) else 0.0:.3g})")
    assert r <= 1.0, what


# --------------------------------------------------------------------------- vector references (np.longdouble, rounded once to the element type)
def np_dtype(dtype):
    return np.float32 if dtype in (torch.float32, np.float32, "fp32") else np.float64


def ref_dot(a, b) -> float:
    return float((np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)).sum())


def ref_factor(num, den, dtype):
    """num / den rounded to the element type as the kernels do ((T)(double / double)); a zero denominator gives a zero factor; NaN propagates."""
    num, den = float(num), float(den)
    if den == 0.0 and not math.isnan(num):
        return np_dtype(dtype)(0.0)
    return np_dtype(dtype)(np.float64(num) / np.float64(den)) if den != 0.0 else np_dtype(dtype)(np.nan)


def ref_fma(alpha, x, y, dtype):
    """alpha * x + y with one rounding to the element type."""
    return (LD(alpha) * np.asarray(x, dtype=LD) + np.asarray(y, dtype=LD)).astype(np_dtype(dtype)).astype(np.float64)


def ref_update_v_r(v, r, p, Ap, rz, pAp, update_r, dtype):
    g = ref_factor(rz, pAp, dtype)
    return ref_fma(g, p, v, dtype), (ref_fma(-g, Ap, r, dtype) if update_r else np.asarray(r, dtype=np.float64).copy()), float(g)


def ref_update_p(p, z, new_rz, rz, restart, dtype):
    if restart:
        return np.asarray(z, dtype=np.float64).copy(), 0.0
    b = ref_factor(new_rz, rz, dtype)
    return ref_fma(b, p, z, dtype), float(b)


def ref_residual(b, Kv, dtype):
    return (np.asarray(b, dtype=LD) - np.asarray(Kv, dtype=LD)).astype(np_dtype(dtype)).astype(np.float64)


def seg_layout(world, per, n, z, partials, fill=np.nan):
    """The all-gather buffer of world slices of per + 1 elements: z of rows [g per, (g + 1) per) then that rank's partial; unused elements `fill`."""
    buf = np.full(world * (per + 1), fill, dtype=np.float64)
    for g in range(world):
        a, b = min(g * per, n), min((g + 1) * per, n)
        buf[g * (per + 1): g * (per + 1) + (b - a)] = z[a:b]
        buf[g * (per + 1) + per] = partials[g]
    return buf


def seg_sum(partials) -> float:
    """Left-to-right double sum of the slices' extra elements."""
    s = 0.0
    for x in partials:
        s += float(x)
    return s


# --------------------------------------------------------------------------- reference-side defects (applied to the oracle's results, never to the library)
def defect_u_drops_last_row(op: OracleLocalOps, r_local):
    """u_partial without the last row of the shard."""
    r = np.asarray(r_local, dtype=np.float64)
    return op.A @ r - op.A[:, -1] * r[-1]


def defect_partial_from_wrong_element(zseg, world, per) -> float:
    """new_rz summed from element per - 1 of every slice instead of element per."""
    seg = np.asarray(zseg, dtype=np.float64).reshape(world, per + 1)
    return seg_sum(np.nan_to_num(seg[:, per - 1]))


def replicated_terms(op: OracleLocalOps, v, sc_sum, aw_sum) -> np.ndarray:
    """The rank-replicated part of the packed gradient (what the shard with row_begin == 0 adds once)."""
    saved = (op.r0, op.r1)
    grad = torch.zeros(op.D + 3 + op.M * op.D, dtype=torch.float64)
    op.r0 = op.r1 = 0
    try:
        OracleLocalOps.obj_phase3(op, _t64(v), _t64(sc_sum), _t64(aw_sum), grad)
    finally:
        op.r0, op.r1 = saved
    return grad.numpy().copy()


def defect_replicated_on_every_rank(w: World, ref: dict, v) -> List[np.ndarray]:
    """Per-rank gradient partials with the replicated terms added on every rank."""
    rep = replicated_terms(w.oracle[0], v, ref["sc_sum"], ref["aw_sum"])
    return [g + (rep if r0 != 0 else 0.0) for g, (r0, _) in zip(ref["grad"], w.parts)]


def defect_noise_on_rank1(partials: List[np.ndarray], p, noise) -> List[np.ndarray]:
    out = [q.copy() for q in partials]
    out[0] -= noise * p
    out[1] += noise * p
    return out


def cyclic_partials(w: World, p) -> List[np.ndarray]:
    """The oracle's per-rank partials of (K_ff + noise I) p."""
    outs = []
    for o in w.oracle:
        t = torch.zeros(w.N, dtype=torch.float64)
        o.matvec_cyclic(_t64(p), t)
        outs.append(t.numpy().copy())
    return outs
