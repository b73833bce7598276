"""Every sharded entry point per rank against the oracle's local op of the same name (tests/shard_cases.py: the case table, the emulated
world, the tolerances).  One process, at most 4 contexts at a time, no process group: the "collectives" are host sums in rank order.  Every
output buffer is pre-filled with NaN, vectors carry one sentinel element past their end, and each check prints its largest error next to its
tolerance (`shard_cases.report`).

Entry points compared here per rank: cglb_vec_dot / update_v_r / residual / update_p / axpy / update_p_seg, cglb_shard_dot / update_v_r / residual /
update_p, cglb_shard_precond_u / precond_z / precond_z_seg, cglb_matvec_cyclic after the weighted-operand hand-off, cglb_shard_obj_phase1 /
phase1_kv / phase2 / obj_w / phase3 / phase3_cyclic / finish.

fp32: the vector primitives at the same round-off bound; z through fp32_error_model.precond_case and TAU['precond']; the rank sums of the
lengthscale and Z gradient blocks and the bound through fp32_error_model.grad_case / bound_scale and their TAU entries.  That model has no entry
for the variance, noise and mean entries of the gradient, for r^T z or for the phase scalars sc[0..5]: those are not compared in fp32.
"""
import numpy as np
import pytest
import torch

import fp32_error_model as em
import geometry_cases as gc
import shard_cases as sc
from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ["fp64", "fp32"]
SENTINEL = 123.0
RZ, PAP, NRZ = 1.7, 0.3, 2.9     # the device scalars of the recurrence


def _np(t, n=None):
    return t.double().cpu().numpy()[:n]


def _padded(w, a):
    """Device copy of `a` with one sentinel element past its end."""
    return w.dev(np.concatenate([np.asarray(a, dtype=np.float64), [SENTINEL]]))


def _tail_ok(t, n):
    return float(t[n].item()) == SENTINEL


def _s(w, x):
    return w.dev([x], scalar=True)


def _check(ops, rc):
    ops._ck(rc)


# =========================================================================== A. vector primitives
VEC_SIZES = (0, 1, 255, 256, 257, 524_288, 524_545, 2_097_152, 2_098_177)


def _vector_ops_at(w, ops, n, shard=False):
    """Every primitive at length n through cglb_vec_* (or, shard=True, the cglb_shard_* twins at n = nloc)."""
    dt = w.dtype
    a = {k: sc.rand(100 + i, n) for i, k in enumerate(("v", "r", "p", "Ap", "z", "b"))}
    lib, h, P = ops.lib, ops.h, ops._p
    # the elementwise kernels take a second grid-stride trip past 2048 * 256 elements, the dot past 2048 * 1024
    tag = f"n={n}{' shard' if shard else ''} {'fp64' if dt == torch.float64 else 'fp32'}"
    # dot
    x, y, out = _padded(w, a["p"]), _padded(w, a["Ap"]), w.nan(1, True)
    _check(ops, lib.cglb_shard_dot(h, P(x), P(y), P(out)) if shard else lib.cglb_vec_dot(h, n, P(x), P(y), P(out)))
    got = float(out.item())
    if n == 0:
        assert got == 0.0
    else:
        sc.report(f"dot {tag}", got - sc.ref_dot(a["p"], a["Ap"]), sc.tol_dot(a["p"], a["Ap"]))
    # v += gamma p ; r -= gamma Ap
    for update_r in (0, 1):
        v, r, p, Ap = (_padded(w, a[k]) for k in ("v", "r", "p", "Ap"))
        if shard:
            ops.update_v_r(v, r, p, Ap, _s(w, RZ), _s(w, PAP), update_r)
        else:
            ops.vec_update_v_r(n, v, r, p, Ap, _s(w, RZ), _s(w, PAP), update_r)
        vr, rr, g = sc.ref_update_v_r(a["v"], a["r"], a["p"], a["Ap"], RZ, PAP, update_r, dt)
        sc.report(f"update_v_r({update_r}) v {tag}", _np(v, n) - vr, sc.tol_elementwise(dt, g * a["p"], a["v"]))
        if update_r:
            sc.report(f"update_v_r({update_r}) r {tag}", _np(r, n) - rr, sc.tol_elementwise(dt, g * a["Ap"], a["r"]))
        else:
            assert np.array_equal(_np(r, n), a["r"])
        assert _tail_ok(v, n) and _tail_ok(r, n)
    # r = b - Kv
    r, b, Kv = w.nan(n + 1), _padded(w, a["b"]), _padded(w, a["Ap"])
    r[n] = SENTINEL
    ops.residual(r, b, Kv) if shard else ops.vec_residual(n, r, b, Kv)
    sc.report(f"residual {tag}", _np(r, n) - sc.ref_residual(a["b"], a["Ap"], dt), sc.tol_elementwise(dt, a["b"], a["Ap"]))
    assert _tail_ok(r, n)
    # p = z + beta p
    for restart in (0, 1):
        p, z = _padded(w, a["p"]), _padded(w, a["z"])
        if shard:
            ops.update_p(p, z, _s(w, NRZ), _s(w, RZ), restart)
        else:
            ops.vec_update_p(n, p, z, _s(w, NRZ), _s(w, RZ), restart)
        pr, beta = sc.ref_update_p(a["p"], a["z"], NRZ, RZ, restart, dt)
        if restart:
            assert np.array_equal(_np(p, n), a["z"])
        else:
            sc.report(f"update_p {tag}", _np(p, n) - pr, sc.tol_elementwise(dt, beta * a["p"], a["z"]))
        assert _tail_ok(p, n)
    if not shard:
        alpha = 1.0 / 3.0
        x, y = _padded(w, a["p"]), _padded(w, a["v"])
        ops.vec_axpy(n, alpha, x, y)
        al = sc.np_dtype(dt)(alpha)
        sc.report(f"axpy {tag}", _np(y, n) - sc.ref_fma(al, a["p"], a["v"], dt), sc.tol_elementwise(dt, float(al) * a["p"], a["v"]))
        assert _tail_ok(y, n)
    # the zero-denominator contract: a zero factor, bitwise; NaN still propagates
    v, r, p, Ap, z = (_padded(w, a[k]) for k in ("v", "r", "p", "Ap", "z"))
    args = (v, r, p, Ap, _s(w, RZ), _s(w, 0.0), 1)
    ops.update_v_r(*args) if shard else ops.vec_update_v_r(n, *args)
    assert np.array_equal(_np(v, n), a["v"]) and np.array_equal(_np(r, n), a["r"]), "pAp = 0 must leave v and r as they are"
    args = (p, z, _s(w, NRZ), _s(w, 0.0), 0)
    ops.update_p(*args) if shard else ops.vec_update_p(n, *args)
    assert np.array_equal(_np(p, n), a["z"]), "rz = 0 must give p = z"
    args = (v, r, p, Ap, _s(w, float("nan")), _s(w, PAP), 1)
    ops.update_v_r(*args) if shard else ops.vec_update_v_r(n, *args)
    assert np.isnan(_np(v, n)).all() and np.isnan(_np(r, n)).all()
    p = _padded(w, a["p"])
    args = (p, z, _s(w, NRZ), _s(w, float("nan")), 0)
    ops.update_p(*args) if shard else ops.vec_update_p(n, *args)
    assert np.isnan(_np(p, n)).all()
    assert _tail_ok(v, n) and _tail_ok(r, n) and _tail_ok(p, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vector_primitives_at_every_grid_edge(dtype):
    """cglb_vec_* on one P2 context (N = 1030; the vectors are as long as n says): n = 0 and 1, one block -+ 1, and both sides of the 2048-block
    cap of the elementwise kernels (524 288) and of the dot (2 097 152)."""
    assert VEC_SIZES[5] == sc.VEC_CAP * 256 and VEC_SIZES[7] == sc.VEC_CAP * 1024
    with sc.emulated_world(sc.CASES["P2"], dtype, world=1) as w:
        for n in VEC_SIZES:
            _vector_ops_at(w, w.hip[0], n)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["P1", "P3"])
def test_shard_twins_of_the_vector_primitives(name, dtype):
    """cglb_shard_* at n = nloc of every rank, the empty and the one-row rank included."""
    with sc.emulated_world(sc.CASES[name], dtype) as w:
        for ops, (r0, r1) in zip(w.hip, w.parts):
            _vector_ops_at(w, ops, r1 - r0, shard=True)


# =========================================================================== B. segmented direction update
def _seg_inputs(w, world, per, n, seed):
    z, partials = sc.rand(seed, n), em.f32(np.abs(sc.rand(seed + 1, world)) + 0.5)
    for g in range(world):
        if min(g * per, n) == min((g + 1) * per, n):
            partials[g] = 0.0                                  # an empty slice contributes a zero partial
    return z, partials, w.dev(sc.seg_layout(world, per, n, z, partials))    # unused elements of short slices hold NaN


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_segmented_update(dtype):
    with sc.emulated_world(sc.CASES["P2"], dtype, world=1) as w:
        ops = w.hip[0]
        for world, per, n in sc.SEG_SHAPES:
            tag = f"update_p_seg world {world} per {per} n {n}"
            z, partials, zseg = _seg_inputs(w, world, per, n, 40 + world)
            want_rz = sc.seg_sum(partials)
            p0 = sc.rand(50 + world, n)
            for restart in (0, 1):
                p, nrz = _padded(w, p0), w.nan(1, True)
                ops.vec_update_p_seg(n, per, world, p, zseg, nrz, _s(w, RZ), restart)
                assert float(nrz.item()) == want_rz, "new_rz is the left-to-right sum of the slices' extra elements"
                got = _np(p, n)
                assert np.isfinite(got).all(), "an unused element of a short slice was read"
                if restart:
                    assert np.array_equal(got, z)
                else:
                    pr, beta = sc.ref_update_p(p0, z, want_rz, RZ, 0, dtype)
                    sc.report(tag, got - pr, sc.tol_elementwise(dtype, beta * p0, z))
                assert _tail_ok(p, n)
            # the driver's first call: new_rz and rz are the same one-element tensor, restart = 1
            p, slot = _padded(w, p0), w.nan(1, True)
            ops.vec_update_p_seg(n, per, world, p, zseg, slot, slot, 1)
            assert float(slot.item()) == want_rz and np.array_equal(_np(p, n), z) and _tail_ok(p, n)
            # the zero-denominator rule of update_p: rz = 0 gives p = z; a NaN scalar still propagates
            p, nrz = _padded(w, p0), w.nan(1, True)
            ops.vec_update_p_seg(n, per, world, p, zseg, nrz, _s(w, 0.0), 0)
            assert np.array_equal(_np(p, n), z), "rz = 0 must give p = z"
            assert float(nrz.item()) == want_rz
            p = _padded(w, p0)
            ops.vec_update_p_seg(n, per, world, p, zseg, nrz, _s(w, float("nan")), 0)
            assert np.isnan(_np(p, n)).all() and _tail_ok(p, n)
            ops.drop_weighted_operand()


# =========================================================================== C. weighted-operand hand-off
def _partial_reference(w, g, p):
    """The oracle's partial of rank g and the mat-vec's established tolerance for it."""
    part = sc.cyclic_partials(w, p)
    full = sum(part)
    if w.dtype == torch.float64:
        return part[g], np.full(w.N, gc.ATOL64 * np.abs(full).max()), 1.0
    case = em.matvec_case(w.kind, w.X, w.oracle[g].hyp, p, chunk=em.sym_chunk(w.N, w.D, w.W))
    return part[g], case.s + em.U * np.abs(part[g]), em.TAU["matvec"]


def _mv(w, g, p_dev):
    out = w.nan(w.N)
    w.hip[g].matvec_cyclic(p_dev, out)
    return _np(out)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("world", [1, 2])
def test_weighted_operand_hand_off(world, dtype):
    """After cglb_vec_update_p_seg(p) the next cglb_matvec_cyclic(p) may skip its weighting pass.  That copy is single-use and is forgotten by
    drop_weighted_operand and by set_hypers: whenever p changed in between, the product is that of the new p."""
    with sc.emulated_world(sc.CASES["P2"], dtype, world=world) as w:
        g = world - 1
        ops, N, per = w.hip[g], w.N, w.per
        z, partials, zseg = _seg_inputs(w, world, per, N, 60)
        q = sc.rand(61, N)                                      # what p is changed to

        def direction():
            p, nrz = w.nan(N), w.nan(1, True)
            ops.vec_update_p_seg(N, per, world, p, zseg, nrz, _s(w, RZ), 1)
            return p

        def check(out, vec, what):
            ref, s, bound = _partial_reference(w, g, vec)
            r = em.ratio(out, ref, s)
            print(f"{what}: max |out - ref| / s = {r:.3g} (bound {bound})")
            assert r <= bound, what

        p = direction()
        handed, fresh = _mv(w, g, p), _mv(w, g, p.clone())
        print(f"world {world} rank {g}: handed-off and re-weighted products bitwise equal: {np.array_equal(handed, fresh)}")
        check(handed, z, "mat-vec after the hand-off")
        check(fresh, z, "mat-vec of a clone at another address")
        p = direction()
        p.copy_(w.dev(q))
        ops.drop_weighted_operand()
        check(_mv(w, g, p), q, "p changed, then drop_weighted_operand")
        p = direction()
        first = _mv(w, g, p)
        assert np.array_equal(first, handed)
        p.copy_(w.dev(q))
        check(_mv(w, g, p), q, "second mat-vec after one update (the copy is single-use)")
        p = direction()
        p.copy_(w.dev(q))
        h = w.oracle[g].hyp
        ls = np.asarray(h.lengthscales) * 1.25
        for o in w.oracle:
            o.set_hypers(ls, h.variance, h.noise, h.mean, h.Z, h.jitter)
        ops.set_hypers(ls, h.variance, h.noise, h.mean, h.Z, h.jitter)
        check(_mv(w, g, p), q, "p changed, then set_hypers with new lengthscales")


# =========================================================================== D. preconditioner pieces per rank
PRECOND_CASES = [(n, torch.float64) for n in sc.CASES] + [(n, torch.float32) for n in sc.FP32]


@pytest.mark.parametrize("name,dtype", PRECOND_CASES, ids=[f"{n}-{'fp64' if d == torch.float64 else 'fp32'}" for n, d in PRECOND_CASES])
def test_preconditioner_pieces_per_rank(name, dtype):
    case = sc.CASES[name]
    fp64 = dtype == torch.float64
    esz = 8 if fp64 else 4
    with sc.emulated_world(case, dtype) as w:
        w.setup()
        M, per, W = w.M, w.per, w.W
        r = sc.rand(70, case.N)
        r_full = w.dev(r)
        assert r_full.data_ptr() % 16 == 0
        us_ref, u_ref, zs_ref, rzs_ref = sc.run_precond(w, r)
        z_ref_full, rz_ref = orc.nystrom_precond(*(lambda t: (t.A, t.LB))(orc.common_terms(case.kind, w.X, w.hyp)), w.hyp.noise, r)
        assert np.abs(np.concatenate(zs_ref) - z_ref_full).max() <= 1e-12 * np.abs(z_ref_full).max()
        own_A = [_np(c.get_matrix("A")).reshape(M, c.nloc) if c.nloc else np.zeros((M, 0)) for c in w.ctx]
        us = []
        for g, (ops, (r0, r1)) in enumerate(zip(w.hip, w.parts)):
            nloc = r1 - r0
            for how in ("own", "view"):
                if nloc == 0:
                    r_loc = w.nan(1)                            # a 1-element dummy for the empty rank
                else:
                    r_loc = r_full[r0:r1].clone() if how == "own" else r_full[r0:r1]
                    if how == "view":
                        assert (r_loc.data_ptr() % 16 == 0) == sc.view_aligned(r0, esz), "the view's alignment is the one the table claims"
                u = w.nan(M + 1)
                ops.precond_u(r_loc, u)
                assert np.isnan(u[M].item())
                got = _np(u, M)
                if nloc == 0:
                    assert np.all(got == 0.0)
                elif fp64:
                    sc.report(f"{name} rank {g} u ({how})", got - us_ref[g], sc.tol_u(w.oracle[g].A, r[r0:r1]))
                else:   # on the context's own panel: what is left is the kernel's double accumulation and one rounding to float
                    ref = own_A[g] @ r[r0:r1]
                    sc.report(f"{name} rank {g} u ({how}, fp32)", got - ref, sc.tol_u(own_A[g], r[r0:r1], dtype, ref))
                if how == "own":
                    us.append(got)
                else:
                    assert np.array_equal(got, us[g]) or not sc.view_aligned(r0, esz), "an aligned view takes the same body as an own allocation"
        u_sum = sum(us)
        if fp64:
            z_tol = sc.tol_z(z_ref_full)
        else:
            LB = np.tril(_np(w.ctx[0].get_matrix("LB")).reshape(M, M))
            z_model, z_scale = em.precond_case(np.concatenate(own_A, axis=1), LB, w.hyp.noise, r)
        gather = w.nan(W * (per + 1))
        for g, (ops, (r0, r1)) in enumerate(zip(w.hip, w.parts)):
            nloc = r1 - r0
            r_loc = r_full[r0:r1] if nloc else w.nan(1)
            results = []
            for with_rz in (True, False):
                z, rz = w.nan(nloc + 1), (w.nan(1, True) if with_rz else None)
                ops.precond_z(r_loc, w.dev(u_sum), z, rz)
                assert np.isnan(z[nloc].item()), "precond_z wrote past its rows"
                results.append(_np(z, nloc))
                if with_rz:
                    rz_g = float(rz.item())
            assert np.array_equal(results[0], results[1]), "z must not depend on the rz slot"
            slot = gather[g * (per + 1): (g + 1) * (per + 1)]
            ops.precond_z_seg(r_loc, w.dev(u_sum), slot, per)
            sl = _np(slot)
            assert np.isnan(sl[nloc:per]).all() and not np.isnan(sl[:nloc]).any() and not np.isnan(sl[per]), "written only at [0, nloc) and at element per"
            assert np.array_equal(sl[:nloc], results[0])
            assert sl[per] == float(sc.np_dtype(dtype)(rz_g)), "element per is this rank's partial of r^T z in the element type"
            if nloc == 0:
                assert rz_g == 0.0 and sl[per] == 0.0
            if fp64:
                sc.report(f"{name} rank {g} z", results[0] - zs_ref[g], z_tol)
                sc.report(f"{name} rank {g} partial of r^T z", rz_g - rzs_ref[g], sc.TOL_RZ * abs(rz_ref))
            else:
                ratio = em.ratio(results[0], z_model[r0:r1], z_scale[r0:r1]) if nloc else 0.0
                print(f"{name} rank {g} z (fp32): max |err| / s = {ratio:.3g} (tau {em.TAU['precond']})")
                assert ratio <= em.TAU["precond"]
        seg = _np(gather).reshape(W, per + 1)
        z_gathered = seg[:, :per].reshape(-1)[:case.N]
        assert not np.isnan(z_gathered).any()
        if fp64:
            sc.report(f"{name} gathered z against the whole problem", z_gathered - z_ref_full, z_tol)
            sc.report(f"{name} r^T z from the gathered partials", sc.seg_sum(seg[:, per]) - rz_ref, sc.TOL_RZ * abs(rz_ref))
        else:
            assert em.ratio(z_gathered, z_model, z_scale) <= em.TAU["precond"]


# =========================================================================== E. objective phases per rank
def _sc_abs(o, v_loc):
    """Sums of the magnitudes of the terms of sc[0..5] over one rank's rows (obj_scalars_kernel)."""
    s = o.hyp.noise
    uu = o.w + 0.5 * v_loc
    return np.array([np.abs(v_loc * (o.res + 0.5 * o.Kv)).sum(), np.abs(o.w * o.res).sum(), np.abs(uu * v_loc).sum(), np.abs(o.w * o.w).sum(),
                     (np.abs(v_loc) + np.abs(o.w)).sum(), np.abs(uu * (o.Kv - s * v_loc)).sum()])


def _compare_phases(w, name, label, got, ref, want, v, cyclic):
    case, D, M = w.case, w.D, w.M
    kv_max = max((np.abs(k).max() for k in ref["Kv"] if len(k)), default=0.0) if not cyclic else 0.0
    w_full = np.concatenate(ref["w"])
    sc_abs = sum(_sc_abs(o, v[r0:r1]) for o, (r0, r1) in zip(w.oracle, w.parts))
    packed = sc.pack_grad(want.grad)
    g_tol = sc.tol_grad(packed, want.bound, D)
    for g, (o, (r0, r1)) in enumerate(zip(w.oracle, w.parts)):
        tag = f"{name} {label} rank {g}"
        # u = A res; on the row path res carries the mat-vec's own established error, gc.ATOL64 max |K v|, through |A|
        sc.report(f"{tag} u_partial", got["u"][g] - ref["u"][g], sc.tol_u(o.A, o.res) + np.abs(o.A).sum(axis=1) * gc.ATOL64 * kv_max)
        sc.report(f"{tag} sc[0..5]", got["sc"][g][:6] - ref["sc"][g][:6], sc.TOL_VALUE * sc_abs)
        assert np.all(got["sc"][g][6:] == 0.0)
        # A w with w = P r held to 1e-9 max |w|
        sc.report(f"{tag} aw_partial", got["aw"][g] - ref["aw"][g], sc.tol_u(o.A, o.w) + np.abs(o.A).sum(axis=1) * sc.tol_z(w_full))
        sc.report(f"{tag} obj_w", got["w"][g] - ref["w"][g], sc.tol_z(w_full))
        sc.report(f"{tag} gradient partial", got["grad"][g] - ref["grad"][g], g_tol)
        if r0 != 0:   # the header places the replicated terms on the shard with row_begin == 0
            sc.report(f"{tag} noise and mean entries are zero", got["grad"][g][D + 1:D + 3], g_tol[D + 1:D + 3])
        for x, y, what in zip(got["fin"][g], (want.bound, want.lower, want.upper, want.logdet), ("bound", "lower", "upper", "logdet")):
            sc.report(f"{tag} {what}", x - y, sc.TOL_VALUE * abs(y))
    sc.report(f"{name} {label} gradient summed over the ranks", got["grad_sum"] - packed, g_tol)


@pytest.mark.parametrize("name", sc.FULL)
def test_objective_phases_per_rank(name):
    case = sc.CASES[name]
    with sc.emulated_world(case) as w:
        w.setup()
        v = sc.rand_v(case)
        want = sc.reference_objective(w, v)
        ref = sc.run_objective(w, v, hip=False, cyclic=False)
        got = sc.run_objective(w, v, hip=True, cyclic=False)
        _compare_phases(w, name, "row-sharded", got, ref, want, v, cyclic=False)
        ref_c = sc.run_objective(w, v, hip=False, cyclic=True, Kv_locals=ref["Kv"])
        got_c = sc.run_objective(w, v, hip=True, cyclic=True, Kv_locals=ref["Kv"])
        _compare_phases(w, name, "cyclic", got_c, ref_c, want, v, cyclic=True)


def test_objective_phases_rank_sums_in_fp32():
    """P2 in fp32: only the rank sums, through fp32_error_model.grad_case / bound_scale and their TAU entries."""
    case = sc.CASES["P2"]
    with sc.emulated_world(case, torch.float32) as w:
        w.setup()
        v = sc.rand_v(case)
        g, sg, wv = em.grad_case(case.kind, w.X, w.y, w.hyp, v)
        bref = orc.objective(case.kind, w.X, w.y, w.hyp, v, run_cg=False)
        s_b = em.bound_scale(case.kind, w.X, w.y, w.hyp, v, wv)
        ref = sc.run_objective(w, v, hip=False, cyclic=False)
        for label, cyclic in (("row-sharded", False), ("cyclic", True)):
            got = sc.run_objective(w, v, hip=True, cyclic=cyclic, Kv_locals=ref["Kv"])
            D = case.D
            ratios = {"grad_ls": em.ratio(got["grad_sum"][:D], g["lengthscales"], sg["lengthscales"]),
                      "grad_Z": em.ratio(got["grad_sum"][D + 3:].reshape(case.M, D), g["Z"], sg["Z"]),
                      "bound": abs(got["fin"][0][0] - bref.bound) / s_b}
            print(f"P2 fp32 {label}: {ratios} (tau {[em.TAU[q] for q in ratios]})")
            assert all(f == got["fin"][0] for f in got["fin"])
            bad = {q: x for q, x in ratios.items() if not x <= em.TAU[q]}
            assert not bad, (label, bad)
