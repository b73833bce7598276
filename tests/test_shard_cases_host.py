"""The per-rank case table of tests/shard_cases.py on the CPU: it selects what its docstring says, its reference agrees with itself, each
reference-side defect is told apart at 10x the GPU tolerance or more, and the vector references agree with math.fsum / np.longdouble."""
import math

import numpy as np
import pytest
import torch

import geometry_cases as gc
import matern52_ref as m52
import shard_cases as sc
from cglb_amd.distributed import row_partition
from oracle import cglb_oracle as orc

SELF_TOL = 1e-12   # oracle ops summed over ranks against orc.objective / orc.nystrom_precond (measured: 9e-14 at most)
TEETH = 10.0       # a defect moves a compared quantity by at least this many GPU tolerances


# --------------------------------------------------------------------------- the table
def test_table_covers_what_it_says():
    parts = {n: sc.check_geometry(c)[1] for n, c in sc.CASES.items()}
    assert {c.kind for c in sc.CASES.values()} == {"rbf", "matern32", "matern52"}
    assert any(b == a for p in parts.values() for a, b in p), "an empty shard"
    assert any(b - a == 1 for p in parts.values() for a, b in p), "a one-row shard"
    assert any(a % 2 == 1 and b > a for p in parts.values() for a, b in p), "an odd first row"
    assert any(a % 4 != 0 and b > a for n, p in parts.items() if sc.CASES[n].fp32 for a, b in p), "a first row that is no multiple of 4, in fp32"
    assert any(c.M % 4 != 0 for c in sc.CASES.values()) and any(c.M > 64 for c in sc.CASES.values())
    assert any(sc.gemv_u_split(sc.CASES[n].M, b - a)[0] > 1 for n, p in parts.items() for a, b in p), "nsplit > 1"
    assert all(not sc.CASES[n].full for n in sc.CASES if sc.CASES[n].N > 4000), "nothing N x N for the large case"
    for world, per, n in sc.SEG_SHAPES:
        assert row_partition(n, world)[0] == per


def test_large_case_builds_nothing_n_by_n():
    case = sc.CASES["P6"]
    with sc.emulated_world(case, gpu=False) as w:
        w.setup(hip=False)
        sc.run_precond(w, sc.rand(1, case.N))
        assert all(o._Kloc is None and o._Kfull is None for o in w.oracle)


# --------------------------------------------------------------------------- the reference agrees with itself
@pytest.mark.parametrize("name", sc.FULL)
def test_oracle_ops_summed_over_ranks_equal_the_whole_problem(name):
    case = sc.CASES[name]
    with sc.emulated_world(case, gpu=False) as w:
        w.setup(hip=False)
        v = sc.rand_v(case)
        row = sc.run_objective(w, v, hip=False, cyclic=False)
        cyc = sc.run_objective(w, v, hip=False, cyclic=True, Kv_locals=row["Kv"])
        ref = sc.reference_objective(w, v)
        g = sc.pack_grad(ref.grad)
        for label, out in (("row", row), ("cyclic", cyc)):
            for got, want, what in zip(out["fin"][0], (ref.bound, ref.lower, ref.upper, ref.logdet), ("bound", "lower", "upper", "logdet")):
                print(f"{name} {label} {what}: rel {abs(got - want) / abs(want):.3g}")
                assert abs(got - want) <= SELF_TOL * abs(want), (label, what)
            assert all(f == out["fin"][0] for f in out["fin"])
            err = np.abs(out["grad_sum"] - g).max() / np.abs(g).max()
            print(f"{name} {label} packed gradient: {err:.3g} of its largest entry")
            assert err <= SELF_TOL
        r = sc.rand(2, case.N)
        _, _, zs, rzs = sc.run_precond(w, r)
        terms = orc.common_terms(case.kind, w.X, w.hyp)
        z, rz = orc.nystrom_precond(terms.A, terms.LB, w.hyp.noise, r)
        assert np.abs(np.concatenate(zs) - z).max() <= SELF_TOL * np.abs(z).max()
        assert abs(sum(rzs) - rz) <= SELF_TOL * abs(rz)
        total = sum(sc.cyclic_partials(w, r))
        ref_mv = orc.dense_cov(case.kind, w.X, w.hyp) @ r
        assert np.abs(total - ref_mv).max() <= SELF_TOL * np.abs(ref_mv).max()


# --------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("name", list(sc.CASES))
def test_defect_last_row_left_out_of_u(name):
    case = sc.CASES[name]
    with sc.emulated_world(case, gpu=False) as w:
        w.setup(hip=False)
        r = sc.rand(3, case.N)
        for o, (r0, r1) in zip(w.oracle, w.parts):
            if r1 == r0:
                continue
            ref = o.A @ r[r0:r1]
            moved = sc.worst(sc.defect_u_drops_last_row(o, r[r0:r1]) - ref, sc.tol_u(o.A, r[r0:r1]))
            assert moved >= TEETH, (name, r0, moved)


@pytest.mark.parametrize("world,per,n", sc.SEG_SHAPES)
def test_defect_partial_read_from_the_wrong_element(world, per, n):
    z, partials = sc.rand(4, n), np.abs(sc.rand(5, world)) + 0.5
    buf = sc.seg_layout(world, per, n, z, partials)
    ref = sc.seg_sum(partials)
    assert ref == sc.seg_sum(buf.reshape(world, per + 1)[:, per])
    bad = sc.defect_partial_from_wrong_element(buf, world, per)
    assert abs(bad - ref) >= TEETH * sc.TOL_RZ * abs(ref)      # the GPU test asks for bitwise equality; the scalar's own bound is TOL_RZ


@pytest.mark.parametrize("name", [n for n in sc.FULL if sc.CASES[n].world > 1])
def test_defects_of_placement(name):
    """Replicated gradient terms on every rank; the noise term on rank 1."""
    case = sc.CASES[name]
    with sc.emulated_world(case, gpu=False) as w:
        w.setup(hip=False)
        v = sc.rand_v(case)
        ref = sc.run_objective(w, v, hip=False, cyclic=False)
        tol = sc.tol_grad(ref["grad_sum"], ref["fin"][0][0], case.D)
        bad = sc.defect_replicated_on_every_rank(w, ref, v)
        assert sc.worst(sum(bad) - ref["grad_sum"], tol) >= TEETH
        for g, (r0, r1) in enumerate(w.parts):
            if r0 != 0:   # the per-rank check: noise and mean entries of such a partial are zero within the tolerance
                assert np.all(ref["grad"][g][case.D + 1:case.D + 3] == 0.0)
                assert sc.worst(bad[g][case.D + 1:case.D + 3], tol[case.D + 1:case.D + 3]) >= TEETH, (name, g)
        p = sc.rand(6, case.N)
        parts = sc.cyclic_partials(w, p)
        moved = sc.defect_noise_on_rank1(parts, p, w.hyp.noise)
        tol_mv = gc.ATOL64 * np.abs(sum(parts)).max()
        for g in (0, 1):
            assert sc.worst(moved[g] - parts[g], tol_mv) >= TEETH, (name, g)


@pytest.mark.parametrize("name", [n for n in sc.FULL if sc.CASES[n].kind == "matern52"])
def test_defect_matern32_for_kind_2(name):
    case = sc.CASES[name]
    outs = []
    for kw in ({}, dict(profile=m52.k32, grad_factor=m52.h32)):
        with sc.emulated_world(case, gpu=False, **kw) as w:
            w.setup(hip=False)
            v = sc.rand_v(case)
            row = sc.run_objective(w, v, hip=False, cyclic=False)
            outs.append((row, sc.run_objective(w, v, hip=False, cyclic=True, Kv_locals=row["Kv"])))
    for good, bad in zip(outs[0], outs[1]):
        tol = sc.tol_grad(good["grad_sum"], good["fin"][0][0], case.D)
        assert sc.worst(bad["grad_sum"] - good["grad_sum"], tol) >= TEETH                     # the rank sums
        assert abs(bad["fin"][0][0] - good["fin"][0][0]) >= TEETH * sc.TOL_VALUE * abs(good["fin"][0][0])
        for g, (r0, r1) in enumerate(w.parts):
            if r1 > r0:                                                                       # and every rank's own partial
                assert sc.worst(bad["grad"][g] - good["grad"][g], tol) >= TEETH, (name, g)
    # the profile alone (grad factor right) is seen by the bound, the grad factor alone by phase 3
    with sc.emulated_world(case, gpu=False, grad_factor=m52.h32) as w:
        w.setup(hip=False)
        only_h = sc.run_objective(w, sc.rand_v(case), hip=False, cyclic=False)
    good = outs[0][0]
    assert only_h["fin"][0] == good["fin"][0]
    assert sc.worst(only_h["grad_sum"] - good["grad_sum"], sc.tol_grad(good["grad_sum"], good["fin"][0][0], case.D)) >= TEETH


# --------------------------------------------------------------------------- vector references
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_vector_references(dtype):
    n = 4099
    a, b, c = sc.rand(7, n), sc.rand(8, n), sc.rand(9, n)     # float32-representable: a * b is exact in double
    assert sc.ref_dot(a, b) == pytest.approx(math.fsum(a * b), rel=0, abs=2.0 ** -60 * float(np.abs(a * b).sum()))
    T = sc.np_dtype(dtype)
    eps = np.finfo(T).eps
    rz, pap = 1.7, 0.3
    f = sc.ref_factor(rz, pap, dtype)
    assert float(f) == float(T(rz / pap))
    got = sc.ref_fma(f, a, b, dtype)
    # a double evaluation: exact product for a float factor (fp32), one more rounding of the product for a double factor (fp64)
    plain = float(f) * a + b
    assert np.all(np.abs(got - plain) <= (0.5 * eps * np.abs(plain) if dtype == "fp32" else eps * (np.abs(float(f) * a) + np.abs(b))) * (1 + 1e-9))
    assert dtype == "fp64" or np.array_equal(got, plain.astype(T).astype(np.float64))   # fp32: `plain` is exact up to 2^-53, far below half a float ulp
    assert np.array_equal(got, got.astype(T).astype(np.float64))
    vv, rr, g = sc.ref_update_v_r(a, b, c, a, rz, pap, True, dtype)
    assert np.array_equal(vv, sc.ref_fma(f, c, a, dtype)) and np.array_equal(rr, sc.ref_fma(-f, a, b, dtype)) and g == float(f)
    assert np.array_equal(sc.ref_residual(a, b, dtype), (a.astype(np.longdouble) - b.astype(np.longdouble)).astype(T).astype(np.float64))
    # the zero-denominator contract of the reference itself
    v0, r0, g0 = sc.ref_update_v_r(a, b, c, a, rz, 0.0, True, dtype)
    assert g0 == 0.0 and np.array_equal(v0, a) and np.array_equal(r0, b)
    p0, b0 = sc.ref_update_p(a, b, rz, 0.0, False, dtype)
    assert b0 == 0.0 and np.array_equal(p0, b)
    assert np.isnan(sc.ref_update_p(a, b, float("nan"), 1.0, False, dtype)[0]).all()
    assert np.isnan(sc.ref_update_v_r(a, b, c, a, 1.0, float("nan"), True, dtype)[0]).all()


def test_oracle_ops_carry_the_zero_denominator_rule():
    case = sc.CASES["P3"]
    with sc.emulated_world(case, gpu=False) as w:
        o = w.oracle[0]
        n = 5
        one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        v, r, p, Ap = (torch.from_numpy(sc.rand(k, n)) for k in range(4))
        v0, r0 = v.clone(), r.clone()
        o.update_v_r(v, r, p, Ap, one, zero, True)
        assert torch.equal(v, v0) and torch.equal(r, r0)
        z = torch.from_numpy(sc.rand(9, n))
        o.update_p(p, z, one, zero, False)
        assert torch.equal(p, z)
        buf = torch.from_numpy(sc.seg_layout(4, 2, 5, sc.rand(10, 5), [1.0, 2.0, 3.0, 0.0], fill=0.0))
        nrz = torch.zeros(1, dtype=torch.float64)
        p = torch.from_numpy(sc.rand(11, n))
        o.vec_update_p_seg(5, 2, 4, p, buf, nrz, zero, False)
        assert float(nrz[0]) == 6.0 and np.array_equal(p.numpy(), buf.numpy().reshape(4, 3)[:, :2].reshape(-1)[:5])
