"""The selection cases on the CPU (tests/select_cases.py): the follower and the restatement agree with the oracle's greedy rule, the stored
round-off constants bracket their measurements, every case that claims the single-candidate condition meets it, and every planted defect
is rejected.  No GPU."""
import numpy as np
import pytest

import select_cases as sc
from oracle import cglb_oracle as orc

FP64_GENERIC = [i for i in sc.INSTANCES if i.case.startswith("G") and i.dtype == "f64"]
CLAIM_SINGLE = [i for i in sc.INSTANCES if not sc.CASES[i.case].exhaust and i.case[0] in "GWE"]
_measured = {}


def measured(inst):
    """(problem, E_ref, KV32, restatement, follower on its path): computed once per instance, shared and left unchanged."""
    if inst not in _measured:
        p = sc.problem(inst)
        sc.check_geometry(inst, p)
        _measured[inst] = (p,) + sc.measure(inst, p)
    return _measured[inst]


def _ids(insts):
    return [i.id for i in insts]


def test_table_shape():
    assert all(c.N <= 3001 and min(c.M, c.N) <= 300 for c in sc.CASES.values())
    assert sum(c.exhaust for c in sc.CASES.values()) <= 3
    generic = [c for n, c in sc.CASES.items() if n.startswith("G") and not c.sqrt_d]
    scaled = [c for n, c in sc.CASES.items() if n.startswith("G") and c.sqrt_d]
    assert {(c.D, c.N, c.M, c.jitter) for c in scaled} <= {(c.D, c.N, c.M, c.jitter) for c in generic}    # the same shapes, other lengthscales
    assert sorted(c.D for c in generic) == [3, 5, 9, 17, 27, 32] and sorted(c.N for c in generic) == [255, 256, 257, 513, 1000, 2999]
    assert sorted(c.M for c in generic) == [7, 8, 9, 16, 17, 64] and {c.jitter for c in generic} == {1e-12, 1e-6}
    for D in (3, 5, 9, 17, 27, 32):     # per width, not over the union: every kind in both types is selected on
        have = {(i.kind, i.dtype) for i in sc.INSTANCES if i.case.startswith("G") and sc.CASES[i.case].D == D}
        assert have == {(k, t) for k in sc.KINDS for t in ("f64", "f32")}, D
    assert {sc.CASES[i.case].D for i in sc.INSTANCES if i.case.startswith("W")} == {33, 40, 100}
    assert {i.dtype for i in sc.INSTANCES if i.case.startswith("W")} == {"f64", "f32"}
    assert len(set(sc.INSTANCES)) == len(sc.INSTANCES) and {i.case for i in sc.INSTANCES} == set(sc.CASES)


@pytest.mark.parametrize("inst", FP64_GENERIC, ids=_ids(FP64_GENERIC))
def test_follower_and_restatement_agree_with_the_oracle(inst):
    """On the oracle's own greedy path the follower has zero regret at every step, and the float64 restatement makes the oracle's picks."""
    p, _, _, r, _ = measured(inst)
    Zref = orc.greedy_conditional_variance(p.X, p.M, sc.kernel_fn(inst.kind, p.ls, p.var), jitter=p.jitter)
    picks = np.array([int(np.flatnonzero((p.X == z).all(axis=1))[0]) for z in Zref])
    f = sc.follow(p.X, inst.kind, p.ls, p.var, p.jitter, picks)
    assert f.regret.max() == 0.0
    np.testing.assert_array_equal(r.picks, picks)


@pytest.mark.parametrize("inst", sc.INSTANCES, ids=_ids(sc.INSTANCES))
def test_stored_constants_bracket_the_measurement(inst):
    _, e_ref, kv, _, _ = measured(inst)
    print(f"{inst.id}: E_ref measured {e_ref:.3g} stored {sc.E_REF[inst]:.3g} (x {sc.HEADROOM}); KV32 measured {kv} stored {sc.KV32[inst]}")
    assert e_ref <= sc.E_REF[inst] <= 2.0 * e_ref
    if inst.dtype == "f32":
        assert kv <= sc.KV32[inst] <= 2.0 * kv
    else:
        assert sc.KV32[inst] is None


@pytest.mark.parametrize("inst", sc.INSTANCES, ids=_ids(sc.INSTANCES))
def test_restatement_passes_its_own_checks(inst):
    """The clean restatement is inside every bound a GPU result is held to (regret, trace, uniqueness, the exact properties)."""
    p, _, _, r, _ = measured(inst)
    v = sc.judge(inst, p, r.picks, r.trace)
    assert v.worst_regret <= 1.0 and v.trace_err <= 1.0 and v.unique_ok
    assert sc.exact_violations(p, r.picks, r.trace) == []
    assert np.isfinite(r.d_hist).all() and ((0 <= r.picks) & (r.picks < p.N)).all()


@pytest.mark.parametrize("inst", CLAIM_SINGLE, ids=_ids(CLAIM_SINGLE))
def test_single_admissible_candidate(inst):
    p, _, _, r, f = measured(inst)
    share = sc.single_share(f, sc.tol(inst, p.var))
    print(f"{inst.id}: {share:.3f} of the steps after the first have one admissible candidate")
    assert share >= sc.MIN_SINGLE


def test_edge_cases_visit_every_planted_row_out_of_row_order():
    for inst in (i for i in sc.INSTANCES if i.case.startswith("E1")):
        p, _, _, r, _ = measured(inst)
        order = [int(j) for j in r.picks if int(j) in p.planted]
        assert sorted(order) == sorted(p.planted), inst.id
        assert order != sorted(order), inst.id


def test_ties_inside_a_wave_are_on_the_path():
    """T1: at least three picks are made while an identical row of the same wave is still unpicked, beside the ties across waves and blocks."""
    for inst in (i for i in sc.INSTANCES if i.case == "T1"):
        p, _, _, r, _ = measured(inst)
        assert len(sc.intra_wave_tie_steps(p, r.picks)) >= 3, inst.id


@pytest.mark.parametrize("ident", ["J1-6-rbf-f64", "G2-matern32-f64", "G4s-matern52-f64", "I1a-rbf-f64"])
def test_follower_trace_equals_the_closed_form(ident):
    """The follower runs the recurrence; the closed form N (variance + jitter) - tr(K_fu K_uu^-1 K_uf) is a float64 solve.  At jitter 1e-6
    cond(K_uu) <= variance M / jitter = 3e7 at most, so the solve is good to ~1e-9 relative of the removed part; 1e-8 N variance is asserted."""
    inst = sc.by_id(ident)
    p, _, _, r, f = measured(inst)
    assert p.jitter == 1e-6
    closed = sc.closed_form_trace(p, inst.kind, r.picks)
    print(f"{ident}: follower {f.trace!r} closed form {closed!r}")
    assert abs(f.trace - closed) <= 1e-8 * p.N * p.var


def test_jitter_enters_the_trace():
    """J1: the reference trace holds N jitter minus what the picks removed - the four jitters give four different traces in the right order."""
    tr = [measured(sc.by_id(f"J1-{s}-rbf-f64"))[4].trace for s in ("0", "12", "6", "2")]
    assert tr[0] < tr[1] < tr[2] < tr[3]
    p = measured(sc.by_id("J1-2-rbf-f64"))[0]
    assert tr[3] - tr[0] > (p.N - p.picks) * 1e-2      # each unpicked row keeps its own jitter, and a jittered pivot removes less
    assert (tr[2] - tr[0]) / p.N > 100.0 * sc.tol(sc.by_id("J1-6-rbf-f64"), p.var)   # ... far outside the trace bound: a lost jitter is seen


# --------------------------------------------------------------------------- the planted defects
# by how many tolerances (regret in tol, trace in N tol) a defect has to miss the check of at least one instance
TEETH = 10.0
# defect -> the instances it is tried on (those it can apply to; kept short, the whole matrix takes a minute)
TRIED = {
    "drop_tail": ["G3-rbf-f64", "G3-matern32-f32", "G1-rbf-f32"],
    "skip_last_block": ["E1b-rbf-f64", "E1a-matern32-f32"],
    "no_init_jitter": ["J1-2-rbf-f64", "J1-2-matern32-f32", "J1-6-rbf-f64"],
    "stale_ls": ["G2-rbf-f64", "G1-matern32-f32"],
    "m52_as_m32": ["G1-matern52-f64", "G1-matern52-f32", "W3-matern52-f64"],
    "pad_nonzero": ["G2-rbf-f64", "G2-matern32-f32"],
    "wide_stride": ["W1-rbf-f64", "W1-rbf-f32", "W3-matern52-f32"],
}


@pytest.mark.parametrize("defect", sorted(TRIED))
def test_defect_misses_by_ten_tolerances(defect):
    worst = 0.0
    with np.errstate(all="ignore"):
        for ident in TRIED[defect]:
            inst = sc.by_id(ident)
            p = measured(inst)[0]
            r = sc.restate(p, inst.kind, inst.np_dtype, defect)
            v = sc.judge(inst, p, r.picks, r.trace)
            miss = max(v.worst_regret, v.trace_err)
            print(f"{defect} on {ident}: regret {v.worst_regret:.3g} tol at step {v.worst_step}, trace {v.trace_err:.3g} N tol")
            assert miss >= TEETH, ident       # every instance listed for the defect, not only one
            worst = max(worst, miss)
    assert worst >= TEETH


def test_tie_defect_violates_the_exact_tie_assertion():
    for inst in (i for i in sc.INSTANCES if i.case == "T1"):
        p = measured(inst)[0]
        r = sc.restate(p, inst.kind, inst.np_dtype, "ties_high")
        assert r.picks[0] == p.N - 1
        assert len(sc.tie_rule_violations(p, r.picks)) >= 5, inst.id


# The two defects below stay inside the tolerances by construction: a pivot's own update leaves d_j - (col_j - dot_j)^2 / d_j, twice the
# difference of two round-off errors of d_j, and a missing clamp leaves values of -O(round-off); both are of the size of E_ref itself, which the
# tolerance exceeds fourfold.  Measured over every instance and on jitter-free exhaustion shapes (RBF, N = 300, D = 1 and 2, M = 200 and 300, both
# types): at most 0.48 N tol (no_clamp) and 0.006 N tol (pivot_not_zeroed) in the trace, no change of the regret.  They are held by what is exact instead.
EXACT_ONLY = {"no_clamp": "negative trace", "pivot_not_zeroed": "after all rows were picked"}
FULL_SELECTIONS = ["X1c-matern32-f64", "X1c-matern32-f32", "O1-matern32-f64", "O1-matern52-f32"]


@pytest.mark.parametrize("defect", sorted(EXACT_ONLY))
def test_benign_defect_violates_an_exact_property(defect):
    for ident in FULL_SELECTIONS:
        inst = sc.by_id(ident)
        p = measured(inst)[0]
        r = sc.restate(p, inst.kind, inst.np_dtype, defect)
        v = sc.judge(inst, p, r.picks, r.trace)
        print(f"{defect} on {ident}: regret {v.worst_regret:.3g} tol, trace {v.trace_err:.3g} N tol (trace {r.trace!r})")
        assert max(v.worst_regret, v.trace_err) < 1.0     # the reason it is listed here and not above
        assert any(EXACT_ONLY[defect] in msg for msg in sc.exact_violations(p, r.picks, r.trace)), ident


def test_every_defect_is_tried():
    assert set(TRIED) | set(EXACT_ONLY) | {"ties_high"} == set(sc.DEFECTS)
