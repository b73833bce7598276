"""The per-element kernel-value checks judged on the CPU (tests/kernel_value_cases.py): the point sets are what their rows claim, the
longdouble reference is certified, the float64 restatement of the device's arithmetic passes the tolerance on every element, every planted
defect fails it by a factor of ten or more - and the aggregate check the suite relied on so far sees two of them far more weakly or not at all."""
import numpy as np
import pytest

import kernel_value_cases as kv
from oracle import cglb_oracle as orc

CASES = kv.case_table()
IDS = [kv.case_id(c) for c in CASES]
ENTRIES = ("matvec_sym", "matvec_plain", "cross_matvec")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_point_sets_are_what_their_rows_claim(case):
    st = kv.check_set(case)   # N mod 16, all 256 table slots, >= 100 near-integer exponents per side, the range figure reached within 1 %
    clamp, bias = kv.regime(case.kind, *kv.build_set(case))
    assert clamp == case.clamp
    d = kv.regime_details(case.kind, *kv.build_set(case))
    if case.kind == "rbf":
        assert bias == 0.0 and d.int_ok
        assert (d.oct < 950.0) == (case.clamp == 0)
        assert abs(d.oct / case.target - 1.0) < 1e-6
        if case.name in ("B", "C"):
            assert 0.015 < abs(d.oct / 950.0 - 1.0) < 0.025
    else:
        cap = kv.bias_cap_s2(case.D)
        assert abs(d.s2 / case.target - 1.0) < 1e-6
        assert (bias <= kv.BIAS_MAX) == (case.clamp == 0)          # the Matern rows switch on the bias cap, far below oct = 950
        assert d.oct < 950.0 or case.name == "D"
        if case.name in ("B", "C"):
            assert 0.015 < abs(d.s2 / cap - 1.0) < 0.025
        if case.name.startswith("C'"):
            assert 0.015 < abs(d.s2 / kv.INT_BOUND_S2 - 1.0) < 0.025
            assert d.int_ok == (case.name == "C'-")
    if case.name == "D" or (case.name == "F77" and case.kind == "rbf"):
        assert st["max_oct"] > kv.FLOOR_OCT                        # values below the floor
    if case.name == "C":
        assert st["max_oct"] < kv.FLOOR_OCT                        # clamped, every value still above the floor


def _smallest_tolerance(case, g):
    """the tightest bound any configuration puts on a pair: EXACT level, fewest roundings"""
    clamp, bias = kv.regime(case.kind, *kv.build_set(case))
    p = kv.path_for("matvec_plain", case.kind, kv.EXACT, clamp)
    pg = kv.path_for("grad", case.kind, kv.EXACT, clamp)
    return np.minimum(kv.tolerance(case.kind, g, p).tol, kv.tolerance(case.kind, g, pg).tol), kv.tolerance(case.kind, g, pg, which="h").tol


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_longdouble_reference_is_certified_by_mpmath(case):
    X, ls = kv.build_set(case)
    g = kv.pair_geometry(case.kind, X, ls)
    tk, th = _smallest_tolerance(case, g)
    rng = np.random.default_rng(5)
    N = X.shape[0]
    n_pairs = 2000 if case.D <= 8 else 600    # D = 32: 50-digit sums of 32 terms per pair
    pairs = [tuple(rng.integers(0, N, 2)) for _ in range(n_pairs - 8)]
    far = np.argsort(-g.E.astype(np.float64), axis=None)[:8]   # the smallest values, where the exponent's rounding weighs most
    pairs += [tuple(np.unravel_index(q, g.E.shape)) for q in far]
    ek, eh = kv.certify(case.kind, X, X, ls, pairs, g.E, g.kap, g.h)
    i, j = np.array(pairs).T
    rel_k = (tk[i, j] / g.kap[i, j]).astype(np.float64)
    rel_h = (th[i, j] / g.h[i, j]).astype(np.float64)
    print(f"{kv.case_id(case)}: longdouble vs mpmath, kappa {ek.max():.2e}, h {eh.max():.2e}; smallest relative tolerance {rel_k.min():.2e}")
    assert np.all(ek <= rel_k / 10.0) and np.all(eh <= rel_h / 10.0)   # pair by pair: a tenth of the tightest bound any configuration uses


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("prec", [kv.EXACT, kv.FAST, kv.LOW])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_restatement_passes_on_every_element(case, prec, entry):
    """the inputs are fair: the same arithmetic in float64 NumPy, Gram form included, is inside the tolerance everywhere"""
    X, ls = kv.build_set(case)
    clamp, bias = kv.regime(case.kind, X, ls)
    if case.D > 32:   # wide inputs: the mid-width symmetric stream, the Gram tiles; the cross products of wide inputs are tiles
        entry = {"matvec_sym": "matvec_mid", "matvec_plain": "tiles", "cross_matvec": "tiles"}[entry] if case.D <= 96 else "tiles"
    p = kv.path_for(entry, case.kind, prec, clamp)
    rows = kv.new_points(case) if entry == "cross_matvec" else None
    g = kv.pair_geometry(case.kind, X, ls, rows)
    val = kv.emulate(case.kind, X, ls, p, bias, rows=rows)
    r = kv.ratios(val, g.kap, kv.tolerance(case.kind, g, p, bias))
    w = np.unravel_index(np.argmax(r), r.shape)
    print(f"{kv.case_id(case)} {entry} prec {prec}: worst error / tolerance {r.max():.3f} at pair {w}, E = {float(g.E[w]):.6f}")
    assert r.max() <= 1.0


def _defect_cases(defect):
    if defect == "m52_quadratic":
        return [c for c in CASES if c.kind == "matern52" and c.name in ("A", "E8")]
    return [c for c in CASES if c.name in ("A", "E8")]


@pytest.mark.parametrize("defect", kv.DEFECTS)
def test_every_planted_defect_moves_an_element_by_ten_tolerances(defect):
    for case in _defect_cases(defect):
        X, ls = kv.build_set(case)
        clamp, bias = kv.regime(case.kind, X, ls)
        p = kv.path_for("matvec_sym", case.kind, kv.FAST, clamp)
        g = kv.pair_geometry(case.kind, X, ls)
        b = kv.tolerance(case.kind, g, p, bias)
        good = kv.ratios(kv.emulate(case.kind, X, ls, p, bias), g.kap, b)
        bad = kv.ratios(kv.emulate(case.kind, X, ls, p, bias, defect=defect), g.kap, b)
        print(f"{defect} on {kv.case_id(case)}: worst error / tolerance {bad.max():.3g} ({int((bad > 1).sum())} of {bad.size} elements outside; clean {good.max():.3f})")
        assert good.max() <= 1.0
        assert bad.max() >= 10.0


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("N,D", [(333, 5), (700, 12), (600, 24), (520, 32)])
@pytest.mark.parametrize("defect", ["table_entry", "low_tail"])
def test_the_aggregate_check_against_the_per_element_check(defect, N, D, kind):
    """The statement of the gap, on shapes of tests/test_gpu_kff_variants.py::test_matvec_variants (seeded normal data, lengthscales
    0.6 + U(0, 1), random p, max |K p - ref| <= 2e-12 max |ref|).  Looked at one value at a time, a wrong table entry and a wrong polynomial
    on the ragged tail columns fail their tolerance tenfold on every shape.  What the aggregate makes of them, measured here:
      table entry off by 1e-11    3.7e-13 .. 2.5e-12 of max |ref| on the dense shapes, 2e-14 .. 2.2e-12 at D >= 24: it straddles the bound of
                                  2e-12 - six of the eight shapes pass, two fail by a quarter
      LOW polynomial on the tail  1.9e-11 .. 9.9e-11 on every shape: SEEN, through the diagonal elements of the tail columns (kappa_jj = 1 takes
                                  the polynomial's full error into (K p)_j).  The aggregate is not blind to this one, whatever the data.
    Asserted: in units of its own bound, the per-element check sees each defect at least ten times as strongly as the aggregate does (measured
    17 .. 2000 times), and the table entry never moves the aggregate by more than 1.5 bounds - no margin a test could rely on."""
    X, y, Z = orc.synthetic_problem(N, D, 8, seed=N + D)
    rng = np.random.default_rng(1)
    ls = 0.6 + rng.random(D)
    pvec = rng.standard_normal(N)
    clamp, bias = kv.regime(kind, X, ls)
    p = kv.path_for("matvec_sym", kind, kv.FAST, clamp)
    g = kv.pair_geometry(kind, X, ls)
    ref = (g.kap @ pvec.astype(kv.LD)).astype(np.float64)
    bad = kv.emulate(kind, X, ls, p, bias, defect=defect)
    agg = np.abs(bad @ pvec - ref).max() / np.abs(ref).max()
    r = kv.ratios(bad, g.kap, kv.tolerance(kind, g, p, bias))
    print(f"{defect} {kind} N {N} D {D} (clamp {clamp}): aggregate {agg:.2e} (bound 2e-12), per element {r.max():.3g} tolerances")
    assert r.max() >= 10.0
    assert r.max() >= 10.0 * (agg / 2e-12)
    if defect == "table_entry":
        assert agg <= 1.5 * 2e-12
