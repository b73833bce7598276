"""The per-element kernel-value checks judged on the CPU (tests/kernel_value_cases.py): the point sets are what their rows claim, the
longdouble reference is certified, the float64 restatement of the device's arithmetic passes the tolerance on every element, every planted
defect fails it by a factor of ten or more - and the aggregate check the suite relied on so far sees two of them far more weakly or not at all.
The same for the direct form of the input-gradient products and the mid-width multi-pair gradient pass: value, h and every gradient entry of
the float64 restatement inside the bound, the sweep moved into every lane part a mid-width point is split over (`axis_variants`), and the
defects that only a unit-vector read-out in every column slot, pair slot, orientation and lane part can see."""
import numpy as np
import pytest

import kernel_value_cases as kv
from oracle import cglb_oracle as orc

CASES = kv.case_table()
IDS = [kv.case_id(c) for c in CASES]
MID = [c for c in CASES if 32 < c.D <= 96]
MID_ALL = [v for c in MID for v in [c] + kv.axis_variants(c)]          # what the mid-width GPU tests run on
DIRECT = [c for c in CASES if c.D <= 32] + MID_ALL                     # every set an input-gradient product is read out on
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
    if case.name == "C" or (case.name == "F64" and case.kind == "rbf"):
        assert st["max_oct"] < kv.FLOOR_OCT                        # clamped, every value still above the floor


@pytest.mark.parametrize("case", MID, ids=[kv.case_id(c) for c in MID])
def test_axis_variants_keep_the_regime_and_move_the_sweep(case):
    """The regime rule is a sum over coordinates and a minimum over lengthscales: moving the sweep (with its lengthscale) to another coordinate
    leaves exp_clamp and m32_bias where they were (the sets are fitted to the same range figure: equal to the 1e-6 of that fit), and every
    variant is a full set of its own.  The designed exponents then sit in the lane part of the sweep's coordinate: parts 0, 2 and 3 over the row
    and its two variants; at D = 40 and 77 the last part is partly zero padding."""
    X0, ls0 = kv.build_set(case)
    r0 = kv.regime_details(case.kind, X0, ls0)
    parts = {kv.lane_part(case, 0)}
    for v in kv.axis_variants(case):
        st = kv.check_set(v)
        X, ls = kv.build_set(v)
        r = kv.regime_details(v.kind, X, ls)
        assert np.array_equal(ls, ls0)
        assert r.exp_clamp == r0.exp_clamp and r.int_ok == r0.int_ok and st["exp_clamp"] == case.clamp
        assert r.m32_bias == pytest.approx(r0.m32_bias, rel=1e-6, abs=0.0) and r.s2 == pytest.approx(r0.s2, rel=1e-6)
        sweep = X[4:]
        assert np.all(sweep[:, np.arange(v.D) != v.axis] == 0.0) and np.all(sweep[1:, v.axis] != 0.0)
        parts.add(kv.lane_part(v, v.axis))
    assert parts == {0, 2, 3}
    assert kv.lane_part(case, case.D - 1) == 3 and (kv.hot_width(case.D) == case.D) == (case.D == 64)


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


def _all_levels_on_rows(cases):
    """the rows of the case table at the three levels, their axis variants (the same arithmetic on other lanes) at the default one"""
    return [pytest.param(c, prec, id=f"{kv.case_id(c)}-{prec}") for c in cases for prec in ((kv.EXACT, kv.FAST, kv.LOW) if c.axis == 0 else (kv.FAST,))]


@pytest.mark.parametrize("case,prec", _all_levels_on_rows(DIRECT))
def test_float64_restatement_of_the_direct_form_passes_on_every_element(case, prec):
    """cross_grad (and cross_grad_weighted: the same pair, the same counts) on narrow sets, cross_grad_mid on mid-width ones and their axis variants:
    value, h and EVERY gradient entry [282, 276, D] of the float64 restatement against the longdouble reference.  Where x*_ik == x_jk the entry is
    exactly zero; the elements under the floor are inside it with the right sign, and their number is capped (the cap the GPU test asserts)."""
    X, ls = kv.build_set(case)
    rows = kv.new_points(case)
    entry = "cross_grad_mid" if case.D > 32 else "cross_grad"
    p = kv.path_for(entry, case.kind, prec, case.clamp)
    if case.D <= 32:
        pw = kv.path_for("cross_grad_weighted", case.kind, prec, case.clamp)
        assert (pw.n_round, pw.n_round_h, pw.form, pw.clamp) == (p.n_round, p.n_round_h, p.form, p.clamp)
        assert kv.INPUT_GRAD_ROUNDINGS[pw.name] == kv.INPUT_GRAD_ROUNDINGS[p.name]
    assert p.clamp and not p.fold and not p.biased and p.form == "direct" and not p.hot_poly
    g = kv.set_geometry(case, cross=True)
    ops = kv.direct_operands(case.kind, X, ls, rows)
    bk, bh = kv.tolerance(case.kind, g, p), kv.tolerance(case.kind, g, p, which="h")
    N = X.shape[0]
    assert bk.floored[-1].all() and int(bk.floored[:-1].sum()) <= kv.floored_cap(case, N)      # only the row at 1e3 is under the floor by design
    live = ~bk.floored
    rk = kv.ratios(kv.emulate_direct(case.kind, X, ls, p, rows, "kappa", ops=ops), g.kap, bk)
    hv = kv.emulate_direct(case.kind, X, ls, p, rows, "h", ops=ops)
    rh = kv.ratios(hv, g.h, bh)
    rg, zeros = np.zeros(rk.shape), 0
    for k in range(case.D):
        r, same = kv.input_grad_ratios(case.kind, g, p, rows, X, ls, k, bh, kv.direct_grad_entry(case.kind, X, ls, p, rows, hv, k, ops))
        zeros += same
        rg = np.maximum(rg, r)
    print(f"{kv.case_id(case)} {entry} prec {prec}: worst error / tolerance kappa {rk[live].max():.3f} h {rh[live].max():.3f} gradient {rg[live].max():.3f}; "
          f"under the floor {int(bk.floored.sum())} pairs, largest value / floor {max(rk[~live].max(), rh[~live].max(), rg[~live].max()):.3f}; {zeros} exact zeros")
    assert rk.max() <= 1.0 and rh.max() <= 1.0 and rg.max() <= 1.0
    assert zeros >= (N - 3) ** 2 * (case.D - 1) + N + 2   # off-axis coordinates of centre and sweep; on the axis the diagonal and the duplicate row


@pytest.mark.parametrize("case,prec", _all_levels_on_rows(MID_ALL))
def test_float64_restatement_of_the_multi_pair_gradient_pass(case, prec):
    """grad_multi_mid: kappa and h of every pair through the Gram-form restatement on the path's own flags (clamp, fold, bias, Horner polynomial of the
    exponent's root), and the gradient entries of the probe pairs of the GPU test in the moment form, against `grad_tolerance(moments=True)`."""
    X, ls = kv.build_set(case)
    clamp, bias = kv.regime(case.kind, X, ls)
    p = kv.path_for("grad_multi_mid", case.kind, prec, clamp)
    assert p.form == "gram" and p.chain_extra == 5 and p.clamp == bool(clamp) and not p.hot_poly
    assert p.fold == (case.kind == "rbf" and not clamp) and p.biased == (case.kind != "rbf" and not clamp and prec != kv.EXACT)
    g = kv.set_geometry(case)
    kap = kv.emulate(case.kind, X, ls, p, bias)
    hv = kv.emulate(case.kind, X, ls, p, bias, which="h")
    rk = kv.ratios(kap, g.kap, kv.tolerance(case.kind, g, p, bias))
    rh = kv.ratios(hv, g.h, kv.tolerance(case.kind, g, p, bias, "h"))
    pairs = kv.probe_pairs_blocks(case)
    ref, bound = kv.grad_tolerance(case.kind, g, p, X, ls, pairs, 1.0, bias=bias, moments=True)
    i, j = pairs[:, 0], pairs[:, 1]
    dev = np.stack([kv.moment_grad_entry(case.kind, X, ls, hv, k)[i, j] for k in range(case.D)] + [kap[i, j]], axis=1)
    rg = kv.ratios(dev, ref, bound)
    print(f"{kv.case_id(case)} grad_multi_mid prec {prec}: worst error / tolerance kappa {rk.max():.3f} h {rh.max():.3f} probe entries {rg.max():.3f}")
    assert rk.max() <= 1.0 and rh.max() <= 1.0 and rg.max() <= 1.0


NEW_ROWS = [c for c in CASES if c.name in ("E12", "F64", "F90")]


@pytest.mark.parametrize("case", NEW_ROWS, ids=[kv.case_id(c) for c in NEW_ROWS])
def test_gradient_entry_reference_is_certified_by_mpmath(case):
    """-h delta_k / l_k of `input_grad_tolerance` against mpmath at 50 digits, on the sweep's coordinate and on three others, for pairs of every kind
    of row (kappa and h of these rows are certified with all the others above): a tenth of the tightest bound, pair by pair."""
    import mpmath as mp
    X, ls = kv.build_set(case)
    rows = kv.new_points(case)
    entry = "cross_grad_mid" if case.D > 32 else "cross_grad"
    p = kv.path_for(entry, case.kind, kv.EXACT, case.clamp)
    g = kv.pair_geometry(case.kind, X, ls, rows)
    bh = kv.tolerance(case.kind, g, p, which="h")
    rng = np.random.default_rng(11)
    pairs = [(int(a), int(b)) for a, b in zip(rng.integers(0, rows.shape[0] - 1, 150), rng.integers(0, X.shape[0], 150))]
    pairs += [(1, 2), (3, 1), (0, 275), (277, 1), (280, 2)]
    worst = 0.0
    for k in (case.axis, 1, case.D // 2, case.D - 1):
        ref, b, _ = kv.input_grad_tolerance(case.kind, g, p, rows, X, ls, k, bh)
        with mp.workdps(50):
            for a, c in pairs:
                q = mp.mpf(0)
                for d in range(case.D):
                    t = (mp.mpf(float(rows[a, d])) - mp.mpf(float(X[c, d]))) / mp.mpf(float(ls[d]))
                    q += t * t
                if case.kind == "rbf":
                    h = mp.exp(-q / 2)
                else:
                    sq = mp.sqrt((3 if case.kind == "matern32" else 5) * q)
                    h = 3 * mp.exp(-sq) if case.kind == "matern32" else mp.mpf(5) / 3 * (1 + sq) * mp.exp(-sq)
                lk = mp.mpf(float(ls[k]))
                want = -h * (mp.mpf(float(rows[a, k])) - mp.mpf(float(X[c, k]))) / lk / lk
                m, ex = np.frexp(ref[a, c])
                hi = float(m)
                have = (mp.mpf(hi) + mp.mpf(float(m - kv.LD(hi)))) * mp.mpf(2) ** int(ex)
                if want == 0:
                    assert have == 0
                    continue
                err = float(abs(have - want))
                assert b.floored[a, c] or err <= float(b.tol[a, c]) / 10.0
                if not b.floored[a, c]:
                    worst = max(worst, err / float(b.tol[a, c]))
    print(f"{kv.case_id(case)}: gradient-entry reference vs mpmath, worst error / tolerance {worst:.2e}")


def _direct_ratios(case, p, defect=None, part=0):
    """error / tolerance of value, h and gradient entries of the direct-form restatement on the read-out of the GPU test ([282, 276] per entry), and the
    mask of the designed pairs: centre and sweep against centre and sweep"""
    X, ls = kv.build_set(case)
    rows = kv.new_points(case)
    g = kv.pair_geometry(case.kind, X, ls, rows)
    bk, bh = kv.tolerance(case.kind, g, p), kv.tolerance(case.kind, g, p, which="h")
    hv = kv.emulate_direct(case.kind, X, ls, p, rows, "h", defect=defect, part=part)
    r = np.maximum(kv.ratios(kv.emulate_direct(case.kind, X, ls, p, rows, "kappa", defect=defect, part=part), g.kap, bk), kv.ratios(hv, g.h, bh))
    for k in sorted({case.axis, 0, case.D - 1}):
        r = np.maximum(r, kv.input_grad_ratios(case.kind, g, p, rows, X, ls, k, bh, kv.direct_grad_entry(case.kind, X, ls, p, rows, hv, k))[0])
    N = X.shape[0]
    designed = np.zeros(r.shape, dtype=bool)
    idx = np.r_[0, 4:N]
    designed[np.ix_(idx, idx)] = True
    return r, designed


@pytest.mark.parametrize("kind", kv.KINDS)
def test_a_dropped_lane_part_needs_the_axis_variants(kind):
    """part_dropped: d2 of cross_grad_mid_kernel misses the partial of one of the four lane parts.  On the row itself (sweep on coordinate 0) the parts
    1 - 3 hold distance for the corners and the off-set points alone: every one of the designed pairs - all table slots, the integer exponents from
    both sides - has an exact zero there and comes out bit for bit as without the defect, so nothing of the sweep is tested through those parts (the
    corners do see the defect: a handful of exponents).  The variant with its sweep in the part sees it at ten tolerances and more on the designed
    pairs themselves."""
    case = kv.find_case(kind, "F40")
    p = kv.path_for("cross_grad_mid", kind, kv.FAST, case.clamp)
    good, designed = _direct_ratios(case, p)
    assert good.max() <= 1.0
    by_part = {kv.lane_part(v, v.axis): v for v in [case] + kv.axis_variants(case)}
    for part in range(4):
        bad, _ = _direct_ratios(case, p, "part_dropped", part)
        on_row = bad[designed].max()
        if part == 0:
            assert on_row >= 10.0
        else:
            assert on_row < 10.0 and np.array_equal(bad[designed], good[designed])     # the axis-0 set alone: blind on its designed pairs
            assert bad[~designed].max() >= 10.0                                         # only the corners and off-set points differ
        line = f"part_dropped {part} on {kv.case_id(case)}: designed pairs {on_row:.3g} tolerances, corners and off-set points {bad[~designed].max():.3g}"
        if part in by_part and part != 0:
            v = by_part[part]
            vb, vd = _direct_ratios(v, p, "part_dropped", part)
            vg, _ = _direct_ratios(v, p)
            assert vg.max() <= 1.0 and vb[vd].max() >= 10.0
            line += f"; on {kv.case_id(v)} designed pairs {vb[vd].max():.3g} ({int((vb[vd] > 1).sum())} of {int(vd.sum())} outside)"
        print(line)


@pytest.mark.parametrize("kind", ["matern32", "matern52"])
@pytest.mark.parametrize("name", ["A", "E12", "F40"])
def test_the_gradient_polynomial_in_the_value_is_rejected(kind, name):
    """h_for_kappa: the value of kappa_hfac_hot_from_d2 takes h's polynomial (RBF: the two are the same number)"""
    case = kv.find_case(kind, name)
    X, ls = kv.build_set(case)
    rows = kv.new_points(case)
    p = kv.path_for("cross_grad_mid" if case.D > 32 else "cross_grad", kind, kv.FAST, case.clamp)
    g = kv.pair_geometry(kind, X, ls, rows)
    b = kv.tolerance(kind, g, p)
    good = kv.ratios(kv.emulate_direct(kind, X, ls, p, rows), g.kap, b)
    bad = kv.ratios(kv.emulate_direct(kind, X, ls, p, rows, defect="h_for_kappa"), g.kap, b)
    print(f"h_for_kappa on {kv.case_id(case)}: worst error / tolerance {bad.max():.3g} (clean {good.max():.3f})")
    assert good.max() <= 1.0 and bad[~b.floored].max() >= 10.0


@pytest.mark.parametrize("name", ["A", "E12", "E32", "F40", "F90"])
def test_swapped_columns_of_a_group_are_rejected(name):
    """column_swapped: columns b and b ^ 1 of a group exchange their weights.  With V the identity every column stands in every slot of the group of
    8 / 4 / 2 and the matrix comes back with its columns exchanged in pairs; any V whose neighbouring columns are equal returns the right answer."""
    for kind in kv.KINDS:
        case = kv.find_case(kind, name)
        X, ls = kv.build_set(case)
        rows = kv.new_points(case)
        entry = "cross_grad_mid" if case.D > 32 else "cross_grad"
        G = kv.group_width(entry, case.D)
        assert G == {"A": 8, "E12": 4, "E32": 2, "F40": 4, "F90": 2}[name]
        p = kv.path_for(entry, kind, kv.FAST, case.clamp)
        g = kv.pair_geometry(kind, X, ls, rows)
        b = kv.tolerance(kind, g, p)
        val = kv.emulate_direct(kind, X, ls, p, rows)
        good, bad = kv.ratios(val, g.kap, b), kv.ratios(kv.swap_columns(val, G), g.kap, b)
        print(f"column_swapped on {kv.case_id(case)} (groups of {G}): worst error / tolerance {bad[~b.floored].max():.3g} (clean {good.max():.3f})")
        assert good.max() <= 1.0 and bad[~b.floored].max() >= 10.0


@pytest.mark.parametrize("defect", ["orientation_dropped", "slot_crosstalk"])
@pytest.mark.parametrize("kind", kv.KINDS)
def test_defects_of_the_multi_pair_weight_are_rejected(kind, defect):
    """The read-out of test_grad_kff_multi_values_mid_width (probe pairs, slot q % S, both orientations, the alternating fillers) on the pair weight of
    kernels_grad_multi_mid.hip: clean, every probe returns the one value of its pair bit for bit; with the v_bi u_bj half lost, or u_b meeting v_{b+1}, at least one
    probe of every S >= 2 is off by ten tolerances and more.  orientation_dropped is invisible to probes with i and j in one row block or j right of i."""
    case = kv.find_case(kind, "F90")
    X, ls = kv.build_set(case)
    clamp, bias = kv.regime(kind, X, ls)
    p = kv.path_for("grad_multi_mid", kind, kv.FAST, clamp)
    g = kv.pair_geometry(kind, X, ls)
    kap = kv.emulate(kind, X, ls, p, bias)
    tol = kv.tolerance(kind, g, p, bias)
    pairs = kv.probe_pairs_blocks(case)
    N, brows = X.shape[0], kv.multi_block_rows(case.D)
    assert brows == 64 and kv.multi_block_rows(40) == 128
    for S in kv.MULTI_S[1:]:
        worst, seen_by = 0.0, set()
        for q, (i, j) in enumerate(pairs):
            for swap in (False, True):
                Um, Vm, slot = kv.multi_probe(N, S, q, i, j, swap)
                if kv.multi_single_slot(S, slot):
                    continue
                clean = kv.multi_pair_model(kap, Um, Vm, brows)
                assert clean in (kap[i, j], kap[j, i])      # the pair is visited once, from the row of the earlier block
                bad = kv.multi_pair_model(kap, Um, Vm, brows, defect)
                r = abs(bad - float(g.kap[i, j])) / float(tol.tol[i, j])
                if r >= 10.0:
                    seen_by.add((i // brows == j // brows, swap != (i > j)))
                worst = max(worst, r)
        print(f"{defect} on {kv.case_id(case)} S {S}: worst error / tolerance {worst:.3g}")
        assert worst >= 10.0
        if defect == "orientation_dropped":
            assert seen_by == {(False, True)}     # seen only across row blocks, and only by the orientation that puts V's point left of U's


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
