"""The multi-column cross product (cglb_cross_matmat, cglb_amd/csrc/kernels_cross_multi.hip) against a dense numpy product:
out[i, s] = f sum_j kappa(xnew_i, x_j) V[j, s].

The axes (tests/geometry_cases.py prunes its cells the same way: every value of every axis, the edges of a class crossed with the class, the
two- and three-valued axes rotated over the cells instead of crossed with them):
  * padded width D_p in 1, 3, 8 (4 rows per lane, B = 1024 new points per workgroup), 10 (2 rows, B = 512), 20, 32 (1 row, B = 256);
  * n_new in 1, 63, 65, 257 and B - 1, B, B + 1 of the width's class: 7 x 6 = 42 cells, every one its own case;
  * N in 1, 65, 1100; S in 1, 7, 8, 9, 17 (a short group, a full one, a full one and a single column, two and a single);
  * the three kernel kinds, the three precision levels, forced kff_jsplit in 0 (the rule), 1, 3, 7 and the two hyper-parameter sets: rotated
    over the cells with strides that are coprime to each other, so that every kind meets every precision level and every S meets every N.
New points: the first on training row 0, the second on the last training row, the last one at 10^3 in every coordinate, where every kernel
value underflows and the row is 0; the rest standard normal.  Every output is pre-filled with NaN.  (The range-clamped 2^x of the device
floors at 2^-1000, devmath.h CGLB_EXP_FLOOR_OCT, so "0" on the device is at most 2^-1000 = 9.3e-302 times the Matern polynomial per unit of |V|;
the largest polynomial here is 1 + s + s^2 / 3 at s = sqrt(5) 10^3 sqrt(32) (1 + 4 / 10^3), D = 32 at lengthscale 1: 5.4e7.  FLOOR below is
2^-1000 x 1e8.)

Tolerance: 1e-11 of sum_j |kappa V| per entry, what tests/test_gpu_grad_multi.py holds its sums to, at the precision levels 0 and 1 (kernel
values to 3e-16 and 1e-13).  Level 2 is the opt-in whose kernel values are a degree-2 table polynomial with a relative error of 1.03e-10
(devmath.h, CGLB_PREC_LOW): that error of the number format is added to the tolerance there, nothing else.
"""
import functools

import numpy as np
import pytest
import torch

import gpr_ref as ref
import matern52_ref as m52
from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu

KINDS = ["rbf", "matern32", "matern52"]
WIDTHS = {1: 1024, 3: 1024, 8: 1024, 10: 512, 20: 256, 32: 256}   # D (= D_p) -> new points per workgroup
N_VALUES = [1, 65, 1100]
S_VALUES = [1, 7, 8, 9, 17]
JSPLITS = [0, 1, 3, 7]
TOL = 1e-11
LEVEL2_KERNEL_ERROR = 1.03e-10
FLOOR = 2.0 ** -1000 * 1e8


def _cells():
    cells, x = [], 0
    for D, B in WIDTHS.items():
        for n_new in (1, 63, 65, 257, B - 1, B, B + 1):
            cells.append(dict(D=D, n_new=n_new, N=N_VALUES[x % 3], S=S_VALUES[(x // 3 + x) % 5], kind=KINDS[x % 3], prec=(x // 3) % 3,
                              jsplit=JSPLITS[(x // 2) % 4], trained=bool((x // 5) % 2)))
            x += 1
    return cells


CELLS = _cells()


def test_the_cells_cover_every_value_and_the_crossings_the_docstring_names():
    seen = lambda key: {c[key] for c in CELLS}
    assert seen("N") == set(N_VALUES) and seen("S") == set(S_VALUES) and seen("jsplit") == set(JSPLITS) and seen("trained") == {False, True}
    assert {(c["kind"], c["prec"]) for c in CELLS} == {(k, p) for k in KINDS for p in range(3)}
    assert {(c["S"], c["N"]) for c in CELLS} == {(s, n) for s in S_VALUES for n in N_VALUES}
    for D, B in WIDTHS.items():
        assert {c["n_new"] for c in CELLS if c["D"] == D} == {1, 63, 65, 257, B - 1, B, B + 1}


def _new_points(X, n_new, seed):
    Xn = np.random.default_rng(seed).standard_normal((n_new, X.shape[1]))
    Xn[0] = X[0]
    if n_new > 2:
        Xn[1] = X[-1]
    if n_new > 1:
        Xn[-1] = 1.0e3
    return Xn


@functools.lru_cache(maxsize=None)
def _case(D, n_new, N, S, kind, trained):
    """Inputs and the dense numpy product of a cell, computed once: (X, y, h, Xn, V, want, scale)."""
    X, y = ref.problem(N, D)
    h = ref.hypers(D, trained)
    Xn = _new_points(X, n_new, 7 * N + D + n_new)
    V = np.random.default_rng(N + S).standard_normal((N, S))
    with m52.oracle_with_matern52():
        Ksf = orc.kernel_from_sqdist(kind, orc.scaled_sqdist(Xn, X, np.asarray(h["lengthscales"], dtype=np.float64)), h["variance"])
    return X, y, h, Xn, V, Ksf @ V, np.abs(Ksf) @ np.abs(V)


def _context(X, y, kind, h, dtype=torch.float64):
    from cglb_amd.hip_context import HipContext
    ctx = HipContext(X, y, 1, kind, dtype=dtype, device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:1].copy(), 1e-6)
    return ctx


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "D%d_n%d_N%d_S%d_%s_p%d_j%d_%s" % (c["D"], c["n_new"], c["N"], c["S"], c["kind"], c["prec"], c["jsplit"],
                                                                                         "trained" if c["trained"] else "init"))
def test_matches_the_dense_product(cell):
    X, y, h, Xn, V, want, scale = _case(cell["D"], cell["n_new"], cell["N"], cell["S"], cell["kind"], cell["trained"])
    floor = FLOOR * h["variance"] * np.abs(V).sum(axis=0)
    ctx = _context(X, y, cell["kind"], h)
    try:
        ctx.set_option("precision", cell["prec"])
        ctx.set_option("kff_jsplit", cell["jsplit"])
        out = torch.full((cell["n_new"], cell["S"]), float("nan"), dtype=torch.float64, device=ctx.device)
        got = ctx.cross_matmat(Xn, V, out=out).cpu().numpy()
        again = ctx.cross_matmat(Xn, V, out=torch.full_like(out, float("nan"))).cpu().numpy()
    finally:
        ctx.close()
    tol = TOL + (LEVEL2_KERNEL_ERROR if cell["prec"] == 2 else 0.0)
    live = scale > 0
    err = np.abs(got - want)[live] / scale[live]
    print(f"{cell}: largest error {err.max() if err.size else 0.0:.2e} of sum |kappa V|, tolerance {tol:.2e}")
    assert got.shape == want.shape and np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol * scale + floor)
    if cell["n_new"] > 1:
        assert np.all(want[-1] == 0.0) and np.all(np.abs(got[-1]) <= floor)     # the point at 10^3: every kernel value underflows
    assert np.array_equal(got, again)                                    # two calls: bitwise equal


def test_more_new_points_than_one_launch_takes():
    """16384 new points go into one launch; one more starts a second one with its own slab geometry."""
    N, D, S = 65, 3, 9
    X, y = ref.problem(N, D)
    h = ref.hypers(D, True)
    Xn = _new_points(X, 16385, 3)
    V = np.random.default_rng(5).standard_normal((N, S))
    Ksf = orc.kernel_from_sqdist("matern32", orc.scaled_sqdist(Xn, X, np.asarray(h["lengthscales"], dtype=np.float64)), h["variance"])
    ctx = _context(X, y, "matern32", h)
    try:
        out = torch.full((16385, S), float("nan"), dtype=torch.float64, device=ctx.device)
        got = ctx.cross_matmat(Xn, V, out=out).cpu().numpy()
    finally:
        ctx.close()
    assert np.all(np.abs(got - Ksf @ V) <= TOL * (np.abs(Ksf) @ np.abs(V)) + FLOOR * h["variance"] * np.abs(V).sum(axis=0))


def test_refusals():
    from cglb_amd import _lib
    N, D = 65, 3
    X, y = ref.problem(N, D)
    h = ref.hypers(D, False)
    V = np.random.default_rng(1).standard_normal((N, 2))
    ctx = _context(X, y, "rbf", h, dtype=torch.float32)
    try:
        with pytest.raises(ValueError, match="fp64"):
            ctx.cross_matmat(X[:5], V)
    finally:
        ctx.close()
    Xw, yw = ref.problem(65, 40)
    ctx = _context(Xw, yw, "rbf", ref.hypers(40, True))
    try:
        with pytest.raises(ValueError, match="32 input dimensions"):
            ctx.cross_matmat(Xw[:5], V)
    finally:
        ctx.close()
    ctx = _context(X, y, "rbf", h)
    try:
        xn = torch.as_tensor(X[:5], device=ctx.device).contiguous()
        Vt = torch.as_tensor(V.T.copy(), device=ctx.device)
        out = torch.zeros((5, 2), dtype=torch.float64, device=ctx.device)
        for S in (0, -1):
            assert ctx.lib.cglb_cross_matmat(ctx._ctx, xn.data_ptr(), 5, Vt.data_ptr(), S, out.data_ptr()) == _lib.ERR_BAD_ARG
        assert np.all(np.isfinite(ctx.cross_matmat(X[:5], V).cpu().numpy()))     # the context is still usable
    finally:
        ctx.close()
