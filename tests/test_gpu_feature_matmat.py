"""The random-feature product (cglb_feature_matmat, cglb_amd/csrc/kernels_feature_multi.hip) against the np.longdouble restatement
tests/sample_ref.py `features`, element by element.

Cells: the covering table `sample_ref.feature_cells` (40 cells): every D of (1, 3, 8, 17, 32, 40) - the padded widths 1, 3, 8, 20, 32 and the
looping instance - with the row counts 1, 255 and 256 R - 1, 256 R, 256 R + 1 of its rows per lane R; F on both sides of the edges between
one, two and three feature chunks, at the 256-slot cap and at small odd counts; S in (1, 3, 8, 9, 16, 17); two cells of the R = 2 instance
(D = 12); the training rows themselves (x NULL).  Exact cases: omega = b = 0 (every cosine is exactly 1: the sum of the weights to the
summation error alone), W = 0 (exactly 0), phases at eighths of a turn, an offset data set (columns at 10^3 +- 1) and new points at 10^3.
Outputs are pre-filled with NaN; a second call is bitwise equal.

Tolerance of one element (`sample_ref.feature_tolerance`, computed from the inputs; nothing in it is tuned to the device):
    sqrt(2 f / F) sum_j |W_sj| (eps_cos + (d + 3) u (sum_k |omega_jk (x_ik - c_k) / l_k| + |b_j|)) + (F / nsplit + nsplit + 2) u sqrt(2 f / F) sum_j |W_sj|
with eps_cos the bound devmath.h states for cos_turns (3e-16).  The operation count of the phase is the implementation's: 1 / (2 pi l_k)
rounded once on the host, its product with omega_jk, x_ik - c_k; 1 / 2 pi and its product with b_j; d fused multiply-adds: d + 3 roundings.
The worst error / tolerance per instance is printed (DESIGN.md section 4g records a run).
"""
import numpy as np
import pytest
import torch

import sample_ref as sr

pytestmark = pytest.mark.gpu


def _context(X, y, d):
    from cglb_amd.hip_context import HipContext
    h = sr.feature_hypers(d)
    ctx = HipContext(X, y, sr.K_PREC, "matern32", device=torch.device("cuda", 0))
    ctx.set_hypers(h["lengthscales"], h["variance"], h["noise"], h["mean"], X[:sr.K_PREC].copy(), 1e-6)
    return ctx, h


@pytest.mark.parametrize("cell", sr.feature_cells(), ids=lambda c: c[0])
def test_feature_product_matches_the_restatement(cell):
    _id, d, n, F, S, mode, training = cell
    X, y, x, omega, b, W = sr.feature_problem(cell)
    rows = X if x is None else x
    ctx, h = _context(X, y, d)
    try:
        out = torch.full((rows.shape[0], S), float("nan"), dtype=torch.float64, device=ctx.device)
        got = ctx.feature_matmat(x, omega, b, W, out=out).cpu().numpy()
        again = ctx.feature_matmat(x, omega, b, W, out=torch.full_like(out, float("nan"))).cpu().numpy()
        assert ctx.get_stat("feature_ms") > 0.0
    finally:
        ctx.close()
    c = sr.centre(X)
    want = sr.features(rows, c, h["lengthscales"], h["variance"], omega, b, W)
    tol = sr.feature_tolerance(rows, c, h["lengthscales"], h["variance"], omega, b, W)
    assert got.shape == (rows.shape[0], S) and np.all(np.isfinite(got))
    assert np.array_equal(got, again)
    err = np.asarray(np.abs(got.astype(np.longdouble) - want), dtype=np.float64)
    nsplit, chunk = sr.feature_split(rows.shape[0], F, d)
    print(f"{_id}: R = {sr.rows_per_lane(d)}, {nsplit} chunks of {chunk}: worst error {err.max():.2e}, worst error / tolerance "
          f"{(err / np.maximum(tol, 1e-300)).max():.3f}")
    if mode == "zero_w":
        assert np.all(got == 0.0)
    if mode == "zero_phase":   # every cosine is exactly 1: only the fixed-order sums are left of the tolerance
        amp = np.sqrt(2.0 * h["variance"] / F)
        sums = amp * W.astype(np.longdouble).sum(axis=1)
        summation = (F / nsplit + nsplit + 2) * sr.U * amp * np.abs(W).sum(axis=1)
        assert np.all(np.abs(got.astype(np.longdouble) - sums[None, :]) <= summation[None, :])
    assert np.all(err <= tol), (err / np.maximum(tol, 1e-300)).max()


def test_refusals_and_timing_entry():
    from cglb_amd import _lib
    from cglb_amd.hip_context import HipContext
    cell = sr.feature_cells()[0]
    X, y, x, omega, b, W = sr.feature_problem(cell)
    ctx, _h = _context(X, y, cell[1])
    try:
        assert ctx.time_feature_matmat(sr.N_TRAIN, 65, 9, 1) > 0.0
        with pytest.raises(ValueError, match="n_rows <= n_total"):
            ctx.time_feature_matmat(sr.N_TRAIN + 1, 65, 9, 1)
        om, ph, Wt = ctx._features(omega, b, W)
        out = torch.empty((5, Wt.shape[0]), dtype=torch.float64, device=ctx.device)
        rc = ctx.lib.cglb_feature_matmat(ctx._ctx, None, 5, om.data_ptr(), ph.data_ptr(), Wt.data_ptr(), om.shape[0], Wt.shape[0], out.data_ptr())
        assert rc == _lib.ERR_BAD_ARG      # the training rows are all of them
        ctx.set_option("logdet_bound", 1)
        with pytest.raises(ValueError, match="logdet_bound 0"):
            ctx.feature_matmat(x, omega, b, W)
        ctx.set_option("logdet_bound", 0)
        assert np.all(np.isfinite(ctx.feature_matmat(x, omega, b, W).cpu().numpy()))   # the context is still usable
    finally:
        ctx.close()
    ctx32 = HipContext(X, y, sr.K_PREC, "rbf", dtype=torch.float32, device=torch.device("cuda", 0))
    try:
        ctx32.set_hypers(np.ones(cell[1]), 1.0, 0.1, 0.0, X[:sr.K_PREC].copy(), 1e-6)
        with pytest.raises(ValueError, match="fp64"):
            ctx32.feature_matmat(x, omega, b, W)
    finally:
        ctx32.close()
