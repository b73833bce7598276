"""Launch geometry of the plain and the matrix-pipe pair kernels (kernels_kff.hip, kernels_kff_mfma.hip) and of the rectangular pair
kernel behind the implicit preconditioner, against the fp64 direct-difference oracle.

kff_pairs_range / mfma_launch: the slot count is `kff_jsplit` (0: the default rule) clamped to 512 and to ncols / 64 (ncols / 16 for the
matrix pipe), the column chunk is rounded up to even, the rows per thread are `kff_rows` cut down by the padded width.  The design: both
variants x D in {3, 12, 24} x every jsplit value in {0, 1, 3, 7, 512, 5000 (clamps)}, kff_rows and the kernel kind rotated over the
cells (x = variant + D index + jsplit index: rows = (1, 2, 4)[x % 3], kind = x % 2, so each D and each variant meets every value of
both), one ragged N per cell; fp32 runs the plain kernel only.  Bounds as in tests/test_gpu_sym_geometry.py."""
import numpy as np
import pytest
import torch

import fp32_error_model as em
import geometry_cases as gc
from oracle import cglb_oracle as orc

_ctx, _reference, _check, _matvec_dot = gc.make_ctx, gc.reference, gc.check, gc.matvec_dot

pytestmark = pytest.mark.gpu

JSPLITS = (0, 1, 3, 7, 512, 5000)
NS = (1037, 2333, 4099, 777, 3001, 1601)   # ragged against 16, 64, 256 and 1024
PLAIN = [(variant, "fp64", D, js, (1, 2, 4)[(variant + i + q) % 3], em.KINDS[(variant + i + q) % 2], NS[(i + q) % 6])
         for variant in (0, 1) for i, D in enumerate((3, 12, 24)) for q, js in enumerate(JSPLITS)]
PLAIN += [(0, "fp32", D, js, (4, 1, 2)[q % 3], em.KINDS[q % 2], NS[q]) for D in (3, 24) for q, js in enumerate(JSPLITS)]


@pytest.mark.parametrize("variant,dtype,D,jsplit,rows,kind,N", PLAIN, ids=[f"v{c[0]}-{c[1]}-D{c[2]}-j{c[3]}-r{c[4]}-{c[5]}-N{c[6]}" for c in PLAIN])
def test_plain_and_mfma_kernels_with_forced_split_and_rows(variant, dtype, D, jsplit, rows, kind, N):
    X, _, hyp, p = gc.problem(N, D, seed=1)
    ctx = _ctx(kind, dtype, X, hyp, dict(kff_variant=variant, kff_jsplit=jsplit, kff_rows=rows))
    out = ctx.matvec(torch.from_numpy(p)).double().cpu().numpy()
    # accumulation depth of the fp32 model: one column chunk of the split (the whole row for one slot)
    slots = min(jsplit, 512, (N + 63) // 64) if jsplit else min(512, (N + 63) // 64)
    ref, s, bound = _reference(kind, dtype, X, hyp, p, -(-N // max(slots, 1)))
    _check(out, ref, s, bound, f"variant {variant} {dtype} D={D} N={N} jsplit={jsplit} rows={rows}")
    out2, dot = _matvec_dot(ctx, p)
    assert np.array_equal(out2, out)
    pf = p.astype(np.float32).astype(np.float64) if dtype == "fp32" else p
    assert dot == pytest.approx(float(np.sum(pf * out2)), rel=1e-12)
    if variant == 1:  # the matrix pipe really ran: its Gram form (x~ . y~ through MFMA) rounds differently from the plain kernel's fma chain
        ctx.set_option("kff_variant", 0)
        assert not np.array_equal(ctx.matvec(torch.from_numpy(p)).cpu().numpy(), out), "kff_variant 1 gave the plain kernel's bits"
    ctx.close()


@pytest.mark.parametrize("r0,r1,jsplit", [(37, 2999, 7), (1500, 2999, 512), (1501, 1502, 3), (1504, 2000, 1), (1600, 2999, 0)])
def test_plain_and_mfma_kernels_on_row_shards(r0, r1, jsplit):
    """Row shards of N = 2999, D = 12, both variants on one context: variant 1 addresses its row fragments by 16-row blocks and falls
    back to the plain kernel when the shard's first row is not a multiple of 16 (37, 1500, 1501) - then it must give the plain kernel's
    bits; 1504 and 1600 are aligned and keep the matrix pipe - then the bits must differ (another Gram form), and both match the oracle."""
    N, D = 2999, 12
    X, _, hyp, p = gc.problem(N, D, seed=7)
    ctx = _ctx("rbf", "fp64", X, hyp, dict(kff_jsplit=jsplit), row_range=(r0, r1))
    ref, s, bound = _reference("rbf", "fp64", X, hyp, p, 0, r0, r1)
    out = {}
    for variant in (0, 1):
        ctx.set_option("kff_variant", variant)
        out[variant] = ctx.matvec(torch.from_numpy(p)).cpu().numpy()
        _check(out[variant], ref, s, bound, f"variant {variant} shard [{r0},{r1}) jsplit={jsplit}")
    assert np.array_equal(out[0], out[1]) == (r0 % 16 != 0), f"r0 = {r0}: variant 1 {'did not fall' if r0 % 16 else 'fell'} back to the plain kernel"
    ctx.close()


@pytest.mark.parametrize("kind", ["rbf", "matern32"])
@pytest.mark.parametrize("N,D,M", [(3001, 3, 24), (1000, 12, 24), (2999, 24, 100), (700, 8, 300)])
def test_implicit_preconditioner_slab_sums_against_the_oracle(kind, N, D, M):
    """precond_mode 1: K_uf r through kff_rect_generic with nchunk = min(4096 / nrb, N / 64) column slabs.  N = 3001 / 2999 give 47 slabs
    (kff_combine_wide_kernel, nchunk > 32), N = 1000 / 700 give 16 / 11 (kff_combine_kernel); K_fu s has M / 64 slabs at most.  Checked
    through cglb_precond_apply against the oracle's Nystrom preconditioner at the bound of the golden implicit-preconditioner test,
    on one context back and forth between the two modes (the option invalidates the common terms)."""
    from cglb_amd.hip_context import HipContext
    X, y, Z = orc.synthetic_problem(N, D, M, seed=N + D)
    hyp = orc.Hypers(0.6 * np.sqrt(D) * np.ones(D), 0.9, 0.2, 0.1, Z, 1e-6)
    rng = np.random.default_rng(4)
    r = rng.standard_normal(N)
    terms = orc.common_terms(kind, X, hyp)
    zr, rzr = orc.nystrom_precond(terms.A, terms.LB, hyp.noise, r)
    ctx = HipContext(X, y, M, kind)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
    got = {}
    for step, mode in enumerate((1, 0, 1, 0)):
        ctx.set_option("precond_mode", mode)
        ctx.setup()
        z, rz = ctx.precond(torch.from_numpy(r))
        z = z.cpu().numpy()
        np.testing.assert_allclose(z, zr, rtol=0, atol=1e-9 * np.abs(zr).max(), err_msg=f"precond_mode {mode} (step {step})")
        assert rz == pytest.approx(rzr, rel=1e-9)
        if mode in got:
            assert np.array_equal(got[mode], z), f"precond_mode {mode} differs after a round trip through the other mode"
        got[mode] = z
    ctx.close()
