"""Common terms (models.py:176-213) through every Cholesky and A A^T path of setup_local_impl / setup_finish_impl (cglb_api.hip):
chol_mode 0 (rocSOLVER potrf) and 1 (the blocked LDS Cholesky) at block-edge M, the lower-block-triangle split-K A A^T at every
aat_block shape across the 2048-column slab edge, and the second slab group (s0 > 0 in slab_reduce_sym_kernel)."""
import numpy as np
import pytest
import torch

from oracle import cglb_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 128, 129, 513])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_both_cholesky_modes_factorise_like_the_oracle(M, dtype):
    """Tolerances of test_ragged_inducing_counts_factorise_like_the_oracle (1e-9 / 2e-3 of the largest entry); both modes on ONE context,
    back and forth (chol_mode takes effect at the next cglb_setup), against the oracle and against each other."""
    from cglb_amd.hip_context import HipContext
    N, D = 700, 3
    X, y, Z = orc.synthetic_problem(N, D, M, seed=M)
    td = torch.float64 if dtype == "fp64" else torch.float32
    tol = 1e-9 if dtype == "fp64" else 2e-3
    hyp = orc.Hypers(np.array([0.9, 1.1, 1.4]), 1.2, 0.3, 0.1, Z, 1e-6 if dtype == "fp64" else 1e-4)
    terms = orc.common_terms("rbf", X, hyp)
    ctx = HipContext(X, y, M, "rbf", dtype=td)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
    got = {}
    for step, mode in enumerate((0, 1, 0, 1)):
        ctx.set_option("chol_mode", mode)
        ctx.setup()
        mats = {k: ctx.get_matrix(k).double().cpu().numpy() for k in ("L", "LB", "A")}
        assert np.all(np.triu(mats["L"], 1) == 0) and np.all(np.triu(mats["LB"], 1) == 0), f"chol_mode {mode}: upper triangle not zero"
        for k, ref in (("L", terms.L), ("LB", terms.LB), ("A", terms.A)):
            err = np.abs(mats[k] - ref).max() / np.abs(ref).max()
            print(f"M={M} {dtype} chol_mode {mode} {k}: {err:.3g} (bound {tol})")
            np.testing.assert_allclose(mats[k], ref, rtol=0, atol=tol * np.abs(ref).max(), err_msg=f"chol_mode {mode}: {k}")
        if mode in got:
            for k in mats:
                assert np.array_equal(got[mode][k], mats[k]), f"chol_mode {mode}: {k} differs after a round trip through the other mode"
        got[mode] = mats
    for k in ("L", "LB", "A"):
        np.testing.assert_allclose(got[0][k], got[1][k], rtol=0, atol=tol * np.abs(got[1][k]).max(), err_msg=f"modes disagree on {k}")
    ctx.close()


AAT = [(M, blk, (2047, 2048, 2049, 4100)[(i + q) % 4]) for i, M in enumerate((128, 192, 200, 256, 1536)) for q, blk in enumerate((0, 64, 128, 512))]


@pytest.mark.parametrize("M,aat_block,N", AAT)
def test_blocked_aat_at_every_block_shape_and_slab_edge(M, aat_block, N):
    """aat_block b computes only the lower block triangle when b divides M and M >= 2 b (M = 200: no b does, the full square; 192 =
    3 x 64, 1536 = 3 x 512 = 12 x 128 = 24 x 64: an odd number of blocks), N straddles the 2048-column slabs (one full slab, a one-column
    tail, two slabs and a 4-column tail); every M meets every block width, N rotates.

    Two assertions.  LB LB^T = I + A A^T with the library's own A, formed in fp64 on the host: isolates the A A^T and Cholesky paths from
    the conditioning of K_uu.  The bound is the textbook one, not a measured one: a dot product of length N and the Cholesky of an
    M x M matrix have backward errors (N + 1) u and (M + 1) u |LB||LB^T| (u = 2^-53), and |A||A^T|, |LB||LB^T| <= sqrt(B_ii B_jj) <=
    max diag B entry-wise (Cauchy-Schwarz), for the library and for the host reference alike: 2 (N + M + 2) u max diag B.
    And L, LB, A against the oracle's common terms at 1e-9 of the largest entry (D = 8 at lengthscale 1.5 sqrt(D / 3): K_uu well conditioned)."""
    from cglb_amd.hip_context import HipContext
    D = 8
    X, y, Z = orc.synthetic_problem(N, D, M, seed=M + N)
    hyp = orc.Hypers(np.full(D, 1.5 * np.sqrt(D / 3.0)), 1.2, 0.3, 0.1, Z, 1e-6)
    ctx = HipContext(X, y, M, "rbf")
    ctx.set_option("aat_block", aat_block)
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
    ctx.setup()
    A, LB, L = (ctx.get_matrix(k).cpu().numpy() for k in ("A", "LB", "L"))
    B = np.eye(M) + A @ A.T
    err = np.abs(LB @ LB.T - B).max()
    bound = 2.0 * (N + M + 2) * 2.0 ** -53 * B.diagonal().max()
    print(f"M={M} aat_block={aat_block} N={N}: |LB LB^T - (I + A A^T)| = {err:.3g} (bound {bound:.3g}), smallest |B_ij| below the diagonal blocks {np.abs(np.tril(B, -1)).min():.3g}")
    assert err <= bound
    assert np.all(np.triu(LB, 1) == 0)
    terms = orc.common_terms("rbf", X, hyp)
    for got, ref, k in ((L, terms.L, "L"), (A, terms.A, "A"), (LB, terms.LB, "LB")):
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9 * np.abs(ref).max(), err_msg=k)
    ctx.close()


def _gram_compensated(A, chunk=128):
    """A A^T in fp64 with torch, summed to within about one rounding of each entry: the contraction is cut into `chunk`-column pieces and
    the pieces are added with an error-free two-sum (Knuth) whose error terms are carried along.  What is left is the round-off inside a
    piece - a 128-term product sum of 1/145 of the entry, about 5 u of that - so about sqrt(145) * 5 u / 145 = 0.4 u of the entry
    (u = 2^-53).  One GEMM over all 18 500 columns is NOT good enough as a reference here: against 80-bit sums on the host of the entries
    that are largest or differ most (checked in the test below, on every run), torch's single product is off by 3.65e-15 max|B|, 24x the
    Cholesky residual the test measures with it.  The compensated sum is asserted to be within 4 u max|B| of those host sums: the
    rounding of the stored entry, of the added 1 and the ~0.4 u estimated above with room for its tail over 60 entries."""
    s = torch.zeros((A.shape[0], A.shape[0]), dtype=A.dtype, device=A.device)
    c = torch.zeros_like(s)
    for k in range(0, A.shape[1], chunk):
        x = A[:, k:k + chunk] @ A[:, k:k + chunk].T
        t = s + x
        z = t - s
        c += (s - (t - z)) + (x - z)
        s = t
    return s + c


def _multi_group_case():
    from cglb_amd.hip_context import HipContext
    N, D, M = 18_500, 8, 4096
    X, y, Z = orc.synthetic_problem(N, D, M, seed=5)
    hyp = orc.Hypers(np.full(D, 1.5 * np.sqrt(D / 3.0)), 1.2, 0.3, 0.1, Z, 1e-6)
    ctx = HipContext(X, y, M, "rbf")
    ctx.set_hypers(hyp.lengthscales, hyp.variance, hyp.noise, hyp.mean, Z, hyp.jitter)
    ctx.setup()
    A, LB = ctx.get_matrix("A"), ctx.get_matrix("LB")
    assert A.dtype == torch.float64 and A.shape == (M, N)
    B = _gram_compensated(A)
    B.diagonal().add_(1.0)
    B = 0.5 * (B + B.T)
    return ctx, N, M, A, LB, B


def _residual(L, B):
    return float((L @ L.T - B).abs().max()) / float(B.abs().max())


def test_second_slab_group_of_the_blocked_aat():
    """M = 4096, fp64, N = 18 500: 10 slabs of 2048 columns in groups of 8 (1 GB of scratch per group), so slab_reduce_sym_kernel adds a
    second group onto the first (s0 > 0) - with the default aat_block 512, 8 x 8 blocks of which the lower 36 are computed.  No CPU
    oracle at this size: B = I + A A^T is formed on the device in fp64 with torch from the library's A and compared with LB LB^T.
    The tolerance is measured, not guessed: the residual |L^ L^^T - B|max / |B|max of torch.linalg.cholesky on the SAME B is the
    reference's own error, and the library gets 10x that (another blocking and summation order of A A^T and of the factorisation).

    B is summed with compensation (_gram_compensated): with B = A @ A.T in one GEMM the same check reads 3.57e-15 for the
    library against torch.linalg.cholesky's 1.52e-16 - and the whole gap is the error of that one GEMM, which the reference
    factor, computed FROM the erroneous B, does not see, while the library's factor of its own, more accurate sum does (the library's LB
    against its own I + A A^T: 1.52e-16).  A reference has to be more accurate than the tolerance it serves; the rule - 10x the residual
    of torch.linalg.cholesky on the same B - is unchanged.
    Measured on an MI355X with the compensated B: torch.linalg.cholesky 1.52e-16, the library 4.56e-16 (bound 1.52e-15);
    the single-GEMM B differs from the compensated one by 3.65e-15 max|B|."""
    ctx, N, M, A, LB, B = _multi_group_case()
    res_ref = _residual(torch.linalg.cholesky(B), B)
    res_lib = _residual(LB, B)
    one = A @ A.T
    one.diagonal().add_(1.0)
    gemm = float((one - B).abs().max()) / float(B.abs().max())
    # the reference against 80-bit sums on the host, on the 30 largest entries and the 30 on which the two torch sums differ most
    bmax = float(B.abs().max())
    idx = torch.cat([torch.topk((one - B).abs().flatten(), 30).indices, torch.topk(B.abs().flatten(), 30).indices]).cpu().numpy()
    rows = np.unique(np.concatenate([idx // M, idx % M]))
    Ah = dict(zip(rows.tolist(), A[torch.from_numpy(rows).to(A.device)].cpu().numpy().astype(np.longdouble)))
    e_comp = e_gemm = 0.0
    for f in idx.tolist():
        i, j = divmod(f, M)
        exact = float(np.sum(Ah[i] * Ah[j]) + (1.0 if i == j else 0.0))
        e_comp = max(e_comp, abs(float(B[i, j]) - exact) / bmax)
        e_gemm = max(e_gemm, abs(float(one[i, j]) - exact) / bmax)
    print(f"against 80-bit host sums (60 entries): compensated B {e_comp:.3g}, single-GEMM B {e_gemm:.3g} of max|B|")
    assert e_comp <= 4.0 * 2.0 ** -53, "the reference itself is off by more than the few roundings its construction allows"
    print(f"multi-group A A^T: residual of torch.linalg.cholesky {res_ref:.3g}, of the library {res_lib:.3g} (bound {10 * res_ref:.3g}); "
          f"single-GEMM B against the compensated one {gemm:.3g}")
    assert float(torch.triu(LB, 1).abs().max()) == 0.0
    ctx.close()
    assert res_lib <= 10.0 * res_ref


def test_second_slab_group_cholesky_and_slab_sums_separately():
    """The same case, its two halves apart.  (a) The factorisation: LB against the library's OWN I + A A^T gets 10x the residual of
    torch.linalg.cholesky on that same matrix (measured: both 1.52e-16).  (b) The slab sums of both groups: every entry of the library's
    A A^T and of the reference's is a sum of N products of which each carries at most (N + 1) u |a_i|.|a_j| <= (N + 1) u sqrt(B_ii B_jj) of
    round-off in any order (u = 2^-53; Higham, Accuracy and Stability, section 3.1), so the two differ by at most 2 (N + 1) u max diag B
    = 4.1e-12 max|B| - a bound from the accumulation depth, nothing measured in it (measured: 3.04e-16; a lost or doubled slab of the
    second group moves the diagonal by ~1/10 of itself).  The library's A A^T must be exactly symmetric (lower triangle mirrored)."""
    ctx, N, M, A, LB, B = _multi_group_case()
    Bl = ctx.aat_tensor().reshape(M, M).clone()
    assert torch.equal(Bl, Bl.T)
    Bl.diagonal().add_(1.0)
    bmax = float(B.abs().max())
    res_ref = _residual(torch.linalg.cholesky(Bl), Bl)
    res_lib = _residual(LB, Bl)
    diff = float((Bl - B).abs().max()) / bmax
    bound = 2.0 * (N + 1) * 2.0 ** -53 * float(B.diagonal().max()) / bmax
    print(f"multi-group: LB on the library's own B {res_lib:.3g} (torch's factor of it {res_ref:.3g}); |A A^T lib - compensated| {diff:.3g} (bound {bound:.3g})")
    assert res_lib <= 10.0 * res_ref
    assert diff <= bound
    ctx.close()
