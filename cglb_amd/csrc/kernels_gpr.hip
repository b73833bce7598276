// Exact GP regression (model class "gpr": tensorflow/interface.py:200-206, gpflow GPR.log_marginal_likelihood; pytorch/interface.py:561-604), fp64.
//
//   K = f kappa(X, X) + s I = L L^T,  e = y - c,  alpha = K^-1 e,  lml = -1/2 e^T alpha - sum log L_ii - N/2 log 2 pi
//   d lml / d theta = 1/2 sum_ij W_ij dK_ij / d theta,  W = alpha alpha^T - K^-1;  d lml / d c = sum alpha
//
// The N x N matrix is stored once (lower triangle, column-major) and factored in place; a second N x N buffer holds K^-1 when a gradient is
// asked for.  Everything runs on the context stream in outer blocks of edge gpr_block (nb):
//   fill      gpr_fill_kernel writes the tiles J <= I of the lower triangle straight into the factor buffer (pair code of n2m_pair.h)
//   factor    right-looking: the diagonal block goes through the 64-column kernels of kernels_chol.hip (packed into a dense nb x nb buffer),
//             the block column below it through rocblas_dtrsm, the trailing lower triangle through rocblas_dsyrk (diagonal tiles) and
//             rocblas_dgemm (tiles below them): N^3 / 3 flops, all but N nb^2 / 3 of them in rocBLAS at depth nb
//   scalars   sum log L_ii by one block in fixed order, alpha by two rocblas_dtrsv, e^T alpha and sum alpha by the dot kernel of kernels_vec.hip
//   inverse   rocsolver_dpotri on a copy of L (lower); the strict upper triangle of that copy is never read
//   gradient  gpr_grad_kernel per tile I >= J: w_ij = alpha_i alpha_j - K^-1_ij read from the lower triangle (pairs below the diagonal count
//             twice), per-block partials of sum w h delta_d^2, sum w kappa and sum w_ii, added in fixed order by n2m_part_reduce_kernel
//   predict   K_f* in batches of 4096 new points: rocblas_dgemv with alpha, rocblas_dtrsm with L, a column squared-norm kernel
// Flops: N^3 / 3 (factor) + 2 N^3 / 3 (inverse); the pair evaluations are O(N^2 D) on the vector units, twice per gradient evaluation.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "n2m_pair.h"

namespace {

constexpr int64_t GPR_PREDICT_BATCH = 4096;

// L[i + j N] = f kappa(x_i, x_j) + s [i == j] for the pairs i >= j of the tile (rows i0 .. i0 + nI, columns j0 .. j0 + nJ; j0 <= i0, both
// multiples of 64): blocks above the diagonal leave at once, blocks on it write their lower triangle
template <int KIND>
__global__ __launch_bounds__(256) void gpr_fill_kernel(const double* __restrict__ Xn, int D, int64_t i0, int nI, int64_t j0, int nJ, double f,
                                                       double noise, double* __restrict__ L, int64_t N) {
    __shared__ double xi[NT][DC + 1], xj[NT][DC + 1];
    const int bi = blockIdx.x * NT, bj = blockIdx.y * NT;
    if (j0 + bj > i0 + bi) return;
    const int nIb = min(NT, nI - bi), nJb = min(NT, nJ - bj);
    double d2[4][4];
    n2m_d2(d2, xi, xj, Xn, D, i0 + bi, nIb, j0 + bj, nJb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = tx + 16 * p, j = ty + 16 * q;
            const int64_t gi = i0 + bi + i, gj = j0 + bj + j;
            if (i < nIb && j < nJb && gi >= gj) L[gi + gj * N] = n2m_kval<KIND>(d2[p][q], f) + (gi == gj ? noise : 0.0);
        }
}

// dst[i + j ldd] = src[i + j lds], n > i >= j (lower triangle of an n x n block; the strict upper triangle of neither side is touched)
__global__ __launch_bounds__(256) void gpr_tricopy_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i < n && i >= j) dst[(int64_t)i + (int64_t)j * ldd] = src[(int64_t)i + (int64_t)j * lds];
}

// out[0] = sum_i log L_ii (one block, fixed order)
__global__ __launch_bounds__(256) void gpr_sumlog_kernel(const double* __restrict__ L, int64_t N, double* __restrict__ out) {
    __shared__ double smem[16];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += blockDim.x) s += log(L[i * (N + 1)]);
    s = block_sum(s, smem);
    if (threadIdx.x == 0) out[0] = s;
}

// part[blk * (D + 2) + .] = sums over the block's pairs i >= j of m_ij w_ij {h_ij delta_ijd^2 (d < D), k_ij, [i == j]}, w_ij = alpha_i alpha_j -
// K^-1_ij, m_ij = 2 below the diagonal (the pair stands for (j, i) too) and 1 on it.  Entries above the diagonal are never read.
template <int KIND>
__global__ __launch_bounds__(256) void gpr_grad_kernel(const double* __restrict__ Xn, int D, int64_t i0, int nI, int64_t j0, int nJ, double f,
                                                       const double* __restrict__ alpha, const double* __restrict__ Kinv, int64_t N,
                                                       double* __restrict__ part) {
    __shared__ double xi[NT][DC + 1], xj[NT][DC + 1];
    __shared__ double smem[16];
    const int bi = blockIdx.x * NT, bj = blockIdx.y * NT;
    const int P = D + 2;
    double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * P;
    if (j0 + bj > i0 + bi) {  // a block above the diagonal of a diagonal tile: its pairs are counted by the mirrored block
        for (int t = threadIdx.x; t < P; t += blockDim.x) out[t] = 0.0;
        return;
    }
    const int nIb = min(NT, nI - bi), nJb = min(NT, nJ - bj);
    double wgt[4][4];
    n2m_d2(wgt, xi, xj, Xn, D, i0 + bi, nIb, j0 + bj, nJb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double ai[4], aj[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        ai[p] = tx + 16 * p < nIb ? alpha[i0 + bi + tx + 16 * p] : 0.0;
        aj[p] = ty + 16 * p < nJb ? alpha[j0 + bj + ty + 16 * p] : 0.0;
    }
    double sk = 0.0, st = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = tx + 16 * p, j = ty + 16 * q;
            const int64_t gi = i0 + bi + i, gj = j0 + bj + j;
            double w = 0.0, h = 0.0;
            if (i < nIb && j < nJb && gi >= gj) {
                w = (gi == gj ? 1.0 : 2.0) * (ai[p] * aj[q] - Kinv[gi + gj * N]);
                sk = fma(w, n2m_kval<KIND>(wgt[p][q], f), sk);
                st += gi == gj ? w : 0.0;
                h = n2m_hval<KIND>(wgt[p][q], f);
            }
            wgt[p][q] = w * h;
        }
    for (int d0 = 0; d0 < D; d0 += DC) {
        n2m_stage(xi, xj, Xn, D, d0, i0 + bi, nIb, j0 + bj, nJb);
        __syncthreads();
        const int dn = min(DC, D - d0);
        for (int dd = 0; dd < dn; ++dd) {
            double acc = 0.0;
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double df = xi[tx + 16 * p][dd] - xj[ty + 16 * q][dd];
                    acc = fma(wgt[p][q] * df, df, acc);
                }
            acc = block_sum(acc, smem);
            if (threadIdx.x == 0) out[d0 + dd] = acc;
        }
        __syncthreads();
    }
    sk = block_sum(sk, smem);
    st = block_sum(st, smem);
    if (threadIdx.x == 0) { out[D] = sk; out[D + 1] = st; }
}

// Ks[i + n N] = f kappa(x_i, xnew_n): one thread per entry (Xs: the b new points divided by the lengthscales, row-major)
template <int KIND>
__global__ __launch_bounds__(256) void gpr_cross_kernel(const double* __restrict__ Xn, const double* __restrict__ Xs, int64_t N, int D, double f,
                                                        double* __restrict__ Ks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (i >= N) return;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
        const double df = Xn[i * D + d] - Xs[n * D + d];
        d2 = fma(df, df, d2);
    }
    Ks[i + n * N] = n2m_kval<KIND>(d2, f);
}

// var[n] = f - sum_i V[i + n N]^2 and mean[n] += mu (one block per column, fixed order)
__global__ __launch_bounds__(256) void gpr_colnorm_kernel(const double* __restrict__ V, int64_t N, double f, double mu, double* __restrict__ mean_io,
                                                          double* __restrict__ var_out) {
    __shared__ double smem[16];
    const int64_t n = blockIdx.x;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += blockDim.x) { const double v = V[i + n * N]; s = fma(v, v, s); }
    s = block_sum(s, smem);
    if (threadIdx.x == 0) { var_out[n] = f - s; mean_io[n] += mu; }
}

// x[i] = v
__global__ __launch_bounds__(256) void gpr_set_kernel(double* __restrict__ x, int64_t n, double v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = v;
}

int gpr_alloc(cglb_ctx* c, double** p, size_t elems) {
    if (*p) return CGLB_OK;
    CGLB_TRY(c->gpr_mem.alloc(c, p, elems * sizeof(double)));
    c->gpr_bytes += elems * sizeof(double);
    return CGLB_OK;
}

int gpr_reserve(cglb_ctx* c, double** p, size_t* cap, size_t elems) {
    const size_t before = *cap;
    CGLB_TRY(c->gpr_mem.reserve(c, p, cap, elems * sizeof(double)));
    c->gpr_bytes += *cap - before;
    return CGLB_OK;
}

int gpr_require(cglb_ctx* c) {
    if (c->dtype != CGLB_F64)  // log|K| and the difference alpha alpha^T - K^-1 of an N x N matrix lose every digit the gradient needs in fp32
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the exact GPR class needs an fp64 context (-t fp64): the dense N x N factorisation is not available in fp32");
    if (c->r0 != 0 || c->r1 != c->N || c->par_world > 1 || c->comm)
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the exact GPR class needs a single shard covering all rows on one rank");
    if (c->p > 1)
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the exact GPR class takes one target column (the context holds " + std::to_string(c->p) + ")");
    return CGLB_OK;
}

// bytes rocSOLVER's potri asks of the rocBLAS handle for its workspace (0 if the query is not answered)
size_t gpr_potri_workspace(cglb_ctx* c) {
    size_t bytes = 0;
    if (rocblas_start_device_memory_size_query(c->blas) != rocblas_status_success) return 0;
    (void)rocsolver_dpotri(c->blas, rocblas_fill_lower, (rocblas_int)c->N, nullptr, (rocblas_int)c->N, nullptr);
    if (rocblas_stop_device_memory_size_query(c->blas, &bytes) != rocblas_status_success) return 0;
    return bytes;
}

// Every buffer an evaluation needs.  The two N x N matrices dominate: what is still to be allocated is compared with the free device memory
// first, so that a problem that does not fit says so instead of failing inside hipMalloc.
int gpr_reserve_buffers(cglb_ctx* c, bool with_grad) {
    const size_t N = (size_t)c->N, D = (size_t)c->D;
    const size_t nb = (size_t)std::min<int64_t>(c->gpr_block, (c->N + 63) & ~(int64_t)63), tb = nb / NT;
    const size_t scratch = (nb * nb + tb * tb * (D + 2) + N * D + 3 * N + 2 * D + 16) * sizeof(double);
    size_t need = 0;
    if (!c->gpr_L) need += N * N * sizeof(double) + scratch;
    if (with_grad && !c->gpr_Kinv) need += N * N * sizeof(double) + gpr_potri_workspace(c);
    if (need > 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(c, hipMemGetInfo(&free_b, &total_b));
        if (need > free_b)
            return cglb_fail(c, CGLB_ERR_HIP, "the exact GPR evaluation at N = " + std::to_string(c->N) + " needs " + std::to_string(need >> 20) +
                                                  " MiB for the N x N factor" + (with_grad ? ", the N x N inverse" : "") + " and their scratch but only " +
                                                  std::to_string(free_b >> 20) + " MiB of device memory are free: use a sparse model class (cglb, sgpr) at this size");
    }
    CGLB_TRY(gpr_alloc(c, &c->gpr_Xn, N * D));
    CGLB_TRY(gpr_alloc(c, &c->gpr_lsd, D));
    if (!c->gpr_L) {  // the strict upper triangles are never written: zero once, so that no library routine handed the lower triangle meets stray bits
        CGLB_TRY(gpr_alloc(c, &c->gpr_L, N * N));
        CGLB_TRY(gpr_alloc(c, &c->gpr_blk, nb * nb));
        HIP_CHECK(c, hipMemsetAsync(c->gpr_L, 0, N * N * sizeof(double), c->stream));
        HIP_CHECK(c, hipMemsetAsync(c->gpr_blk, 0, nb * nb * sizeof(double), c->stream));
    }
    CGLB_TRY(gpr_alloc(c, &c->gpr_e, N));
    CGLB_TRY(gpr_alloc(c, &c->gpr_alpha, N));
    if (!c->gpr_ones) {
        CGLB_TRY(gpr_alloc(c, &c->gpr_ones, N));
        hipLaunchKernelGGL(gpr_set_kernel, dim3((unsigned)std::min<size_t>(1024, (N + 255) / 256)), dim3(256), 0, c->stream, c->gpr_ones, (int64_t)N, 1.0);
        CGLB_LAUNCH_CHECK(c);
    }
    CGLB_TRY(gpr_alloc(c, &c->gpr_part, tb * tb * (D + 2)));
    CGLB_TRY(gpr_alloc(c, &c->gpr_acc, D + 2));
    CGLB_TRY(gpr_alloc(c, &c->gpr_scal, 8));
    if (!c->gpr_info) {
        CGLB_TRY(c->gpr_mem.alloc(c, &c->gpr_info, 4 * sizeof(int)));
        c->gpr_bytes += 4 * sizeof(int);
    }
    if (with_grad) CGLB_TRY(gpr_alloc(c, &c->gpr_Kinv, N * N));
    for (hipEvent_t& ev : c->gpr_ev)
        if (!ev) HIP_CHECK(c, hipEventCreate(&ev));
    return CGLB_OK;
}

int gpr_mark(cglb_ctx* c, int k) {
    HIP_CHECK(c, hipEventRecord(c->gpr_ev[k], c->stream));
    c->gpr_ev_last = k;
    return CGLB_OK;
}

int gpr_read_info(cglb_ctx* c, int slot, int* host) {
    HIP_CHECK(c, hipMemcpyAsync(host, c->gpr_info + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return CGLB_OK;
}

int gpr_tricopy(cglb_ctx* c, const double* src, int64_t lds, double* dst, int64_t ldd, int n) {
    hipLaunchKernelGGL(gpr_tricopy_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, c->stream, src, lds, dst, ldd, n);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// Xn = X / l and the lower triangle of K, tile by tile
int gpr_fill(cglb_ctx* c, int64_t nb) {
    const int64_t N = c->N;
    const int D = c->D;
    HIP_CHECK(c, hipMemcpyAsync(c->gpr_lsd, c->gpr_ls.data(), (size_t)D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(n2m_scale_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)c->X, (const double*)c->gpr_lsd, N, D, c->gpr_Xn);
    CGLB_LAUNCH_CHECK(c);
    for (int64_t j0 = 0; j0 < N; j0 += nb)
        for (int64_t i0 = j0; i0 < N; i0 += nb) {
            const int nI = (int)std::min(nb, N - i0), nJ = (int)std::min(nb, N - j0);
            dim3 grid((unsigned)((nI + NT - 1) / NT), (unsigned)((nJ + NT - 1) / NT));
            CGLB_DISPATCH_KIND(c->kind, hipLaunchKernelGGL((gpr_fill_kernel<KIND>), grid, dim3(256), 0, c->stream, (const double*)c->gpr_Xn, D, i0, nI,
                                                           j0, nJ, c->gpr_var, c->gpr_noise, c->gpr_L, N));
            CGLB_LAUNCH_CHECK(c);
        }
    return CGLB_OK;
}

// in-place right-looking factorisation of the lower triangle in gpr_L
int gpr_factor(cglb_ctx* c, int64_t nb) {
    const int64_t N = c->N;
    const double one = 1.0, mone = -1.0;
    double* L = c->gpr_L;
    for (int64_t j0 = 0; j0 < N; j0 += nb) {
        const int w = (int)std::min(nb, N - j0);
        double* Ljj = L + j0 + j0 * N;
        CGLB_TRY(gpr_tricopy(c, Ljj, N, c->gpr_blk, w, w));
        CGLB_TRY(launch_cholesky_lower_n(c, c->gpr_blk, w, c->gpr_info));
        int info = 0;
        CGLB_TRY(gpr_read_info(c, 0, &info));
        if (info != 0)  // info counts inside the block: the index reported is the row of K
            return cglb_fail(c, CGLB_ERR_NOT_PD, "exact GPR: K = f kappa(X, X) + s I is not positive definite (non-positive pivot at row " +
                                                     std::to_string(j0 + info - 1) + " of " + std::to_string(N) + ")");
        CGLB_TRY(gpr_tricopy(c, c->gpr_blk, w, Ljj, N, w));
        const int64_t r0 = j0 + w, rest = N - r0;
        if (rest <= 0) break;
        // block column below: L_ij = K_ij L_jj^-T
        BLAS_CHECK(c, rocblas_dtrsm(c->blas, rocblas_side_right, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, (int)rest, w,
                                    &one, c->gpr_blk, w, L + r0 + j0 * N, (int)N));
        // trailing lower triangle, one tile column at a time: K_tt -= P_t P_t^T (syrk), K_bt -= P_b P_t^T for the rows below (gemm)
        for (int64_t t0 = r0; t0 < N; t0 += nb) {
            const int wt = (int)std::min(nb, N - t0);
            const double* Pt = L + t0 + j0 * N;
            BLAS_CHECK(c, rocblas_dsyrk(c->blas, rocblas_fill_lower, rocblas_operation_none, wt, w, &mone, Pt, (int)N, &one, L + t0 + t0 * N, (int)N));
            const int64_t below = N - t0 - wt;
            if (below > 0)
                BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_transpose, (int)below, wt, w, &mone, Pt + wt, (int)N, Pt,
                                            (int)N, &one, L + t0 + wt + t0 * N, (int)N));
        }
    }
    return CGLB_OK;
}

// sum_ij W_ij {h_ij delta_ijd^2, k_ij} and tr W over the lower tile triangle into gpr_acc [D + 2]
int gpr_grad_pass(cglb_ctx* c, int64_t nb) {
    const int64_t N = c->N;
    const int D = c->D, P = D + 2;
    HIP_CHECK(c, hipMemsetAsync(c->gpr_acc, 0, (size_t)P * sizeof(double), c->stream));
    for (int64_t j0 = 0; j0 < N; j0 += nb)
        for (int64_t i0 = j0; i0 < N; i0 += nb) {
            const int nI = (int)std::min(nb, N - i0), nJ = (int)std::min(nb, N - j0);
            dim3 grid((unsigned)((nI + NT - 1) / NT), (unsigned)((nJ + NT - 1) / NT));
            CGLB_DISPATCH_KIND(c->kind, hipLaunchKernelGGL((gpr_grad_kernel<KIND>), grid, dim3(256), 0, c->stream, (const double*)c->gpr_Xn, D, i0, nI,
                                                           j0, nJ, c->gpr_var, (const double*)c->gpr_alpha, (const double*)c->gpr_Kinv, N, c->gpr_part));
            CGLB_LAUNCH_CHECK(c);
            hipLaunchKernelGGL(n2m_part_reduce_kernel, dim3(P), dim3(256), 0, c->stream, (const double*)c->gpr_part, (int64_t)grid.x * grid.y, P, 1.0,
                               c->gpr_acc);
            CGLB_LAUNCH_CHECK(c);
        }
    return CGLB_OK;
}

int gpr_evaluate(cglb_ctx* c, double* out3, double* grad) {
    CGLB_TRY(gpr_require(c));
    if (!c->have_data || !c->gpr_have_hypers) return cglb_fail(c, CGLB_ERR_STATE, "set_data and cglb_gpr_set_hypers must precede the exact GPR evaluation");
    HIP_CHECK(c, hipSetDevice(c->device));
    const bool with_grad = grad != nullptr;
    CGLB_TRY(gpr_reserve_buffers(c, with_grad));
    const int64_t N = c->N;
    const int D = c->D;
    const int64_t nb = std::min<int64_t>(c->gpr_block, (N + 63) & ~(int64_t)63);
    c->gpr_factored = false;
    c->gpr_hot_valid = false;
    CGLB_TRY(gpr_mark(c, 0));
    CGLB_TRY(gpr_fill(c, nb));
    CGLB_TRY(gpr_mark(c, 1));
    CGLB_TRY(gpr_factor(c, nb));
    CGLB_TRY(gpr_mark(c, 2));
    // e = y - c, alpha = L^-T L^-1 e, the three scalars
    CGLB_TRY(launch_sub_scalar(c, c->gpr_e, c->y, c->gpr_mean, N));
    HIP_CHECK(c, hipMemcpyAsync(c->gpr_alpha, c->gpr_e, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    BLAS_CHECK(c, rocblas_dtrsv(c->blas, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, (int)N, c->gpr_L, (int)N, c->gpr_alpha, 1));
    BLAS_CHECK(c, rocblas_dtrsv(c->blas, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, (int)N, c->gpr_L, (int)N, c->gpr_alpha, 1));
    CGLB_TRY(launch_dot(c, c->gpr_e, c->gpr_alpha, N, c->gpr_scal));
    CGLB_TRY(launch_dot(c, c->gpr_ones, c->gpr_alpha, N, c->gpr_scal + 1));
    hipLaunchKernelGGL(gpr_sumlog_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->gpr_L, N, c->gpr_scal + 2);
    CGLB_LAUNCH_CHECK(c);
    CGLB_TRY(gpr_mark(c, 3));
    double h[3];
    HIP_CHECK(c, hipMemcpyAsync(h, c->gpr_scal, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    c->gpr_factored = true;
    const double quad = -0.5 * h[0], logdet = -h[2];
    if (out3) { out3[0] = quad + logdet - 0.5 * (double)N * std::log(2.0 * M_PI); out3[1] = quad; out3[2] = logdet; }
    if (!with_grad) return CGLB_OK;
    // K^-1 from a copy of the factor; potri reads and writes the lower triangle only
    HIP_CHECK(c, hipMemcpyAsync(c->gpr_Kinv, c->gpr_L, (size_t)N * N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    BLAS_CHECK(c, rocsolver_dpotri(c->blas, rocblas_fill_lower, (rocblas_int)N, c->gpr_Kinv, (rocblas_int)N, (rocblas_int*)c->gpr_info + 1));
    int info = 0;
    CGLB_TRY(gpr_read_info(c, 1, &info));
    if (info != 0) return cglb_fail(c, CGLB_ERR_NOT_PD, "exact GPR: the inverse of the factor is singular at row " + std::to_string(info - 1));
    CGLB_TRY(gpr_mark(c, 4));
    CGLB_TRY(gpr_grad_pass(c, nb));
    CGLB_TRY(gpr_mark(c, 5));
    std::vector<double> acc((size_t)D + 2);
    HIP_CHECK(c, hipMemcpyAsync(acc.data(), c->gpr_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    for (int d = 0; d < D; ++d) grad[d] = 0.5 * acc[d] / c->gpr_ls[d];
    grad[D] = 0.5 * acc[D] / c->gpr_var;  // the kernel sums w_ij f kappa_ij
    grad[D + 1] = 0.5 * acc[D + 1];
    grad[D + 2] = h[1];
    return CGLB_OK;
}

// c->gpr_Xh <- X in the pair kernel's hot units at gpr_ls, once per evaluation (gpr_evaluate voids it); mid widths: [N][Dh] by launch_hot_points_mid with
// the scales in the device copy gpr_cs
int gpr_stage_training_hot(cglb_ctx* c, bool mid) {
    const int64_t N = c->N;
    const int D = c->D;
    CGLB_TRY(gpr_alloc(c, &c->gpr_Xh, (size_t)N * (size_t)predict_grad_row_stride(c)));
    if (mid) CGLB_TRY(gpr_alloc(c, &c->gpr_cs, (size_t)2 * D));
    if (c->gpr_hot_valid) return CGLB_OK;
    if (mid) {
        std::vector<double> cs((size_t)2 * D);
        for (int d = 0; d < D; ++d) { cs[d] = c->xmean[d]; cs[D + d] = cglb_kscale(c) / c->gpr_ls[d]; }
        HIP_CHECK(c, hipMemcpyAsync(c->gpr_cs, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(c, hipStreamSynchronize(c->stream));  // `cs` is pageable host memory
        CGLB_TRY(launch_hot_points_mid(c, c->gpr_cs, (const double*)c->X, N, c->gpr_Xh));
    } else {
        CGLB_TRY(launch_hot_points(c, c->gpr_ls.data(), (const double*)c->X, N, c->gpr_Xh));
    }
    c->gpr_hot_valid = true;
    return CGLB_OK;
}

// Wt[m * ldw + i] = alpha_m alpha_{i0 + i} - K^-1(m, i0 + i), m < n, i < nb: the block column of the symmetrised weight of the training-input gradient, K^-1
// read from its lower triangle (column-major, ld n)
__global__ __launch_bounds__(256) void gpr_weight_block_kernel(const double* __restrict__ alpha, const double* __restrict__ Kinv, int64_t n, int64_t i0, int64_t nb,
                                                               int64_t ldw, double* __restrict__ Wt) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * nb) return;
    const int64_t m = idx / nb, i = i0 + (idx - m * nb);
    const int64_t r = m > i ? m : i, q = m > i ? i : m;
    Wt[m * ldw + (i - i0)] = alpha[m] * alpha[i] - Kinv[r + q * n];
}

// gx[i, k] = sum_j (alpha_i alpha_j - K^-1_ij) d k(x_i, x_j) / d x_ik after an evaluation with gradients (gpr_alpha, gpr_Kinv): one row-weighted
// gradient product (kernels_predict_grad.hip) per row block of the factorisation's block edge, rows = points = X
int gpr_input_grad(cglb_ctx* c, double* gx) {
    const int64_t N = c->N;
    const int64_t nb = std::min<int64_t>(c->gpr_block, (N + 63) & ~(int64_t)63);
    const int64_t ldw = (std::min(nb, N) + 7) & ~(int64_t)7;
    size_t need = 0;
    if (!c->gpr_Xh) need += (size_t)N * c->Dp * sizeof(double);
    if (c->gpr_Wt_cap < (size_t)N * ldw * sizeof(double)) need += (size_t)N * ldw * sizeof(double);
    if (need > 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(c, hipMemGetInfo(&free_b, &total_b));
        if (need > free_b)
            return cglb_fail(c, CGLB_ERR_HIP, "the exact GPR training-input gradient at N = " + std::to_string(N) + " needs " + std::to_string(need >> 20) +
                                                  " MiB for the weights of a row block but only " + std::to_string(free_b >> 20) + " MiB of device memory are free");
    }
    CGLB_TRY(gpr_reserve(c, &c->gpr_Wt, &c->gpr_Wt_cap, (size_t)N * ldw));
    CGLB_TRY(gpr_stage_training_hot(c, false));
    for (int64_t i0 = 0; i0 < N; i0 += nb) {
        const int64_t nbi = std::min(nb, N - i0);
        hipLaunchKernelGGL(gpr_weight_block_kernel, dim3((unsigned)((N * nbi + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->gpr_alpha,
                           (const double*)c->gpr_Kinv, N, i0, nbi, ldw, c->gpr_Wt);
        CGLB_LAUNCH_CHECK(c);
        CGLB_TRY(launch_weighted_grad(c, c->gpr_ls.data(), c->gpr_var, c->gpr_Xh + i0 * c->Dp, nbi, c->gpr_Xh, N, nullptr, c->gpr_Wt, ldw, nullptr, nullptr, false,
                                      nullptr, gx + i0 * c->D, 1.0, nullptr));
    }
    return CGLB_OK;
}

// cglb_gpr_predict, and with g_mean set cglb_gpr_predict_grad (var_out / g_var NULL: the mean and its gradient alone), batch by batch
int gpr_predict_batches(cglb_ctx* c, const void* xnew, int64_t n_new, double* mean_out, double* g_mean, double* var_out, double* g_var) {
    CGLB_TRY(gpr_require(c));
    if (!c->gpr_factored) CGLB_TRY(gpr_evaluate(c, nullptr, nullptr));
    HIP_CHECK(c, hipSetDevice(c->device));
    const int64_t N = c->N;
    const int D = c->D;
    const int64_t bmax = std::min(GPR_PREDICT_BATCH, n_new);
    if (bmax == 0) return CGLB_OK;
    const int64_t ldc = (bmax + 7) & ~(int64_t)7;
    const bool mid = g_mean && input_grad_mid_on(c);             // mid width: hot sets [.][Dh] by launch_hot_points_mid, scales from the device copy gpr_cs
    const size_t hw = (size_t)predict_grad_row_stride(c);        // doubles per point of gpr_Xh / gpr_xh
    if (g_mean) {  // X and the batch in the pair kernel's units, C as [N][ldc]: checked against the free memory like the factor
        size_t need = 0;
        if (!c->gpr_Xh) need += (size_t)N * hw * sizeof(double);
        if (c->gpr_Ks_cap < (size_t)N * bmax * sizeof(double)) need += (size_t)N * bmax * sizeof(double);
        if (g_var && c->gpr_Ct_cap < (size_t)N * ldc * sizeof(double)) need += (size_t)N * ldc * sizeof(double);
        if (need > 0) {
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(c, hipMemGetInfo(&free_b, &total_b));
            if (need > free_b)
                return cglb_fail(c, CGLB_ERR_HIP, "the exact GPR input gradients at N = " + std::to_string(N) + " need " + std::to_string(need >> 20) +
                                                      " MiB for the panels of a batch but only " + std::to_string(free_b >> 20) + " MiB of device memory are free");
        }
        CGLB_TRY(gpr_reserve(c, &c->gpr_xh, &c->gpr_xh_cap, (size_t)bmax * hw));
        if (g_var) CGLB_TRY(gpr_reserve(c, &c->gpr_Ct, &c->gpr_Ct_cap, (size_t)N * ldc));
        CGLB_TRY(gpr_stage_training_hot(c, mid));
    }
    CGLB_TRY(gpr_reserve(c, &c->gpr_Ks, &c->gpr_Ks_cap, (size_t)N * bmax));
    CGLB_TRY(gpr_reserve(c, &c->gpr_xnew, &c->gpr_xnew_cap, (size_t)2 * bmax * D));
    DevTemps tmp;
    double* var_tmp = nullptr;  // the column-norm kernel always writes a variance
    if (!var_out) CGLB_TRY(tmp.alloc(c, (void**)&var_tmp, (size_t)bmax * sizeof(double)));
    const double one = 1.0, zero = 0.0;
    int rc = CGLB_OK;
    for (int64_t off = 0; off < n_new && rc == CGLB_OK; off += GPR_PREDICT_BATCH) rc = [&]() -> int {
        const int64_t b = std::min(GPR_PREDICT_BATCH, n_new - off);
        double* raw = c->gpr_xnew + bmax * D;
        HIP_CHECK(c, hipMemcpyAsync(raw, (const double*)xnew + off * D, (size_t)b * D * sizeof(double), hipMemcpyDefault, c->stream));
        hipLaunchKernelGGL(n2m_scale_kernel, dim3((unsigned)std::min<int64_t>(1024, (b * D + 255) / 256)), dim3(256), 0, c->stream, (const double*)raw,
                           (const double*)c->gpr_lsd, b, D, c->gpr_xnew);
        CGLB_LAUNCH_CHECK(c);
        dim3 grid((unsigned)((N + 255) / 256), (unsigned)b);
        CGLB_DISPATCH_KIND(c->kind, hipLaunchKernelGGL((gpr_cross_kernel<KIND>), grid, dim3(256), 0, c->stream, (const double*)c->gpr_Xn,
                                                       (const double*)c->gpr_xnew, N, D, c->gpr_var, c->gpr_Ks));
        CGLB_LAUNCH_CHECK(c);
        // mean = K_*f alpha (+ c below); variance = f - |L^-1 K_f*|^2 column-wise
        BLAS_CHECK(c, rocblas_dgemv(c->blas, rocblas_operation_transpose, (int)N, (int)b, &one, c->gpr_Ks, (int)N, c->gpr_alpha, 1, &zero, mean_out + off, 1));
        BLAS_CHECK(c, rocblas_dtrsm(c->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, (int)N, (int)b, &one,
                                    c->gpr_L, (int)N, c->gpr_Ks, (int)N));
        hipLaunchKernelGGL(gpr_colnorm_kernel, dim3((unsigned)b), dim3(256), 0, c->stream, (const double*)c->gpr_Ks, N, c->gpr_var, c->gpr_mean,
                           mean_out + off, var_out ? var_out + off : var_tmp);
        CGLB_LAUNCH_CHECK(c);
        if (!g_mean) return CGLB_OK;
        // C = L^-T (L^-1 K_f*) in place, transposed to [N][ldc] (a transpose pass); one launch against X with u = alpha, Wt = C
        if (mid) CGLB_TRY(launch_hot_points_mid(c, c->gpr_cs, raw, b, c->gpr_xh));
        else CGLB_TRY(launch_hot_points(c, c->gpr_ls.data(), raw, b, c->gpr_xh));
        if (g_var) {
            BLAS_CHECK(c, rocblas_dtrsm(c->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, (int)N, (int)b,
                                        &one, c->gpr_L, (int)N, c->gpr_Ks, (int)N));
            CGLB_TRY(launch_transpose(c, c->gpr_Ks, N, b, N, c->gpr_Ct, ldc));
        }
        return launch_weighted_grad(c, c->gpr_ls.data(), c->gpr_var, c->gpr_xh, b, c->gpr_Xh, N, c->gpr_alpha, g_var ? c->gpr_Ct : nullptr, ldc, nullptr,
                                    g_mean + off * D, false, nullptr, g_var ? g_var + off * D : nullptr, -2.0, mid ? c->gpr_cs + D : nullptr);
    }();
    if (var_tmp) (void)hipStreamSynchronize(c->stream);  // before `tmp` frees
    return rc;
}

}  // namespace

void gpr_free(cglb_ctx* c) {
    c->gpr_mem.release();
    c->gpr_bytes = 0;
    c->gpr_factored = false;
    c->gpr_hot_valid = false;
}

int gpr_stat(cglb_ctx* c, const char* name, double* value) {
    if (!strcmp(name, "gpr_bytes")) { *value = (double)c->gpr_bytes; return CGLB_OK; }
    static const struct { const char* name; int from, to; } phases[] = {
        {"gpr_fill_ms", 0, 1}, {"gpr_factor_ms", 1, 2}, {"gpr_solve_ms", 2, 3}, {"gpr_inverse_ms", 3, 4}, {"gpr_grad_ms", 4, 5}};
    for (const auto& ph : phases)
        if (!strcmp(name, ph.name)) {
            *value = 0.0;
            if (!c->gpr_ev[0] || c->gpr_ev_last < ph.to) return CGLB_OK;  // the last evaluation did not reach that phase
            float ms = 0.0f;
            HIP_CHECK(c, hipEventSynchronize(c->gpr_ev[ph.to]));
            HIP_CHECK(c, hipEventElapsedTime(&ms, c->gpr_ev[ph.from], c->gpr_ev[ph.to]));
            *value = (double)ms;
            return CGLB_OK;
        }
    return -1;
}

extern "C" {

int cglb_gpr_set_hypers(cglb_ctx* c, const double* lengthscales, double variance, double noise, double mean) {
    if (!c || !lengthscales) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "NULL argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(gpr_require(c));
    if (!c->have_data) return cglb_fail(c, CGLB_ERR_STATE, "set_data must precede cglb_gpr_set_hypers");
    // the noise is not required to be positive: whether K is positive definite is the factorisation's finding (CGLB_ERR_NOT_PD)
    if (!(variance > 0) || !std::isfinite(variance) || !std::isfinite(noise) || !std::isfinite(mean))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "variance must be positive, noise and mean finite");
    for (int d = 0; d < c->D; ++d)
        if (!(lengthscales[d] > 0) || !std::isfinite(lengthscales[d])) return cglb_fail(c, CGLB_ERR_BAD_ARG, "lengthscales must be positive");
    // repeating the current values keeps the factor (a predictor that pushes its model's parameters before every batch does not factor again)
    const bool same = c->gpr_have_hypers && variance == c->gpr_var && noise == c->gpr_noise && mean == c->gpr_mean &&
                      std::equal(c->gpr_ls.begin(), c->gpr_ls.end(), lengthscales);
    c->gpr_ls.assign(lengthscales, lengthscales + c->D);
    c->gpr_var = variance; c->gpr_noise = noise; c->gpr_mean = mean;
    c->gpr_have_hypers = true;
    if (!same) c->gpr_factored = false;
    return CGLB_OK;
}

int cglb_gpr_objective_and_grad(cglb_ctx* c, double* out3, double* grad) {
    if (!c || !out3) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "NULL argument") : CGLB_ERR_BAD_ARG;
    return gpr_evaluate(c, out3, grad);
}

int cglb_gpr_objective_and_grad_x(cglb_ctx* c, double* out3, double* grad, void* gx_out) {
    if (!c || !out3 || !grad || !gx_out) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "NULL argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(gpr_require(c));
    if (is_wide(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient has no wide path yet: it is available up to 32 input dimensions");
    CGLB_TRY(gpr_evaluate(c, out3, grad));
    return gpr_input_grad(c, (double*)gx_out);
}

int cglb_gpr_predict(cglb_ctx* c, const void* xnew, int64_t n_new, void* f_mean, void* f_var) {
    if (!c || !xnew || !f_mean || !f_var || n_new < 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "NULL argument") : CGLB_ERR_BAD_ARG;
    return gpr_predict_batches(c, xnew, n_new, (double*)f_mean, nullptr, (double*)f_var, nullptr);
}

int cglb_gpr_predict_grad(cglb_ctx* c, const void* xnew, int64_t n_new, void* f_mean, void* g_mean, void* f_var, void* g_var) {
    if (!c || !xnew || !f_mean || !g_mean || (!f_var) != (!g_var) || n_new < 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(gpr_require(c));
    if (is_wide(c) && !input_grad_mid_on(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the input-gradient products have no wide path yet: they are available up to 32 input dimensions, and at 33 to 96 with the "
                                              "option input_grad_mid 1 (fp64, wide_reg on)");
    return gpr_predict_batches(c, xnew, n_new, (double*)f_mean, (double*)g_mean, (double*)f_var, (double*)g_var);
}

}  // extern "C"
