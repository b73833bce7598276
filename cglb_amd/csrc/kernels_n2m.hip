// N^2M log-det bound (option "logdet_bound" = 2: cglbn2m, sgprn2m; tensorflow/models.py:311-350, :353-413), fp64.
//
//   tau = tr K~ - tr(C K~ C^T) = N (f + s) - <B^-1, H> - s (M - tr B^-1),   H = A K_ff A^T = A W,  W = K_ff A^T  (N x M)
//   dT/dtheta = sum_ij G_ij dK_ij/dtheta,  G = C^T C = A^T B^-1 A,  T = tr(C K~ C^T)
//
// K_ff is never stored: the N x N kernel is materialised one tile K_IJ (J >= I, edge n2m_bt) at a time by n2m_tile_kernel and consumed
// by two rocBLAS GEMMs of depth n2m_bt (W_I += K_IJ A_J^T, W_J += K_IJ^T A_I^T: each tile of the symmetric matrix evaluated once, used
// twice).  The gradient pass forms G_IJ = C_I^T C_J (rocBLAS, depth M) into a second tile and n2m_grad_kernel re-evaluates the pairs of
// the tile, reducing sum G_ij h_ij delta_ijd^2 per input dimension (the pair weight of the K_ff gradient pass, read from G_IJ).
// Flops: 2 N^2 M (W) + N^2 M (G) = 3 N^2 M, all in GEMMs; the pair evaluations are O(N^2 D) on the vector units.
#include "n2m_pair.h"  // NT, DC, n2m_kval / n2m_hval / n2m_stage / n2m_d2, n2m_part_reduce_kernel, n2m_scale_kernel (shared with kernels_gpr.hip)

namespace {

// K[i + j ldk] = f kappa(x_{i0+i}, x_{j0+j}), i < nI, j < nJ (column-major tile)
template <int KIND>
__global__ __launch_bounds__(256) void n2m_tile_kernel(const double* __restrict__ Xn, int D, int64_t i0, int nI, int64_t j0, int nJ, double f,
                                                       double* __restrict__ K, int64_t ldk) {
    __shared__ double xi[NT][DC + 1], xj[NT][DC + 1];
    const int bi = blockIdx.x * NT, bj = blockIdx.y * NT;
    const int nIb = min(NT, nI - bi), nJb = min(NT, nJ - bj);
    double d2[4][4];
    n2m_d2(d2, xi, xj, Xn, D, i0 + bi, nIb, j0 + bj, nJb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = tx + 16 * p, j = ty + 16 * q;
            if (i < nIb && j < nJb) K[(int64_t)(bi + i) + (int64_t)(bj + j) * ldk] = n2m_kval<KIND>(d2[p][q], f);
        }
}

// part[blk * D + d] = sum over the block's pairs of G_ij h_ij delta_ijd^2 (fixed order inside the block)
template <int KIND>
__global__ __launch_bounds__(256) void n2m_grad_kernel(const double* __restrict__ Xn, int D, int64_t i0, int nI, int64_t j0, int nJ, double f,
                                                       const double* __restrict__ G, int64_t ldg, double* __restrict__ part) {
    __shared__ double xi[NT][DC + 1], xj[NT][DC + 1];
    __shared__ double smem[16];
    const int bi = blockIdx.x * NT, bj = blockIdx.y * NT;
    const int nIb = min(NT, nI - bi), nJb = min(NT, nJ - bj);
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    double wgt[4][4];
    n2m_d2(wgt, xi, xj, Xn, D, i0 + bi, nIb, j0 + bj, nJb);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tx + 16 * p, j = ty + 16 * q;
            wgt[p][q] = (i < nIb && j < nJb) ? G[(int64_t)(bi + i) + (int64_t)(bj + j) * ldg] * n2m_hval<KIND>(wgt[p][q], f) : 0.0;
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
            if (threadIdx.x == 0) part[blk * D + d0 + dd] = acc;
        }
        __syncthreads();
    }
}

// out[0] = tr P (M x M; one block over the diagonal)
__global__ __launch_bounds__(256) void n2m_trace_kernel(const double* __restrict__ P, int M, double* __restrict__ out) {
    __shared__ double smem[16];
    double t = 0.0;
    for (int i = threadIdx.x; i < M; i += blockDim.x) t += P[(int64_t)i * M + i];
    t = block_sum(t, smem);
    if (threadIdx.x == 0) out[0] = t;
}

// out = P + a Q (M x M)
__global__ __launch_bounds__(256) void n2m_add_kernel(const double* __restrict__ P, double a, const double* __restrict__ Q, int64_t n, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = P[k] + a * Q[k];
}

inline int n2m_alloc(cglb_ctx* c, double** p, size_t elems) { return c->n2m_mem.alloc(c, p, elems * sizeof(double)); }

inline int64_t n2m_tiles(const cglb_ctx* c) { return (c->N + c->n2m_bt - 1) / c->n2m_bt; }

int n2m_launch_tile(cglb_ctx* c, int64_t i0, int nI, int64_t j0, int nJ) {
    dim3 grid((unsigned)((nI + NT - 1) / NT), (unsigned)((nJ + NT - 1) / NT));
    CGLB_DISPATCH_KIND(c->kind, hipLaunchKernelGGL((n2m_tile_kernel<KIND>), grid, dim3(256), 0, c->stream, (const double*)c->n2m_Xn, c->D, i0, nI, j0,
                                                   nJ, c->var, c->n2m_K, c->n2m_bt));
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

}  // namespace

int n2m_setup(cglb_ctx* c) {
    if (c->dtype != CGLB_F64) return cglb_fail(c, CGLB_ERR_BAD_ARG, "logdet_bound 2 (N^2M) needs an fp64 context");
    if (c->precond_mode != 0) return cglb_fail(c, CGLB_ERR_BAD_ARG, "logdet_bound 2 (N^2M) needs the stored panel A (precond_mode 0)");
    if (c->r0 != 0 || c->r1 != c->N || c->par_world > 1) return cglb_fail(c, CGLB_ERR_BAD_ARG, "logdet_bound 2 (N^2M) needs a single shard covering all rows");
    const int M = c->M, D = c->D;
    const int64_t N = c->N, lda = c->lda;
    if (c->n2m_bt == 0) {
        c->n2m_bt = std::min<int64_t>(c->n2m_tile > 0 ? c->n2m_tile : 4096, (N + 63) & ~(int64_t)63);
        const int64_t nb = (c->n2m_bt + NT - 1) / NT;
        CGLB_TRY(n2m_alloc(c, &c->n2m_Xn, (size_t)N * D));
        CGLB_TRY(n2m_alloc(c, &c->n2m_ls, (size_t)D));
        CGLB_TRY(n2m_alloc(c, &c->n2m_Wt, (size_t)lda * M));
        CGLB_TRY(n2m_alloc(c, &c->n2m_K, (size_t)c->n2m_bt * c->n2m_bt));
        CGLB_TRY(n2m_alloc(c, &c->n2m_H, (size_t)M * M));
        CGLB_TRY(n2m_alloc(c, &c->n2m_T, (size_t)M * M));
        CGLB_TRY(n2m_alloc(c, &c->n2m_part, (size_t)nb * nb * D));
        CGLB_TRY(n2m_alloc(c, &c->n2m_gacc, (size_t)D));
        CGLB_TRY(n2m_alloc(c, &c->n2m_scal, 4));
    }
    HIP_CHECK(c, hipMemcpyAsync(c->n2m_ls, c->ls, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(n2m_scale_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)c->X, (const double*)c->n2m_ls, N, D, c->n2m_Xn);
    CGLB_LAUNCH_CHECK(c);
    // W = K_ff A^T, column-major N x M with ld lda (the layout of At): tiles on and right of the diagonal, each used for both blocks
    HIP_CHECK(c, hipMemsetAsync(c->n2m_Wt, 0, (size_t)lda * M * sizeof(double), c->stream));
    const double one = 1.0, zero = 0.0;
    const double* At = (const double*)c->At;
    const int64_t bt = c->n2m_bt, nt = n2m_tiles(c);
    for (int64_t I = 0; I < nt; ++I)
        for (int64_t J = I; J < nt; ++J) {
            const int64_t i0 = I * bt, j0 = J * bt;
            const int nI = (int)std::min(bt, N - i0), nJ = (int)std::min(bt, N - j0);
            CGLB_TRY(n2m_launch_tile(c, i0, nI, j0, nJ));
            BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_none, nI, M, nJ, &one, c->n2m_K, (int)bt, At + j0, (int)lda,
                                        &one, c->n2m_Wt + i0, (int)lda));
            if (J != I)
                BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_transpose, rocblas_operation_none, nJ, M, nI, &one, c->n2m_K, (int)bt, At + i0,
                                            (int)lda, &one, c->n2m_Wt + j0, (int)lda));
        }
    // H = A W (M x M, depth N); B^-1 = LB^-T LB^-1; <B^-1, H> and tr B^-1
    BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_transpose, rocblas_operation_none, M, M, (int)N, &one, At, (int)lda, c->n2m_Wt, (int)lda,
                                &zero, c->n2m_H, M));
    BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_transpose, rocblas_operation_none, M, M, M, &one, (const double*)c->LBinv, M,
                                (const double*)c->LBinv, M, &zero, c->n2m_T, M));
    CGLB_TRY(launch_dot(c, c->n2m_T, c->n2m_H, (int64_t)M * M, c->n2m_scal));   // <B^-1, H> over all blocks of the GPU
    hipLaunchKernelGGL(n2m_trace_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->n2m_T, M, c->n2m_scal + 1);
    CGLB_LAUNCH_CHECK(c);
    double h[2];
    HIP_CHECK(c, hipMemcpyAsync(h, c->n2m_scal, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const double s = c->noise, f = c->var;
    c->n2m_BH = h[0];
    c->n2m_trBinv = h[1];
    // tr(C K~ C^T) = tr(B^-1 A (K_ff + s I) A^T) = <B^-1, H> + s tr(B^-1 (B - I)) = <B^-1, H> + s (M - tr B^-1)
    c->n2m_tau = (double)N * (f + s) - h[0] - s * ((double)M - h[1]);
    if (!(c->n2m_tau > 0.0) || !std::isfinite(c->n2m_tau))
        return cglb_fail(c, CGLB_ERR_NOT_PD, "N^2M bound: tr K~ - tr(C K~ C^T) = " + std::to_string(c->n2m_tau) + " is not positive");
    return CGLB_OK;
}

int n2m_grad_terms(cglb_ctx* c, const double* Binv) {
    const int M = c->M, D = c->D;
    const int64_t N = c->N, lda = c->lda, bt = c->n2m_bt, nt = n2m_tiles(c);
    const double one = 1.0, zero = 0.0;
    const double* At = (const double*)c->At;
    CGLB_TRY(n2m_alloc(c, &c->n2m_E, (size_t)M * M));
    CGLB_TRY(n2m_alloc(c, &c->n2m_Ct, (size_t)lda * M));
    CGLB_TRY(n2m_alloc(c, &c->n2m_G, (size_t)bt * bt));
    // E = B^-1 (H + s A A^T) B^-1 and its trace
    const int64_t mm = (int64_t)M * M;
    hipLaunchKernelGGL(n2m_add_kernel, dim3((unsigned)((mm + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->n2m_H, c->noise,
                       (const double*)c->AAt, mm, c->n2m_E);
    BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_none, M, M, M, &one, Binv, M, c->n2m_E, M, &zero, c->n2m_T, M));
    BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_none, M, M, M, &one, c->n2m_T, M, Binv, M, &zero, c->n2m_E, M));
    hipLaunchKernelGGL(n2m_trace_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->n2m_E, M, c->n2m_scal + 3);
    // C^T = A^T LB^-T (layout of At)
    BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_transpose, (int)N, M, M, &one, At, (int)lda,
                                (const double*)c->LBinv, M, &zero, c->n2m_Ct, (int)lda));
    // sum_ij G_ij h_ij delta_ijd^2 over the upper tile triangle; an off-diagonal tile stands for itself and its transpose
    HIP_CHECK(c, hipMemsetAsync(c->n2m_gacc, 0, (size_t)D * sizeof(double), c->stream));
    for (int64_t I = 0; I < nt; ++I)
        for (int64_t J = I; J < nt; ++J) {
            const int64_t i0 = I * bt, j0 = J * bt;
            const int nI = (int)std::min(bt, N - i0), nJ = (int)std::min(bt, N - j0);
            BLAS_CHECK(c, rocblas_dgemm(c->blas, rocblas_operation_none, rocblas_operation_transpose, nI, nJ, M, &one, c->n2m_Ct + i0, (int)lda,
                                        c->n2m_Ct + j0, (int)lda, &zero, c->n2m_G, (int)bt));
            dim3 grid((unsigned)((nI + NT - 1) / NT), (unsigned)((nJ + NT - 1) / NT));
            CGLB_DISPATCH_KIND(c->kind, hipLaunchKernelGGL((n2m_grad_kernel<KIND>), grid, dim3(256), 0, c->stream, (const double*)c->n2m_Xn, D, i0, nI,
                                                           j0, nJ, c->var, (const double*)c->n2m_G, bt, c->n2m_part));
            hipLaunchKernelGGL(n2m_part_reduce_kernel, dim3(D), dim3(256), 0, c->stream, (const double*)c->n2m_part, (int64_t)grid.x * grid.y, D,
                               I == J ? 1.0 : 2.0, c->n2m_gacc);
            CGLB_LAUNCH_CHECK(c);
        }
    return CGLB_OK;
}

void n2m_free(cglb_ctx* c) {
    c->n2m_mem.release();
    c->n2m_bt = 0;
}
