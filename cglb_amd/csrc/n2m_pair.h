// Pair evaluation shared by the translation units that tile the N x N kernel matrix in fp64: the N^2M pass (kernels_n2m.hip) and the exact
// GPR pipeline (kernels_gpr.hip).  Blocks of 256 threads evaluate 64 x 64 pairs, 4 x 4 per thread, on the rows of Xn = X / l staged in LDS
// 16 dimensions at a time; per-block partial sums are added in fixed order by n2m_part_reduce_kernel.
#pragma once
#include "dispatch.h"

namespace {

constexpr int NT = 64;  // pairs per block edge: 16 x 16 threads, 4 x 4 pairs each
constexpr int DC = 16;  // input dimensions staged in LDS per step

template <int KIND>
__device__ __forceinline__ double n2m_kval(double d2, double f) {
    if constexpr (KIND == CGLB_RBF) {
        return f * exp(-0.5 * d2);
    } else if constexpr (KIND == CGLB_MATERN32) {
        const double r = sqrt(d2);
        return f * (1.0 + CGLB_SQRT3 * r) * exp(-CGLB_SQRT3 * r);
    } else if constexpr (KIND == CGLB_MATERN52) {
        const double s = CGLB_SQRT5 * sqrt(d2);
        return f * matern_kpoly<double, KIND>(s, 1.0) * exp(-s);
    } else {
        return (void)cglb_kind_unknown<KIND>{}, 0.0;
    }
}
// h with dk/dl_d = h delta_d^2 / l_d, delta_d = (x_id - x_jd) / l_d (oracle kernel_grad_factor)
template <int KIND>
__device__ __forceinline__ double n2m_hval(double d2, double f) {
    if constexpr (KIND == CGLB_RBF) {
        return f * exp(-0.5 * d2);
    } else if constexpr (KIND == CGLB_MATERN32) {
        return 3.0 * f * exp(-CGLB_SQRT3 * sqrt(d2));
    } else if constexpr (KIND == CGLB_MATERN52) {
        const double s = CGLB_SQRT5 * sqrt(d2);
        return f * matern_hpoly<double, KIND>(s, 1.0) * exp(-s);
    } else {
        return (void)cglb_kind_unknown<KIND>{}, 0.0;
    }
}

// stage dimensions [d0, d0 + DC) of the block's 64 rows of I and of J in LDS (zeros outside the tile and beyond D)
__device__ __forceinline__ void n2m_stage(double (*xi)[DC + 1], double (*xj)[DC + 1], const double* __restrict__ Xn, int D, int d0, int64_t ri,
                                          int nIb, int64_t rj, int nJb) {
    for (int k = threadIdx.x; k < NT * DC; k += 256) {
        const int r = k / DC, dd = k - r * DC, d = d0 + dd;
        xi[r][dd] = (r < nIb && d < D) ? Xn[(ri + r) * D + d] : 0.0;
        xj[r][dd] = (r < nJb && d < D) ? Xn[(rj + r) * D + d] : 0.0;
    }
}

// scaled squared distances of the thread's 4 x 4 pairs: rows bi + tx + 16 p of I, columns bj + ty + 16 q of J
__device__ __forceinline__ void n2m_d2(double (&d2)[4][4], double (*xi)[DC + 1], double (*xj)[DC + 1], const double* __restrict__ Xn, int D,
                                       int64_t ri, int nIb, int64_t rj, int nJb) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) d2[p][q] = 0.0;
    for (int d0 = 0; d0 < D; d0 += DC) {
        n2m_stage(xi, xj, Xn, D, d0, ri, nIb, rj, nJb);
        __syncthreads();
#pragma unroll 4
        for (int dd = 0; dd < DC; ++dd) {
            double a[4], b[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) { a[p] = xi[tx + 16 * p][dd]; b[p] = xj[ty + 16 * p][dd]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) { const double df = a[p] - b[q]; d2[p][q] = fma(df, df, d2[p][q]); }
        }
        __syncthreads();
    }
}

// acc[d] += scale * sum_b part[b * D + d]  (one block per dimension, fixed order)
__global__ __launch_bounds__(256) void n2m_part_reduce_kernel(const double* __restrict__ part, int64_t nblk, int D, double scale,
                                                              double* __restrict__ acc) {
    __shared__ double smem[16];
    const int d = blockIdx.x;
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += blockDim.x) s += part[b * D + d];
    s = block_sum(s, smem);
    if (threadIdx.x == 0) acc[d] += scale * s;
}

// Xn = X / l (row-major N x D)
__global__ __launch_bounds__(256) void n2m_scale_kernel(const double* __restrict__ X, const double* __restrict__ ls, int64_t N, int D,
                                                        double* __restrict__ Xn) {
    const int64_t n = (int64_t)N * D;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) Xn[k] = X[k] / ls[k % D];
}

}  // namespace
