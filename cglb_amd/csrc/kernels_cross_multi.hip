// Rectangular multi-column product  out[i, s] = var * sum_j kappa(xnew_i, x_j) V[j, s]  over all N training points, every kernel value
// evaluated ONCE per group of 8 columns.  It applies the Lanczos variance cache of the iterative exact-GP class (cglb_itergp_predict_cached:
// V = the N x r_pad factor R with K^-1 ~ R R^T; the reference reaches the same estimator through gpytorch.settings.fast_pred_var(),
// pytorch/interface.py:582) and is exposed on its own as cglb_cross_matmat.
//
// A row-slab product (row_slab.h) of the plain pair kernel's pairs: a lane keeps x_i, the row seed and R x 8 accumulators; the column range is
// split by the kff_jsplit rule; slab [jsplit][nrows][8].  The column side is row-major Vi[N][ldv] (ldv a multiple of 8), so the 8 values of a training point for one group are ONE contiguous
// scalar load next to x_j (kernels_grad_multi.hip interleaves its operands the same way), and every kernel value feeds 8 v_fma_f64 with a
// scalar source: k + 8 vector-fp64 instructions per pair and group against 8 (k + 1) for 8 single products.  S > 8 runs in groups of 8; a short
// group reads zero padding.  Always the range-clamped 2^x: new points may lie anywhere.  fp64, Dp <= 32.
// Register use of every instance: DESIGN.md section 4f.
#include "pair_common.h"
#include "row_slab.h"

#define CROSS_MULTI_ROWS 16384    // new points per launch: bounds the slab at ROW_SLAB_SLOTS * CROSS_MULTI_ROWS * 8 doubles

// rows per lane: the rule of the plain kernel (4 up to padded width 8, 2 up to 16, 1 beyond), halved while the R (DP + 8) row-resident doubles
// exceed 64 (half of the 256 VGPRs): with 8 accumulators per row the rule holds as it stands (64 at DP = 8, 48 at DP = 16, 40 at DP = 32)
static constexpr int cross_multi_rows_per_lane(int dp) {
    int r = dp <= 8 ? 4 : (dp <= 16 ? 2 : 1);
    while (r > 1 && r * (dp + CROSS_MULTI_SP) > 64) r /= 2;
    return r;
}

// Vi[j][b] = V[b][j] for b < s, zero for s <= b < ldv
__global__ __launch_bounds__(256) void cross_multi_operand_kernel(const double* __restrict__ V, int s, int ldv, int64_t n, double* __restrict__ Vi) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * ldv) return;
    const int64_t j = idx / ldv;
    const int b = (int)(idx - j * ldv);
    Vi[idx] = b < s ? V[(int64_t)b * n + j] : 0.0;
}

// grid (row blocks of 256 R new points, column chunks of jchunk training points); Vi points at the first column of the group
template <int KIND, int DP, int R, int PREC>
__global__ __launch_bounds__(256) void cross_multi_kernel(const double* __restrict__ XsRow, const double* __restrict__ xaRow, int64_t nrows,
                                                          const double* __restrict__ Xs, const double* __restrict__ xa,
                                                          const double* __restrict__ Vi, int64_t ldv, int64_t ncols, int64_t jchunk,
                                                          double* __restrict__ part, const double* __restrict__ exp_tab) {
    constexpr int SP = CROSS_MULTI_SP;
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double xi[R][DP], ai[R], acc[R][SP];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = row_slab_clamped(rbase, k, nrows);
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[k][d] = XsRow[row * DP + d];
        ai[k] = cglb_kind_matern<KIND>() ? -0.5 * xaRow[row] : xaRow[row];  // seed of the Gram chain (any Matern kind: -|x|^2 / 2)
        row_slab_zero(acc[k]);
    }
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < ncols) ? j0 + jchunk : ncols;
    for (int64_t j = j0; j < j1; ++j) {
        const double aj = xa[j];
        const double* __restrict__ cj = Vi + j * ldv;  // wave-uniform: one scalar load of 8 doubles
        double xj[DP], vj[SP];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Xs[j * DP + d];
#pragma unroll
        for (int b = 0; b < SP; ++b) vj[b] = cj[b];
        double gram[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double g = ai[k];
#pragma unroll
            for (int d = 0; d < DP; ++d) g = __builtin_fma(xi[k][d], xj[d], g);
            gram[k] = g;
        }
        KappaPend<double> kp[R];
        kappa_hot_begin_batch<double, KIND, true, false, PREC, R>(gram, aj, tab, kp);  // the R range reductions share one rounding-mode window
#pragma unroll
        for (int k = 0; k < R; ++k) {
            kappa_hot_poly<double, KIND, PREC>(kp[k]);
            const double kv = kappa_hot_end<double, KIND>(kp[k]);
#pragma unroll
            for (int b = 0; b < SP; ++b) acc[k][b] = __builtin_fma(kv, vj[b], acc[k][b]);
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) row_slab_store(part, nrows, rbase + (int64_t)k * 256, acc[k]);
}

// f_var[i] = var - sum_{s < sp} blk[i][s]^2 in column order: the variance of the cached path from the summed block, not a second pass over pairs
__global__ __launch_bounds__(256) void cross_multi_var_kernel(const double* __restrict__ blk, int64_t nrows, int sp, int64_t ld, double var,
                                                              double* __restrict__ f_var) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const double* __restrict__ row = blk + i * ld;
    double q = 0.0;
    for (int s = 0; s < sp; ++s) q = __builtin_fma(row[s], row[s], q);
    f_var[i] = var - q;
}

// one group of 8 columns for the rows (XsRow, xaRow, nrows <= CROSS_MULTI_ROWS)
template <int KIND, int DP>
static int cross_multi_group(cglb_ctx* c, const double* XsRow, const double* xaRow, int64_t nrows, const double* Vi, int64_t ldv, int sg, double* out,
                             int64_t ldo) {
    constexpr int R = cross_multi_rows_per_lane(DP);
    const int64_t ncols = c->N;
    const int64_t bx = (nrows + 256 * R - 1) / (256 * R);
    int64_t jsplit = 0, jchunk = 0;
    row_slab_pair_split(c->kff_jsplit, bx, ncols, ROW_SLAB_SLOTS, true, &jsplit, &jchunk);
    CGLB_TRY(c->mem.reserve(c, &c->cm_part, &c->cm_part_cap, (size_t)jsplit * nrows * CROSS_MULTI_SP * sizeof(double)));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((cross_multi_kernel<KIND, DP, R, PREC>), dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream, XsRow,
                                             xaRow, nrows, (const double*)c->Xh, (const double*)c->xah, Vi, ldv, ncols, jchunk, (double*)c->cm_part,
                                             (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    return row_slab_finish<CROSS_MULTI_SP>(c, (const double*)c->cm_part, jsplit, nrows, sg, c->var, out, ldo);
}

int cross_multi_rows_per_block(const cglb_ctx* c) { return 256 * cross_multi_rows_per_lane(c->Dp); }
int cross_multi_width() { return CROSS_MULTI_SP; }

// out[i * ldo + s] = var * sum_j kappa(row_i, x_j) Vi[j * ldv + s], s < S <= ldv.  Vi: dev [N][ldv] row-major, ldv a multiple of 8, the columns
// S .. ldv - 1 of the last group readable (zero padding).  XsRow / xaRow: hot-scaled new points.  Rows in blocks of CROSS_MULTI_ROWS, columns
// in groups of 8.
int launch_cross_multi(cglb_ctx* c, const void* XsRow, const void* xaRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo) {
    if (c->dtype != CGLB_F64 || is_wide(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the multi-column cross product needs an fp64 context of at most 32 input dimensions");
    if (S < 1 || ldv < S || (ldv % CROSS_MULTI_SP) || ldo < S) return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad column count or leading dimension of the multi-column cross product");
    for (int64_t i0 = 0; i0 < nrows; i0 += CROSS_MULTI_ROWS) {
        const int64_t nr = std::min<int64_t>(CROSS_MULTI_ROWS, nrows - i0);
        const double* xs = (const double*)XsRow + i0 * c->Dp;
        const double* xa = (const double*)xaRow + i0;
        for (int b0 = 0; b0 < S; b0 += CROSS_MULTI_SP) {
            const int sg = std::min(CROSS_MULTI_SP, S - b0);
            CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((cross_multi_group<KIND, DP>(c, xs, xa, nr, Vi + b0, ldv, sg, out + i0 * ldo + b0, ldo)))));
        }
    }
    return CGLB_OK;
}

// the interleaved copy of V [S][N] (column b contiguous) in c->cm_vi [N][ldv], ldv = S rounded up to 8
int launch_cross_multi_operand(cglb_ctx* c, const void* V, int S, int64_t* ldv_out) {
    const int64_t ldv = ((int64_t)S + CROSS_MULTI_SP - 1) / CROSS_MULTI_SP * CROSS_MULTI_SP;
    CGLB_TRY(c->mem.reserve(c, &c->cm_vi, &c->cm_vi_cap, (size_t)c->N * ldv * sizeof(double)));
    hipLaunchKernelGGL(cross_multi_operand_kernel, dim3((unsigned)((c->N * ldv + 255) / 256)), dim3(256), 0, c->stream, (const double*)V, S, (int)ldv, c->N,
                       (double*)c->cm_vi);
    CGLB_LAUNCH_CHECK(c);
    *ldv_out = ldv;
    return CGLB_OK;
}

int launch_cross_multi_var(cglb_ctx* c, const double* blk, int64_t nrows, int sp, int64_t ld, double* f_var) {
    if (nrows == 0) return CGLB_OK;
    hipLaunchKernelGGL(cross_multi_var_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, blk, nrows, sp, ld, c->var, f_var);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}
