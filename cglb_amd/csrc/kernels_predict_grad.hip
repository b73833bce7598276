// Row-weighted value AND input gradient of a cross product (cglb_cross_grad_weighted; the predictors cglb_predict_grad, cglb_gpr_predict_grad):
//   out_u[i] =  f sum_m u[m]     kappa(x*_i, p_m)     gout_u[i, k] = -f sum_m u[m]     h_im delta_imk / l_k
//   out_w[i] =  f sum_m Wt[m, i] kappa(x*_i, p_m)     gout_w[i, k] = -f sum_m Wt[m, i] h_im delta_imk / l_k
// with h the radial derivative factor (devmath.h: d kappa / d x*_k = -h delta_k / l_k, delta_k = (x*_k - p_k) / l_k).  u is the weight every new point
// shares (q of the CGLB mean, alpha of the exact GP); Wt[m][i] is new point i's OWN weight of point m (C^T of the variance), which the shared-column
// product of kernels_input_grad.hip can only express with one column per new point.  One evaluation of a pair serves both sums.
//
// A row-slab product (row_slab.h) of cross_grad_kernel's pairs: a lane keeps the coordinates and R x NW x (DP + 1) accumulators, NW = 2 or 1 by the
// template flags; point p_m and u[m] are wave-uniform scalar loads; Wt[m][.] has the new-point index fastest (ldw >= n_new, the layout of the
// predictive panels), so a wave reads 64 consecutive doubles per point, and the next point's weight is requested before the current pair's
// profile.  Rows past n_new read the last row's weight (never the padding columns [n_new, ldw)) and write nothing.  The point range is split by the
// kff_jsplit rule; slab [jsplit][nrows][NW][DP + 1]; ONE finish kernel applies f, -f / (l_k hot scale) and the caller's factor of the Wt gradient
// (-2 for g_var).  The split never depends on NW, and the u sums of the two-weight instance are the operations of the one-weight
// instance, so every output is bitwise the same whichever of the others are requested.
// Pair: DIRECT differences in hot units and kappa_hfac_hot_from_d2 (always the range-clamped 2^x), as cross_grad_kernel and for its reason; a
// coincident pair has delta = 0 exactly and adds exactly zero to the gradient.  fp64, Dp <= 32.  Register use of every instance: DESIGN.md 4i.
// Mid widths (33 .. 96 dimensions, option "input_grad_mid"): the same contract in kernels_predict_grad_mid.hip, where launch_weighted_grad sends each row block.
#include "pair_common.h"
#include "row_slab.h"
#include <cstring>

#define PREDICT_GRAD_ROWS 4096        // new points per launch

// rows per lane by padded width, chosen so that R (DP + 2 (DP + 1) + 2) + DP row-resident doubles (coordinates, both accumulator sets, the current and the
// next weight, the differences of the pair in flight) stay near 100: 4 up to width 4 (64 + 4), 2 up to 8 (56 + 8), 1 beyond (100 + 32 at 32)
static constexpr int predict_grad_rows_per_lane(int dp) { return dp <= 4 ? 4 : (dp <= 8 ? 2 : 1); }

// grid (row blocks of 256 R new points, chunks of jchunk points)
template <int KIND, int DP, int R, bool HAS_U, bool HAS_W, int PREC>
__global__ __launch_bounds__(256) void weighted_grad_kernel(const double* __restrict__ XhRow, int64_t nrows, const double* __restrict__ Ph, int64_t npts,
                                                            const double* __restrict__ u, const double* __restrict__ Wt, int64_t ldw, int64_t jchunk,
                                                            double* __restrict__ part, const double* __restrict__ exp_tab) {
    static_assert(HAS_U || HAS_W, "no weight");
    constexpr int NW = (HAS_U ? 1 : 0) + (HAS_W ? 1 : 0), IW = HAS_U ? 1 : 0;
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double xi[R][DP], acc[R][NW][DP + 1], wn[R];
    int64_t rowc[R];
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < npts) ? j0 + jchunk : npts;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        rowc[k] = row_slab_clamped(rbase, k, nrows);
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[k][d] = XhRow[rowc[k] * DP + d];
        row_slab_zero(acc[k]);
        wn[k] = (HAS_W && j0 < j1) ? Wt[j0 * ldw + rowc[k]] : 0.0;
    }
    for (int64_t j = j0; j < j1; ++j) {
        double xj[DP], wj[R];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Ph[j * DP + d];  // wave-uniform: scalar loads
        const double uj = HAS_U ? u[j] : 0.0;
        const int64_t jn = j + 1 < j1 ? j + 1 : j;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            wj[k] = wn[k];
            if (HAS_W) wn[k] = Wt[jn * ldw + rowc[k]];  // in flight during this pair's profile
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            // Written out, not row_slab_grad_acc / row_slab_store (row_slab.h): with the two calls the register allocation of 270 of the 351 instances
            // moves (167 with the accumulate alone, 27 with the store alone).  The difference loop as a function of its own moves 189 (and all 81 of
            // cross_grad_kernel, which keeps it written out too).
            double df[DP];
            double d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                df[d] = xi[k][d] - xj[d];
                d2 = __builtin_fma(df[d], df[d], d2);
            }
            double kv, hv;
            kappa_hfac_hot_from_d2<KIND, PREC>(d2, tab, kv, hv);
            if (HAS_U) {
                const double t = hv * uj;
#pragma unroll
                for (int d = 0; d < DP; ++d) acc[k][0][d] = __builtin_fma(t, df[d], acc[k][0][d]);
                acc[k][0][DP] = __builtin_fma(kv, uj, acc[k][0][DP]);
            }
            if (HAS_W) {
                const double t = hv * wj[k];
#pragma unroll
                for (int d = 0; d < DP; ++d) acc[k][IW][d] = __builtin_fma(t, df[d], acc[k][IW][d]);
                acc[k][IW][DP] = __builtin_fma(kv, wj[k], acc[k][IW][DP]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = rbase + (int64_t)k * 256;
        if (row < nrows) {
            double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (NW * (DP + 1));
#pragma unroll
            for (int b = 0; b < NW; ++b)
#pragma unroll
                for (int d = 0; d <= DP; ++d) o[b * (DP + 1) + d] = acc[k][b][d];
        }
    }
}

// the slabs in fixed order, then the constants; one thread per (i, b < nw, k <= dp).  Weight slot b writes out[b] / gout[b] (either may be NULL);
// gscale[b] multiplies the gradient constant, add_u adds the u gradient to what gout[0] holds (the K_*f v term of cglb_predict_grad)
struct PredictGradOut { double* out[2]; double* gout[2]; double gscale[2]; };
__global__ __launch_bounds__(256) void weighted_grad_finish_kernel(const double* __restrict__ part, int jsplit, int64_t nrows, int nw, int dp, int d, double vscale,
                                                                   RowSlabGradScale gs, PredictGradOut o, int add_u) {
    const int64_t per = (int64_t)nw * (dp + 1);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * per) return;
    const int64_t i = idx / per;
    const int e = (int)(idx - i * per);
    const int b = e / (dp + 1), k = e - b * (dp + 1);
    double* __restrict__ dst = k == dp ? o.out[b] : o.gout[b];
    if (!dst || (k >= d && k < dp)) return;
    double s = 0.0;
    for (int js = 0; js < jsplit; ++js) s += part[(int64_t)js * nrows * per + idx];
    if (k == dp) dst[i] = vscale * s;
    else {
        const double g = (o.gscale[b] * gs.g[k]) * s;
        dst[i * d + k] = (add_u && b == 0) ? dst[i * d + k] + g : g;
    }
}

// out[i * dp + k] = (x[i * d + k] - centre_k) * scale_k, zero in the padding (the exact GPR class stages X and its batches at its own lengthscales)
__global__ __launch_bounds__(256) void hot_points_kernel(const double* __restrict__ x, int64_t n, int d, int dp, ScaleParams sp, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * dp) return;
    const int64_t i = idx / dp;
    const int k = (int)(idx - i * dp);
    out[idx] = k < d ? (x[i * d + k] - sp.center[k]) * sp.scale[k] : 0.0;
}

// dst[j * ldd + i] = src[i * lds + j], i < rows, j < cols (C of the exact GPR class from its column-major panel to the [N][ld] layout)
__global__ __launch_bounds__(256) void transpose_kernel(const double* __restrict__ src, int64_t lds, int64_t rows, int64_t cols, double* __restrict__ dst, int64_t ldd) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t i0 = (int64_t)blockIdx.y * 32, jb = (int64_t)blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) {
        const int64_t i = i0 + r, j = jb + tx;
        tile[r][tx] = (i < rows && j < cols) ? src[i * lds + j] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t j = jb + r, i = i0 + tx;
        if (j < cols && i < rows) dst[j * ldd + i] = tile[tx][r];
    }
}

int predict_grad_rows_per_block(const cglb_ctx* c) { return input_grad_mid_on(c) ? predict_grad_mid_rows_per_block(c) : 256 * predict_grad_rows_per_lane(c->Dp); }

template <int KIND, int DP, bool HAS_U, bool HAS_W>
static int weighted_grad_pairs(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw,
                               unsigned bx, int64_t jsplit, int64_t jchunk) {
    constexpr int R = predict_grad_rows_per_lane(DP);
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((weighted_grad_kernel<KIND, DP, R, HAS_U, HAS_W, PREC>), dim3(bx, (unsigned)jsplit), dim3(256), 0, c->stream, XhRow,
                                             nrows, Ph, npts, u, Wt, ldw, jchunk, (double*)c->ig_part, (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// XhRow [nrows][Dp] and Ph [npts][Dp]: the two point sets in hot units at the lengthscales ls (host, [D]); variance var.  u: dev [npts] or NULL,
// Wt: dev [npts][ldw] or NULL (one at least).  out_* [nrows], gout_* [nrows][D]: any may be NULL.  gout_w carries the factor wscale; add_u: gout_u
// is added to.  Rows in blocks of PREDICT_GRAD_ROWS.  On a mid-width context under "input_grad_mid" both sets are [.][Dh] and scale_dev, the device copy of
// ks / l_k at ls, carries the gradient constants; every other wide context is refused.
int launch_weighted_grad(cglb_ctx* c, const double* ls, double var, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u,
                         const double* Wt, int64_t ldw, double* out_u, double* gout_u, bool add_u, double* out_w, double* gout_w, double wscale, const double* scale_dev) {
    const bool mid = input_grad_mid_on(c);  // a mid-width context under "input_grad_mid": kernels_predict_grad_mid.hip, block by block
    if (c->dtype != CGLB_F64 || (is_wide(c) && !mid)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the row-weighted gradient product needs an fp64 context of at most 32 input dimensions");
    if ((!u && !Wt) || npts < 1 || (Wt && ldw < nrows) || (!u && (out_u || gout_u)) || (!Wt && (out_w || gout_w)) || (mid && !scale_dev))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad weights, leading dimension or outputs of the row-weighted gradient product");
    if (nrows == 0) return CGLB_OK;
    const RowSlabGradScale gs = mid ? RowSlabGradScale() : row_slab_cross_grad_scale(c, ls, var);
    const int nw = (u ? 1 : 0) + (Wt ? 1 : 0);
    const int R = predict_grad_rows_per_lane(c->Dp);
    for (int k = 0; k < 2; ++k)
        if (!c->pg_ev[k]) HIP_CHECK(c, hipEventCreate(&c->pg_ev[k]));
    c->pg_ev_set = false;
    HIP_CHECK(c, hipEventRecord(c->pg_ev[0], c->stream));
    for (int64_t i0 = 0; i0 < nrows; i0 += PREDICT_GRAD_ROWS) {
        const int64_t nr = std::min<int64_t>(PREDICT_GRAD_ROWS, nrows - i0);
        if (mid) {
            CGLB_TRY(launch_weighted_grad_mid(c, scale_dev, var, XhRow + i0 * c->Dh, nr, Ph, npts, u, Wt ? Wt + i0 : nullptr, ldw, out_u ? out_u + i0 : nullptr,
                                              gout_u ? gout_u + i0 * c->D : nullptr, add_u, out_w ? out_w + i0 : nullptr, gout_w ? gout_w + i0 * c->D : nullptr, wscale));
            continue;
        }
        const int64_t bx = (nr + 256 * R - 1) / (256 * R);
        // capped by the slab of the two-weight instance whatever nw is.  even = false: this product never rounded its chunk to an even length as the
        // other pair kernels do; no reason is on record, kept as measured and tested
        int64_t jsplit = 0, jchunk = 0;
        row_slab_pair_split(c->kff_jsplit, bx, npts, row_slab_slot_cap(nr, 2 * (c->Dp + 1)), false, &jsplit, &jchunk);
        CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nr * nw * (c->Dp + 1) * sizeof(double)));
        const double* xh = XhRow + i0 * c->Dp;
        const double* wt = Wt ? Wt + i0 : nullptr;
        if (u && Wt) { CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((weighted_grad_pairs<KIND, DP, true, true>(c, xh, nr, Ph, npts, u, wt, ldw, (unsigned)bx, jsplit, jchunk))))); }
        else if (u) { CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((weighted_grad_pairs<KIND, DP, true, false>(c, xh, nr, Ph, npts, u, wt, ldw, (unsigned)bx, jsplit, jchunk))))); }
        else { CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((weighted_grad_pairs<KIND, DP, false, true>(c, xh, nr, Ph, npts, u, wt, ldw, (unsigned)bx, jsplit, jchunk))))); }
        PredictGradOut o;
        const int iw = u ? 1 : 0;
        o.out[0] = o.out[1] = o.gout[0] = o.gout[1] = nullptr;
        o.gscale[0] = o.gscale[1] = 1.0;
        if (u) { o.out[0] = out_u ? out_u + i0 : nullptr; o.gout[0] = gout_u ? gout_u + i0 * c->D : nullptr; }
        if (Wt) { o.out[iw] = out_w ? out_w + i0 : nullptr; o.gout[iw] = gout_w ? gout_w + i0 * c->D : nullptr; o.gscale[iw] = wscale; }
        const int64_t total = nr * nw * (c->Dp + 1);
        hipLaunchKernelGGL(weighted_grad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->ig_part, (int)jsplit, nr, nw,
                           c->Dp, c->D, var, gs, o, (int)(add_u && u));
        CGLB_LAUNCH_CHECK(c);
    }
    HIP_CHECK(c, hipEventRecord(c->pg_ev[1], c->stream));
    c->pg_ev_set = true;
    return CGLB_OK;
}

// out [n][Dp] <- x (dev [n][D]) in hot units at the lengthscales ls (host)
int launch_hot_points(cglb_ctx* c, const double* ls, const double* x, int64_t n, double* out) {
    if (n == 0) return CGLB_OK;
    ScaleParams sp;
    const double ks = cglb_kscale(c) * cglb_hot_scale(c);
    for (int d = 0; d < CGLB_MAX_D_NARROW; ++d) {
        sp.center[d] = d < c->D ? c->xmean[d] : 0.0;
        sp.scale[d] = d < c->D ? ks / ls[d] : 0.0;
    }
    hipLaunchKernelGGL(hot_points_kernel, dim3((unsigned)((n * c->Dp + 255) / 256)), dim3(256), 0, c->stream, x, n, c->D, c->Dp, sp, out);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

int launch_transpose(cglb_ctx* c, const double* src, int64_t lds, int64_t rows, int64_t cols, double* dst, int64_t ldd) {
    if (rows == 0 || cols == 0) return CGLB_OK;
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, c->stream, src, lds, rows, cols, dst, ldd);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// "predict_grad_kernel_ms": device time of the pair kernel and slab sums of the last row-weighted gradient product; -1: not this name
int predict_grad_stat(cglb_ctx* c, const char* name, double* value) {
    if (strcmp(name, "predict_grad_kernel_ms")) return -1;
    *value = 0.0;
    if (!c->pg_ev_set) return CGLB_OK;
    float ms = 0.0f;
    HIP_CHECK(c, hipEventSynchronize(c->pg_ev[1]));
    HIP_CHECK(c, hipEventElapsedTime(&ms, c->pg_ev[0], c->pg_ev[1]));
    *value = (double)ms;
    return CGLB_OK;
}
