// Value AND input gradient of the two products under the iterative exact-GP class, one evaluation of a pair serving a group of columns:
//   cross (cglb_cross_grad_matmat):    out[i, s] = var sum_j kappa(x*_i, x_j) V[s, j],   gout[i, s, k] = -var sum_j h(x*_i, x_j) (x*_ik - x_jk) / l_k^2 V[s, j]
//   feature (cglb_feature_grad_matmat): out[i, s] = amp sum_j W[s, j] cos(phi_ij),        gout[i, s, k] = -amp sum_j W[s, j] sin(phi_ij) omega_jk / l_k
// with h the radial derivative factor of the lengthscale gradient (devmath.h: hfac_hot_from_d2; d kappa / d x_ik = -h delta_k / l_k) and
// amp = sqrt(2 var / F).  Gradients are with respect to the RAW coordinates of the new point.
//
// Row-slab products (row_slab.h) of cross_multi_kernel's and feature_multi_kernel's operands: a lane keeps the coordinates and R x G x (DP + 1)
// accumulators; the range is split by the kff_jsplit rule (cross) or the feature rule, each capped by the slab [jsplit][nrows][G][DP + 1]; ONE
// finish kernel applies the constants.
// Cross pair: DIRECT differences delta_k = xh*_k - xh_jk in hot units, d2 = sum delta_k^2, kappa and h from that exact d2
// (kappa_hfac_hot_from_d2; always the range-clamped 2^x) - not the Gram chain, whose cancellation error in r would show in h, which is not flat at
// r = 0 for the Matern kinds.  A coincident pair has delta = 0 exactly: it adds exactly zero to the gradient.  Per pair and column: one multiply
// t = h v_s, DP fma acc[s][k] += t delta_k, one fma for the value; 2 DP for the distance.  -var / (l_k hot scale) goes into the finish kernel.
// Feature pair: one phase (DP fma), one range reduction shared by cosine and sine (sincos_turns), then per column one multiply t = sin w_s, DP fma
// acc[s][k] += t omega'_jk with omega' = omega / (2 pi l) of the operand record (a scalar source), one fma for the value; -2 pi amp in the finish.
// (DP + 1) accumulators per (row, column): the group is narrower than 8 at larger widths (input_grad_group_width); groups stay aligned inside the
// interleave blocks of 8, so any ldv that is a multiple of 8 serves (the variance cache as it lies) and the feature records are the existing ones.
// fp64, Dp <= 32.  Register use of every instance: DESIGN.md section 4h.
#include "pair_common.h"
#include "row_slab.h"

#define INPUT_GRAD_ROWS 4096            // new points per launch

// rows per lane and columns per group by padded width: input_grad_rows_per_lane, input_grad_group_width (row_slab.h)

// grid (row blocks of 256 R new points, column chunks of jchunk training points); Vi points at the first column of the group
template <int KIND, int DP, int R, int G, int PREC>
__global__ __launch_bounds__(256) void cross_grad_kernel(const double* __restrict__ XhRow, int64_t nrows, const double* __restrict__ Xh,
                                                         const double* __restrict__ Vi, int64_t ldv, int64_t ncols, int64_t jchunk,
                                                         double* __restrict__ part, const double* __restrict__ exp_tab) {
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double xi[R][DP], acc[R][G][DP + 1];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = row_slab_clamped(rbase, k, nrows);
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[k][d] = XhRow[row * DP + d];
        row_slab_zero(acc[k]);
    }
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < ncols) ? j0 + jchunk : ncols;
    for (int64_t j = j0; j < j1; ++j) {
        const double* __restrict__ cj = Vi + j * ldv;  // wave-uniform: one scalar load of G doubles
        double xj[DP], vj[G];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Xh[j * DP + d];
#pragma unroll
        for (int b = 0; b < G; ++b) vj[b] = cj[b];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double df[DP];  // the difference loop stays written out: as a function of its own it moves the register allocation of all 81 instances
            double d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                df[d] = xi[k][d] - xj[d];
                d2 = __builtin_fma(df[d], df[d], d2);
            }
            double kv, hv;
            kappa_hfac_hot_from_d2<KIND, PREC>(d2, tab, kv, hv);
#pragma unroll
            for (int b = 0; b < G; ++b) row_slab_grad_acc(acc[k][b], hv, kv, vj[b], df);
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) row_slab_store(part, nrows, rbase + (int64_t)k * 256, acc[k]);
}

// grid (row blocks of 256 R rows, feature chunks of jchunk); rec points at the first record of the block of 8 columns, sub at the group inside it
template <int DP, int R, int G>
__global__ __launch_bounds__(256) void feature_grad_kernel(const double* __restrict__ X, int d, RowSlabCentre cen, int64_t nrows,
                                                           const double* __restrict__ rec, int sub, int64_t F, int64_t jchunk, double* __restrict__ part) {
    constexpr int RL = FEATURE_REC(DP);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double z[R][DP], acc[R][G][DP + 1];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = row_slab_clamped(rbase, k, nrows);
#pragma unroll
        for (int q = 0; q < DP; ++q) z[k][q] = q < d ? X[row * d + q] - cen.c[q] : 0.0;
        row_slab_zero(acc[k]);
    }
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < F) ? j0 + jchunk : F;
    for (int64_t j = j0; j < j1; ++j) {
        const double* __restrict__ rj = rec + j * RL;  // wave-uniform: one run of scalar loads
        double om[DP], wj[G];
        const double bj = rj[0];
#pragma unroll
        for (int q = 0; q < DP; ++q) om[q] = rj[1 + q];
#pragma unroll
        for (int b = 0; b < G; ++b) wj[b] = rj[1 + DP + sub + b];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double ph = bj;
#pragma unroll
            for (int q = 0; q < DP; ++q) ph = __builtin_fma(z[k][q], om[q], ph);
            double cv, sv;
            sincos_turns(ph, cv, sv);
#pragma unroll
            for (int b = 0; b < G; ++b) row_slab_grad_acc(acc[k][b], sv, cv, wj[b], om);
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) row_slab_store(part, nrows, rbase + (int64_t)k * 256, acc[k]);
}

// the slabs in fixed order, then the constants: gout[(i * S + b) * d + k] = gs.g[k] * sum_js part[js][i][b][k] (k < d), out[i * ldo + b] = vscale * sum_js
// part[js][i][b][dp] (out may be NULL), b < sg.  out / gout point at the group's first column; one thread per (i, b, k <= dp)
__global__ __launch_bounds__(256) void input_grad_finish_kernel(const double* __restrict__ part, int jsplit, int64_t nrows, int g, int sg, int dp, int d,
                                                                double vscale, RowSlabGradScale gs, double* __restrict__ out, int64_t ldo,
                                                                double* __restrict__ gout, int64_t S) {
    const int64_t per = (int64_t)g * (dp + 1);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * per) return;
    const int64_t i = idx / per;
    const int e = (int)(idx - i * per);
    const int b = e / (dp + 1), k = e - b * (dp + 1);
    if (b >= sg || (k >= d && k < dp) || (k == dp && !out)) return;
    double s = 0.0;
    for (int js = 0; js < jsplit; ++js) s += part[(int64_t)js * nrows * per + idx];
    if (k == dp) out[i * ldo + b] = vscale * s;
    else gout[(i * S + b) * d + k] = gs.g[k] * s;
}

// g_var[i][k] = -2 sum_{s < sp} B[i][s] G[i][s][k] in column order (cglb_itergp_predict_grad): B [nrows][ldb], G [nrows][sp][d]
__global__ __launch_bounds__(256) void input_grad_var_kernel(const double* __restrict__ B, int64_t ldb, const double* __restrict__ G, int64_t nrows, int sp, int d,
                                                             double* __restrict__ g_var) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * d) return;
    const int64_t i = idx / d;
    const int k = (int)(idx - i * d);
    double q = 0.0;
    for (int s = 0; s < sp; ++s) q = __builtin_fma(B[i * ldb + s], G[(i * sp + s) * d + k], q);
    g_var[idx] = -2.0 * q;
}

// f[s][i] = (mean + Gf[i][s]) + KU[i][s],  g[s][i][k] = gf[i][s][k] + gk[i][s][k]  (cglb_itergp_paths_eval with gradients)
__global__ __launch_bounds__(256) void input_grad_paths_kernel(double mean, const double* __restrict__ Gf, const double* __restrict__ KU, const double* __restrict__ gf,
                                                               const double* __restrict__ gk, int64_t n, int S, int d, double* __restrict__ f,
                                                               double* __restrict__ g) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * S * (d + 1)) return;
    const int64_t si = idx / (d + 1);
    const int k = (int)(idx - si * (d + 1));
    const int64_t s = si / n, i = si - s * n;
    if (k == d) f[si] = (mean + Gf[i * S + s]) + KU[i * S + s];
    else g[si * d + k] = gf[(i * S + s) * d + k] + gk[(i * S + s) * d + k];
}

int input_grad_rows_per_block(const cglb_ctx* c) { return 256 * input_grad_rows_per_lane(c->Dp); }
int input_grad_width(const cglb_ctx* c) { return input_grad_group_width(c->Dp); }

static int input_grad_finish(cglb_ctx* c, int64_t jsplit, int64_t nrows, int g, int sg, double vscale, const RowSlabGradScale& gs, double* out, int64_t ldo,
                             double* gout, int64_t S) {
    const int64_t total = nrows * g * (c->Dp + 1);
    hipLaunchKernelGGL(input_grad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->ig_part, (int)jsplit, nrows, g,
                       sg, c->Dp, c->D, vscale, gs, out, ldo, gout, S);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// one group of G columns for the rows (XhRow, nrows <= INPUT_GRAD_ROWS)
template <int KIND, int DP>
static int cross_grad_group(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int sg, const RowSlabGradScale& gs, double* out,
                            int64_t ldo, double* gout, int64_t S) {
    constexpr int R = input_grad_rows_per_lane(DP), G = input_grad_group_width(DP);
    const int64_t ncols = c->N;
    const int64_t bx = (nrows + 256 * R - 1) / (256 * R);
    int64_t jsplit = 0, jchunk = 0;
    row_slab_pair_split(c->kff_jsplit, bx, ncols, row_slab_slot_cap(nrows, G * (DP + 1)), true, &jsplit, &jchunk);
    CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nrows * G * (DP + 1) * sizeof(double)));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((cross_grad_kernel<KIND, DP, R, G, PREC>), dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream, XhRow, nrows,
                                             (const double*)c->Xh, Vi, ldv, ncols, jchunk, (double*)c->ig_part, (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    return input_grad_finish(c, jsplit, nrows, G, sg, c->var, gs, out, ldo, gout, S);
}

// out[i * ldo + s] (out may be NULL) and gout[(i * S + s) * D + k], s < S <= ldv, from Vi: dev [N][ldv] row-major, ldv a multiple of 8, the columns
// S .. ldv - 1 readable.  XhRow: hot-scaled new points.  Rows in blocks of INPUT_GRAD_ROWS, columns in groups of input_grad_group_width.
// A mid-width context with the option "input_grad_mid" goes to kernels_input_grad_mid.hip; XhRow then has input_grad_row_stride(c) = Dh doubles per point.
int launch_cross_grad(cglb_ctx* c, const void* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo, double* gout) {
    if (input_grad_mid_on(c)) return launch_cross_grad_mid(c, XhRow, nrows, Vi, ldv, S, out, ldo, gout);
    if (c->dtype != CGLB_F64 || is_wide(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the input-gradient cross product needs an fp64 context of at most 32 input dimensions");
    if (S < 1 || ldv < S || (ldv % CROSS_MULTI_SP) || !gout || (out && ldo < S))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad column count, leading dimension or output of the input-gradient cross product");
    const RowSlabGradScale gs = row_slab_cross_grad_scale(c, c->ls, c->var);
    const int G = input_grad_group_width(c->Dp);
    for (int64_t i0 = 0; i0 < nrows; i0 += INPUT_GRAD_ROWS) {
        const int64_t nr = std::min<int64_t>(INPUT_GRAD_ROWS, nrows - i0);
        const double* xh = (const double*)XhRow + i0 * c->Dp;
        for (int b0 = 0; b0 < S; b0 += G) {
            const int sg = std::min(G, S - b0);
            CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((cross_grad_group<KIND, DP>(c, xh, nr, Vi + b0, ldv, sg, gs, out ? out + i0 * ldo + b0 : nullptr,
                                                                                                    ldo, gout + (i0 * S + b0) * c->D, S)))));
        }
    }
    return CGLB_OK;
}

template <int DP>
static int feature_grad_group(cglb_ctx* c, const double* X, int64_t nrows, const double* rec, int sub, int64_t F, int64_t jsplit, int64_t jchunk, unsigned bx) {
    constexpr int R = input_grad_rows_per_lane(DP), G = input_grad_group_width(DP);
    hipLaunchKernelGGL((feature_grad_kernel<DP, R, G>), dim3(bx, (unsigned)jsplit), dim3(256), 0, c->stream, X, c->D, row_slab_centre(c), nrows, rec, sub, F,
                       jchunk, (double*)c->ig_part);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// out[i * ldo + s] (out may be NULL) and gout[(i * S + s) * D + k] from the records launch_feature_operand left.  X: dev [nrows][D] raw rows.  The feature
// rule (row_slab_feature_split) at this kernel's rows per block, capped by the slab
int launch_feature_grad(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo, double* gout) {
    if (input_grad_mid_on(c)) return launch_feature_grad_mid(c, X, nrows, F, S, out, ldo, gout);
    if (c->dtype != CGLB_F64 || is_wide(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the input-gradient feature product needs an fp64 context of at most 32 input dimensions");
    if (S < 1 || F < 1 || !gout || (out && ldo < S)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad feature count, column count or output of the input-gradient feature product");
    const int G = input_grad_group_width(c->Dp);
    const double amp = std::sqrt(2.0 * c->var / (double)F);
    RowSlabGradScale gs;
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) gs.g[k] = k < c->D ? -6.283185307179586476925286766559 * amp : 0.0;  // the records hold omega / (2 pi l)
    const int64_t rl = FEATURE_REC(c->Dp);
    const int64_t rb = input_grad_rows_per_block(c);
    for (int64_t i0 = 0; i0 < nrows; i0 += INPUT_GRAD_ROWS) {
        const int64_t nr = std::min<int64_t>(INPUT_GRAD_ROWS, nrows - i0);
        const int64_t bx = (nr + rb - 1) / rb;
        int64_t jsplit = 0, jchunk = 0;
        row_slab_feature_split(rb, nr, F, row_slab_slot_cap(nr, G * (c->Dp + 1)), &jsplit, &jchunk);
        CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nr * G * (c->Dp + 1) * sizeof(double)));
        for (int b0 = 0; b0 < S; b0 += G) {
            const int sg = std::min(G, S - b0);
            const double* rec = c->ft_rec + (int64_t)(b0 / FEATURE_SP) * F * rl;
            CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((feature_grad_group<DP>(c, X + i0 * c->D, nr, rec, b0 % FEATURE_SP, F, jsplit, jchunk, (unsigned)bx))));
            CGLB_TRY(input_grad_finish(c, jsplit, nr, G, sg, amp, gs, out ? out + i0 * ldo + b0 : nullptr, ldo, gout + (i0 * S + b0) * c->D, S));
        }
    }
    return CGLB_OK;
}

int launch_input_grad_var(cglb_ctx* c, const double* B, int64_t ldb, const double* G, int64_t nrows, int sp, double* g_var) {
    if (nrows == 0) return CGLB_OK;
    hipLaunchKernelGGL(input_grad_var_kernel, dim3((unsigned)((nrows * c->D + 255) / 256)), dim3(256), 0, c->stream, B, ldb, G, nrows, sp, c->D, g_var);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

int launch_input_grad_paths(cglb_ctx* c, const double* Gf, const double* KU, const double* gf, const double* gk, int64_t n, int S, double* f, double* g) {
    const int64_t total = n * S * (c->D + 1);
    if (total == 0) return CGLB_OK;
    hipLaunchKernelGGL(input_grad_paths_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->mean, Gf, KU, gf, gk, n, S, c->D, f, g);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}
