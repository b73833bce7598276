// Value AND input gradient of the two products under the iterative exact-GP class, one evaluation of a pair serving a group of columns:
//   cross (cglb_cross_grad_matmat):    out[i, s] = var sum_j kappa(x*_i, x_j) V[s, j],   gout[i, s, k] = -var sum_j h(x*_i, x_j) (x*_ik - x_jk) / l_k^2 V[s, j]
//   feature (cglb_feature_grad_matmat): out[i, s] = amp sum_j W[s, j] cos(phi_ij),        gout[i, s, k] = -amp sum_j W[s, j] sin(phi_ij) omega_jk / l_k
// with h the radial derivative factor of the lengthscale gradient (devmath.h: hfac_hot_from_d2; d kappa / d x_ik = -h delta_k / l_k) and
// amp = sqrt(2 var / F).  Gradients are with respect to the RAW coordinates of the new point.
//
// The decomposition is that of cross_multi_kernel / feature_multi_kernel: a lane owns R new points (coordinates and R x G x (DP + 1) accumulators in
// VGPRs for the whole launch); the training point (feature) and its G column values are wave-uniform and arrive by scalar loads; the column
// range is split over blockIdx.y (the kff_jsplit rule for the cross product, the feature product's chunk rule for the other); partial sums go
// to a slab [jsplit][nrows][G][DP + 1] that exactly one workgroup writes, and ONE finish kernel adds the slabs in fixed order and applies the
// constants: no atomics, bitwise repeatable.
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

#define INPUT_GRAD_SLOTS 256            // most column chunks of one launch
#define INPUT_GRAD_ROWS 4096            // new points per launch
#define INPUT_GRAD_SLAB (1 << 24)       // doubles of the slab of one launch (128 MiB): caps the chunk count
#define INPUT_GRAD_REC_SP 8             // columns per feature record / interleave block (FEATURE_SP, CROSS_MULTI_SP)
#define INPUT_GRAD_FEATURE_MIN_CHUNK 64 // as FEATURE_MIN_CHUNK
#define INPUT_GRAD_FEATURE_TARGET_WG 2048
#define INPUT_GRAD_FEATURE_REC(dp) (((dp) + 1 + INPUT_GRAD_REC_SP + 1) & ~1)  // FEATURE_REC of kernels_feature_multi.hip

// rows per lane and columns per group by padded width, chosen so that R (DP + G (DP + 1)) + DP row-resident doubles stay near 100 (200 of the 256
// VGPRs of two waves per SIMD): 2 x 8 up to width 4 (88 + 4), 1 x 8 up to 8 (80 + 8), 1 x 4 up to 16 (84 + 16), 1 x 2 beyond (98 + 32)
static constexpr int input_grad_rows_per_lane(int dp) { return dp <= 4 ? 2 : 1; }
static constexpr int input_grad_group_width(int dp) { return dp <= 8 ? 8 : (dp <= 16 ? 4 : 2); }

struct InputGradScale { double g[CGLB_MAX_D_NARROW]; };  // constant of gradient component k

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
        int64_t row = rbase + (int64_t)k * 256;
        row = row < nrows ? row : nrows - 1;
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[k][d] = XhRow[row * DP + d];
#pragma unroll
        for (int b = 0; b < G; ++b)
#pragma unroll
            for (int d = 0; d <= DP; ++d) acc[k][b][d] = 0.0;
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
            double df[DP];
            double d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                df[d] = xi[k][d] - xj[d];
                d2 = __builtin_fma(df[d], df[d], d2);
            }
            double kv, hv;
            kappa_hfac_hot_from_d2<KIND, PREC>(d2, tab, kv, hv);
#pragma unroll
            for (int b = 0; b < G; ++b) {
                const double t = hv * vj[b];
#pragma unroll
                for (int d = 0; d < DP; ++d) acc[k][b][d] = __builtin_fma(t, df[d], acc[k][b][d]);
                acc[k][b][DP] = __builtin_fma(kv, vj[b], acc[k][b][DP]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = rbase + (int64_t)k * 256;
        if (row < nrows) {
            double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (G * (DP + 1));
#pragma unroll
            for (int b = 0; b < G; ++b)
#pragma unroll
                for (int d = 0; d <= DP; ++d) o[b * (DP + 1) + d] = acc[k][b][d];
        }
    }
}

struct InputGradCentre { double c[CGLB_MAX_D_NARROW]; };

// grid (row blocks of 256 R rows, feature chunks of jchunk); rec points at the first record of the block of 8 columns, sub at the group inside it
template <int DP, int R, int G>
__global__ __launch_bounds__(256) void feature_grad_kernel(const double* __restrict__ X, int d, InputGradCentre cen, int64_t nrows,
                                                           const double* __restrict__ rec, int sub, int64_t F, int64_t jchunk, double* __restrict__ part) {
    constexpr int RL = INPUT_GRAD_FEATURE_REC(DP);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double z[R][DP], acc[R][G][DP + 1];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        int64_t row = rbase + (int64_t)k * 256;
        row = row < nrows ? row : nrows - 1;
#pragma unroll
        for (int q = 0; q < DP; ++q) z[k][q] = q < d ? X[row * d + q] - cen.c[q] : 0.0;
#pragma unroll
        for (int b = 0; b < G; ++b)
#pragma unroll
            for (int q = 0; q <= DP; ++q) acc[k][b][q] = 0.0;
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
            for (int b = 0; b < G; ++b) {
                const double t = sv * wj[b];
#pragma unroll
                for (int q = 0; q < DP; ++q) acc[k][b][q] = __builtin_fma(t, om[q], acc[k][b][q]);
                acc[k][b][DP] = __builtin_fma(cv, wj[b], acc[k][b][DP]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = rbase + (int64_t)k * 256;
        if (row < nrows) {
            double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (G * (DP + 1));
#pragma unroll
            for (int b = 0; b < G; ++b)
#pragma unroll
                for (int q = 0; q <= DP; ++q) o[b * (DP + 1) + q] = acc[k][b][q];
        }
    }
}

// the slabs in fixed order, then the constants: gout[(i * S + b) * d + k] = gs.g[k] * sum_js part[js][i][b][k] (k < d), out[i * ldo + b] = vscale * sum_js
// part[js][i][b][dp] (out may be NULL), b < sg.  out / gout point at the group's first column; one thread per (i, b, k <= dp)
__global__ __launch_bounds__(256) void input_grad_finish_kernel(const double* __restrict__ part, int jsplit, int64_t nrows, int g, int sg, int dp, int d,
                                                                double vscale, InputGradScale gs, double* __restrict__ out, int64_t ldo,
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

static int64_t input_grad_slot_cap(int64_t nrows, int g, int dp) {
    const int64_t cap = (int64_t)INPUT_GRAD_SLAB / (nrows * g * (dp + 1));
    return std::max<int64_t>(1, std::min<int64_t>(INPUT_GRAD_SLOTS, cap));
}

static int input_grad_finish(cglb_ctx* c, int64_t jsplit, int64_t nrows, int g, int sg, double vscale, const InputGradScale& gs, double* out, int64_t ldo,
                             double* gout, int64_t S) {
    const int64_t total = nrows * g * (c->Dp + 1);
    hipLaunchKernelGGL(input_grad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->ig_part, (int)jsplit, nrows, g,
                       sg, c->Dp, c->D, vscale, gs, out, ldo, gout, S);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// one group of G columns for the rows (XhRow, nrows <= INPUT_GRAD_ROWS)
template <int KIND, int DP>
static int cross_grad_group(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int sg, const InputGradScale& gs, double* out,
                            int64_t ldo, double* gout, int64_t S) {
    constexpr int R = input_grad_rows_per_lane(DP), G = input_grad_group_width(DP);
    const int64_t ncols = c->N;
    const int64_t bx = (nrows + 256 * R - 1) / (256 * R);
    // the column split of the plain kernel (kernels_kff.hip: kff_pairs_range), capped by the slab
    int64_t jsplit = c->kff_jsplit > 0 ? c->kff_jsplit : (8192 + bx - 1) / bx;
    jsplit = std::min(jsplit, input_grad_slot_cap(nrows, G, DP));
    if (jsplit > (ncols + 63) / 64) jsplit = (ncols + 63) / 64;
    if (jsplit < 1) jsplit = 1;
    int64_t jchunk = (ncols + jsplit - 1) / jsplit;
    jchunk = (jchunk + 1) & ~(int64_t)1;
    jsplit = (ncols + jchunk - 1) / jchunk;
    CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nrows * G * (DP + 1) * sizeof(double)));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((cross_grad_kernel<KIND, DP, R, G, PREC>), dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream, XhRow, nrows,
                                             (const double*)c->Xh, Vi, ldv, ncols, jchunk, (double*)c->ig_part, (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    return input_grad_finish(c, jsplit, nrows, G, sg, c->var, gs, out, ldo, gout, S);
}

// out[i * ldo + s] (out may be NULL) and gout[(i * S + s) * D + k], s < S <= ldv, from Vi: dev [N][ldv] row-major, ldv a multiple of 8, the columns
// S .. ldv - 1 readable.  XhRow: hot-scaled new points.  Rows in blocks of INPUT_GRAD_ROWS, columns in groups of input_grad_group_width.
int launch_cross_grad(cglb_ctx* c, const void* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo, double* gout) {
    if (c->dtype != CGLB_F64 || is_wide(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the input-gradient cross product needs an fp64 context of at most 32 input dimensions");
    if (S < 1 || ldv < S || (ldv % INPUT_GRAD_REC_SP) || !gout || (out && ldo < S))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad column count, leading dimension or output of the input-gradient cross product");
    InputGradScale gs;
    const double ks = cglb_kscale(c) * cglb_hot_scale(c);  // delta_hot = ks (x*_k - x_jk) / l_k
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) gs.g[k] = k < c->D ? -c->var / (c->ls[k] * ks) : 0.0;
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
    InputGradCentre cen;
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) cen.c[k] = k < c->D ? c->xmean[k] : 0.0;
    hipLaunchKernelGGL((feature_grad_kernel<DP, R, G>), dim3(bx, (unsigned)jsplit), dim3(256), 0, c->stream, X, c->D, cen, nrows, rec, sub, F, jchunk,
                       (double*)c->ig_part);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// out[i * ldo + s] (out may be NULL) and gout[(i * S + s) * D + k] from the records launch_feature_operand left.  X: dev [nrows][D] raw rows.  The chunk
// rule of feature_split at this kernel's rows per block, capped by the slab
int launch_feature_grad(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo, double* gout) {
    if (c->dtype != CGLB_F64 || is_wide(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the input-gradient feature product needs an fp64 context of at most 32 input dimensions");
    if (S < 1 || F < 1 || !gout || (out && ldo < S)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad feature count, column count or output of the input-gradient feature product");
    const int G = input_grad_group_width(c->Dp);
    const double amp = std::sqrt(2.0 * c->var / (double)F);
    InputGradScale gs;
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) gs.g[k] = k < c->D ? -6.283185307179586476925286766559 * amp : 0.0;  // the records hold omega / (2 pi l)
    const int64_t rl = INPUT_GRAD_FEATURE_REC(c->Dp);
    const int64_t rb = input_grad_rows_per_block(c);
    for (int64_t i0 = 0; i0 < nrows; i0 += INPUT_GRAD_ROWS) {
        const int64_t nr = std::min<int64_t>(INPUT_GRAD_ROWS, nrows - i0);
        const int64_t bx = (nr + rb - 1) / rb;
        int64_t jsplit = (INPUT_GRAD_FEATURE_TARGET_WG + bx - 1) / bx;
        jsplit = std::min(jsplit, input_grad_slot_cap(nr, G, c->Dp));
        if (jsplit > (F + INPUT_GRAD_FEATURE_MIN_CHUNK - 1) / INPUT_GRAD_FEATURE_MIN_CHUNK) jsplit = (F + INPUT_GRAD_FEATURE_MIN_CHUNK - 1) / INPUT_GRAD_FEATURE_MIN_CHUNK;
        if (jsplit < 1) jsplit = 1;
        const int64_t jchunk = (F + jsplit - 1) / jsplit;
        jsplit = (F + jchunk - 1) / jchunk;
        CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nr * G * (c->Dp + 1) * sizeof(double)));
        for (int b0 = 0; b0 < S; b0 += G) {
            const int sg = std::min(G, S - b0);
            const double* rec = c->ft_rec + (int64_t)(b0 / INPUT_GRAD_REC_SP) * F * rl;
            CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((feature_grad_group<DP>(c, X + i0 * c->D, nr, rec, b0 % INPUT_GRAD_REC_SP, F, jsplit, jchunk, (unsigned)bx))));
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
