// The pair-weighted gradient of a sum of bilinear forms over K_ff with respect to the TRAINING inputs (cglb_grad_x_kff_multi; the input gradient of
// cglb_itergp_objective_and_grad_x):
//   gx[i, k] = sum_j w_ij d kappa(x_i, x_j) / d x_ik = -var sum_j w_ij h_ij delta_ijk / l_k,   w_ij = sum_b (u_bi v_bj + v_bi u_bj),  b < S
// with h the radial derivative factor (devmath.h: d kappa / d x_ik = -h delta_k / l_k, delta_k = (x_ik - x_jk) / l_k), U and V the left and right vectors
// of launch_grad_kff_multi.  Gradients are with respect to the RAW coordinates.  sum_i x_ik gx[i, k] = -l_k out[k] of launch_grad_kff_multi on the same
// pairs, and sum_i gx[i, k] = 0, both to round-off.
//
// A row-slab product (row_slab.h): a lane keeps R rows - x_i in hot units, u_bi and v_bi of one group of G pairs, DP accumulators each - for the whole
// launch; training point j is wave-uniform: x_j from the hot operand set and the group's 2 G values (u_.j | v_.j), ONE contiguous record per point
// (grad_pass.h: grad_multi_operand_kernel, zero padded), arrive by scalar loads.  The range of j is split by the kff_jsplit rule (row_slab_pair_split),
// capped by the slab part[jsplit][nrows][DP]; ONE finish kernel adds the slabs in fixed order and applies -var / (l_k hot scale).  S > G runs in groups
// of G whose results are added in group order by the finish kernel.  No atomics; two calls give bitwise equal results.
// Pair: DIRECT differences in hot units and kappa_hfac_hot_from_d2 (always the range-clamped 2^x) for h - the value is not needed and is not formed -
// as cross_grad_kernel and for its reason; a coincident pair (i = j, a duplicated row) has delta = 0 exactly and adds exactly zero.  Per pair: 2 DP for
// the distance, the profile, 2 G fmas for w_ij, one multiply t = h w, DP fmas acc[k] += t delta_k.
// The FULL square is swept: every unordered pair is evaluated twice, once from each of its rows.  (A symmetric sweep would owe the column its share,
// DP cross-lane sums per column: DESIGN.md section 4j, open.)
// fp64, one rank, Dp <= 32.  Rows per lane and pairs per group by padded width: train_input_grad_rows_per_lane, train_input_grad_group_width
// (row_slab.h).  Register use of every instance: DESIGN.md section 4j.
// Further down, for the CGLB / SGPR bounds (cglb_objective_and_grad_x): the single-pair instance of this kernel (launch_grad_x_kff_pair) and the
// transposed panel pass over the K_uf adjoint (grad_x_kuf_kernel, launch_grad_x_kuf), which share the finish kernel.
#include "grad_pass.h"
#include "row_slab.h"

#define TRAIN_INPUT_GRAD_ROWS 4096      // rows per launch

// grid (row blocks of 256 R rows of the launch's nrows rows starting at row0, column chunks of jchunk training points); U, V: [s][n] row side;
// UVi: [n][2 G] column side
template <int KIND, int DP, int R, int G, int PREC>
__global__ __launch_bounds__(256) void train_input_grad_kernel(const double* __restrict__ Xh, const double* __restrict__ U, const double* __restrict__ V, int s,
                                                               const double* __restrict__ UVi, int64_t n, int64_t row0, int64_t nrows, int64_t jchunk,
                                                               double* __restrict__ part, const double* __restrict__ exp_tab) {
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double xi[R][DP], ui[R][G], vi[R][G], acc[R][DP];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = row0 + row_slab_clamped(rbase, k, nrows);
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[k][d] = Xh[row * DP + d];
#pragma unroll
        for (int b = 0; b < G; ++b) {  // padded pairs carry zero weight
            ui[k][b] = b < s ? U[(int64_t)b * n + row] : 0.0;
            vi[k][b] = b < s ? V[(int64_t)b * n + row] : 0.0;
        }
        row_slab_zero(acc[k]);
    }
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < n) ? j0 + jchunk : n;
    for (int64_t j = j0; j < j1; ++j) {
        const double* __restrict__ cj = UVi + j * (2 * G);  // wave-uniform: one scalar load of 2 G doubles
        double xj[DP], uj[G], vj[G];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Xh[j * DP + d];
#pragma unroll
        for (int b = 0; b < G; ++b) {
            uj[b] = cj[b];
            vj[b] = cj[G + b];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double df[DP];  // written out, as cross_grad_kernel keeps it
            double d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                df[d] = xi[k][d] - xj[d];
                d2 = __builtin_fma(df[d], df[d], d2);
            }
            double w = ui[k][0] * vj[0];
#pragma unroll
            for (int b = 1; b < G; ++b) w = __builtin_fma(ui[k][b], vj[b], w);
#pragma unroll
            for (int b = 0; b < G; ++b) w = __builtin_fma(vi[k][b], uj[b], w);
            double kv, hv;
            kappa_hfac_hot_from_d2<KIND, PREC>(d2, tab, kv, hv);
            const double t = hv * w;
#pragma unroll
            for (int d = 0; d < DP; ++d) acc[k][d] = __builtin_fma(t, df[d], acc[k][d]);
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) row_slab_store(part, nrows, rbase + (int64_t)k * 256, acc[k]);
}

// the slabs in fixed order, then the constants: gx[i * d + k] (+)= gs.g[k] * sum_js part[js][i][k], k < d; one thread per (i, k < dp)
__global__ __launch_bounds__(256) void train_input_grad_finish_kernel(const double* __restrict__ part, int jsplit, int64_t nrows, int dp, int d, RowSlabGradScale gs,
                                                                      double* __restrict__ gx, int accumulate) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * dp) return;
    const int64_t i = idx / dp;
    const int k = (int)(idx - i * dp);
    if (k >= d) return;
    double s = 0.0;
    for (int js = 0; js < jsplit; ++js) s += part[(int64_t)js * nrows * dp + idx];
    const double g = gs.g[k] * s;
    gx[i * d + k] = accumulate ? gx[i * d + k] + g : g;
}

// one group of s <= G pairs for the rows [row0, row0 + nrows), nrows <= TRAIN_INPUT_GRAD_ROWS; the group's records are in c->gm_uv
template <int KIND, int DP, int R, int G>
static int train_input_grad_block(cglb_ctx* c, const double* U, const double* V, int s, int64_t row0, int64_t nrows, const RowSlabGradScale& gs, double* gx,
                                  int accumulate) {
    const int64_t n = c->N;
    const int64_t bx = (nrows + 256 * R - 1) / (256 * R);
    int64_t jsplit = 0, jchunk = 0;
    row_slab_pair_split(c->kff_jsplit, bx, n, row_slab_slot_cap(nrows, DP), true, &jsplit, &jchunk);
    CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nrows * DP * sizeof(double)));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((train_input_grad_kernel<KIND, DP, R, G, PREC>), dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream,
                                             (const double*)c->Xh, U, V, s, (const double*)c->gm_uv, n, row0, nrows, jchunk, (double*)c->ig_part,
                                             (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(train_input_grad_finish_kernel, dim3((unsigned)((nrows * DP + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->ig_part, (int)jsplit,
                       nrows, DP, c->D, gs, gx + row0 * c->D, accumulate);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

int train_input_grad_rows_per_block(const cglb_ctx* c) { return 256 * train_input_grad_rows_per_lane(c->Dp); }
int train_input_grad_width(const cglb_ctx* c) { return train_input_grad_group_width(c->Dp); }

// the scope of the pass: fp64, at most 32 input dimensions, one rank, one shard covering all rows
bool train_input_grad_native(const cglb_ctx* c) {
    return c->dtype == CGLB_F64 && !is_wide(c) && c->par_world == 1 && !c->comm && c->r0 == 0 && c->r1 == c->N;
}

// gx (dev [N][D], k fastest, overwritten) from U, V: dev [S][N], pair b contiguous, at the hyper-parameters of the last set_hypers.  Groups of
// train_input_grad_group_width pairs in pair order, rows in blocks of TRAIN_INPUT_GRAD_ROWS
int launch_grad_x_kff_multi(cglb_ctx* c, const void* U, const void* V, int S, double* gx) {
    if (!train_input_grad_native(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient pass has no wide path yet: it needs an fp64 context of at most 32 input dimensions on one rank");
    if (S < 1 || !gx) return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad pair count or output of the training-input gradient pass");
    const RowSlabGradScale gs = row_slab_cross_grad_scale(c, c->ls, c->var);
    const int G = train_input_grad_group_width(c->Dp);
    for (int b0 = 0; b0 < S; b0 += G) {
        const int sg = std::min(G, S - b0);
        const double* Ug = (const double*)U + (size_t)b0 * c->N;
        const double* Vg = (const double*)V + (size_t)b0 * c->N;
        CGLB_TRY(grad_multi_operands(c, Ug, Vg, sg, G, nullptr));
        for (int64_t i0 = 0; i0 < c->N; i0 += TRAIN_INPUT_GRAD_ROWS) {
            const int64_t nr = std::min<int64_t>(TRAIN_INPUT_GRAD_ROWS, c->N - i0);
            CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((train_input_grad_block<KIND, DP, train_input_grad_rows_per_lane(DP),
                                                                                                   train_input_grad_group_width(DP)>(c, Ug, Vg, sg, i0, nr, gs, gx, b0 > 0 ? 1 : 0)))));
        }
    }
    return CGLB_OK;
}

// ---- the single-pair instance (cglb_grad_x_kff_pair; the K_ff term of cglb_objective_and_grad_x) ----
// The same kernel at G = 1: the record of a training point is (u_j, v_j), the weight two products, and the 2 G - 2 doubles per row this frees go to
// more rows per lane (train_input_grad_pair_rows_per_lane), so x_j and its record are fetched once for twice as many pairs.  Rows per launch grow with
// the rows per lane, so that a launch keeps the workgroup count of the G-wide pass.  launch_grad_x_kff_multi is not routed here: its S = 1 results stay
// bitwise what they are (another R is another summation order over the chunks).
static constexpr int train_input_grad_pair_launch_rows(int dp) { return TRAIN_INPUT_GRAD_ROWS * (train_input_grad_pair_rows_per_lane(dp) > 2 ? 2 : 1); }

int train_input_grad_pair_rows_per_block(const cglb_ctx* c) { return 256 * train_input_grad_pair_rows_per_lane(c->Dp); }

int launch_grad_x_kff_pair(cglb_ctx* c, const void* u, const void* v, double* gx, int accumulate) {
    if (!train_input_grad_native(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient pass has no wide path yet: it needs an fp64 context of at most 32 input dimensions on one rank");
    if (!u || !v || !gx) return cglb_fail(c, CGLB_ERR_BAD_ARG, "NULL operand or output of the single-pair training-input gradient pass");
    const RowSlabGradScale gs = row_slab_cross_grad_scale(c, c->ls, c->var);
    CGLB_TRY(grad_multi_operands(c, (const double*)u, (const double*)v, 1, 1, nullptr));
    CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, {
        constexpr int64_t rows = train_input_grad_pair_launch_rows(DP);
        for (int64_t i0 = 0; i0 < c->N; i0 += rows) {
            const int64_t nr = std::min<int64_t>(rows, c->N - i0);
            CGLB_TRY((train_input_grad_block<KIND, DP, train_input_grad_pair_rows_per_lane(DP), 1>(c, (const double*)u, (const double*)v, 1, i0, nr, gs, gx, accumulate)));
        }
    }));
    return CGLB_OK;
}

// ---- the transposed panel pass (cglb_grad_x_kuf; the K_uf terms of cglb_objective_and_grad_x) ----
//   gx[n, k] = sum_m (G[m, n] + c_m w_n) d k(z_m, x_n) / d x_nk = +var sum_m (G[m, n] + c_m w_n) h_mn delta_mnk / (l_k ks),   delta = z_m - x_n in scaled units
// the reduction over m of the panel whose reduction over n grad_panel_kernel (kernels_grad.hip) forms for dZ and dl: the same operand sets (Zs, Xs:
// plain scaled units), the same direct differences z - x and the same evaluator (kappa_from_d2 / hfac_from_d2), so dZ and dX differentiate ONE
// function; the constant has the sign opposite to dZ.  A row-slab product: a lane keeps R training points (x_n, w_n, DP accumulators each) for the
// launch; the inducing point is wave-uniform (z_m and c_m by scalar loads); G[m * ldg + n] is ONE coalesced streaming load per lane and row.  The
// range of m is split by row_slab_panel_split (forced: option "kuf_msplit"), slab part[msplit][N][DP], added in fixed order by
// train_input_grad_finish_kernel.  No atomics; a coincident pair x_n = z_m has delta = 0 exactly and adds exactly zero.
// grid (row blocks of 256 R training points, chunks of mchunk inducing points)
template <int KIND, int DP, int R>
__global__ __launch_bounds__(256) void grad_x_kuf_kernel(const double* __restrict__ G, int64_t ldg, const double* __restrict__ cvec, const double* __restrict__ wvec,
                                                         const double* __restrict__ Zs, const double* __restrict__ Xs, int64_t n, int M, int mchunk,
                                                         double* __restrict__ part) {
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double xn[R][DP], wn[R], acc[R][DP];
    int64_t rows[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        rows[k] = row_slab_clamped(rbase, k, n);
#pragma unroll
        for (int d = 0; d < DP; ++d) xn[k][d] = Xs[rows[k] * DP + d];
        wn[k] = wvec ? wvec[rows[k]] : 0.0;
        row_slab_zero(acc[k]);
    }
    const int m0 = (int)blockIdx.y * mchunk;
    const int m1 = (m0 + mchunk < M) ? m0 + mchunk : M;
    for (int m = m0; m < m1; ++m) {
        double z[DP];  // wave-uniform
#pragma unroll
        for (int d = 0; d < DP; ++d) z[d] = Zs[(int64_t)m * DP + d];
        const double cm = cvec ? cvec[m] : 0.0;
        const double* __restrict__ Gm = G + (int64_t)m * ldg;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double g = CGLB_STREAM_LOAD(Gm + rows[k]);
            if (cvec) g = __builtin_fma(cm, wn[k], g);
            double df[DP], d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                df[d] = z[d] - xn[k][d];
                d2 = __builtin_fma(df[d], df[d], d2);
            }
            const double h = (KIND == CGLB_RBF) ? kappa_from_d2<double, KIND>(d2) : hfac_from_d2<double, KIND>(d2);  // as grad_panel_kernel
            const double t = g * h;
#pragma unroll
            for (int d = 0; d < DP; ++d) acc[k][d] = __builtin_fma(t, df[d], acc[k][d]);
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) row_slab_store(part, n, rbase + (int64_t)k * 256, acc[k]);
}

int grad_x_kuf_rows_per_block(const cglb_ctx* c) { return 256 * grad_x_kuf_rows_per_lane(c->Dp); }

template <int KIND, int DP>
static int grad_x_kuf_launch(cglb_ctx* c, const double* G, int64_t ldg, const double* cvec, const double* wvec, const RowSlabGradScale& gs, double* gx) {
    constexpr int R = grad_x_kuf_rows_per_lane(DP);
    const int64_t n = c->N;
    const int64_t bx = (n + 256 * R - 1) / (256 * R);
    int64_t msplit = 0, mchunk = 0;
    row_slab_panel_split(c->kuf_msplit, bx, c->M, row_slab_slot_cap(n, DP), &msplit, &mchunk);
    CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)msplit * n * DP * sizeof(double)));
    hipLaunchKernelGGL((grad_x_kuf_kernel<KIND, DP, R>), dim3((unsigned)bx, (unsigned)msplit), dim3(256), 0, c->stream, G, ldg, cvec, wvec, (const double*)c->Zs,
                       (const double*)c->Xs, n, c->M, (int)mchunk, (double*)c->ig_part);
    CGLB_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(train_input_grad_finish_kernel, dim3((unsigned)((n * DP + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->ig_part, (int)msplit, n, DP,
                       c->D, gs, gx, 0);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

int launch_grad_x_kuf(cglb_ctx* c, const void* G, int64_t ldg, const void* cvec, const void* wvec, double* gx) {
    if (!train_input_grad_native(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the transposed panel pass has no wide path yet: it needs an fp64 context of at most 32 input dimensions on one rank");
    if (!G || !gx || ldg < c->N || (cvec == nullptr) != (wvec == nullptr))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the transposed panel pass needs a panel with ldg >= N, an output, and cvec and wvec both set or both NULL");
    RowSlabGradScale gs;  // +var / (l_k ks) in plain scaled units: the sign opposite to dZ (grad_panel_finalize_kernel)
    const double ks = cglb_kscale(c);
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) gs.g[k] = k < c->D ? c->var / (c->ls[k] * ks) : 0.0;
    CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((grad_x_kuf_launch<KIND, DP>(c, (const double*)G, ldg, (const double*)cvec, (const double*)wvec, gs, gx)))));
    return CGLB_OK;
}
