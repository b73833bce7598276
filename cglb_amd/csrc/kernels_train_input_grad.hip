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
template <int KIND, int DP>
static int train_input_grad_block(cglb_ctx* c, const double* U, const double* V, int s, int64_t row0, int64_t nrows, const RowSlabGradScale& gs, double* gx,
                                  int accumulate) {
    constexpr int R = train_input_grad_rows_per_lane(DP), G = train_input_grad_group_width(DP);
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
            CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((train_input_grad_block<KIND, DP>(c, Ug, Vg, sg, i0, nr, gs, gx, b0 > 0 ? 1 : 0)))));
        }
    }
    return CGLB_OK;
}
