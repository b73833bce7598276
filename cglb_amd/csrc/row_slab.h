// The row-slab products: the plain pair kernel behind launch_cross_matvec (kernels_kff.hip), the multi-column cross product
// (kernels_cross_multi.hip), the random-feature product (kernels_feature_multi.hip), their two value-and-gradient forms (kernels_input_grad.hip)
// and the row-weighted gradient product (kernels_predict_grad.hip).  One decomposition:
//   * a lane owns R rows (new points): their coordinates and R x G x W accumulators stay in VGPRs for the whole launch (G columns or weight slots,
//     W = 1 value or DP gradient components + 1 value);
//   * the other operand (training point, feature, inducing point) is wave-uniform and arrives by scalar loads;
//   * its range is split over blockIdx.y in chunks of jchunk (row_slab_pair_split, row_slab_feature_split: host, below);
//   * workgroup (blockIdx.x, blockIdx.y) alone writes its partial sums to the slab part[blockIdx.y][row][G * W];
//   * a finish kernel adds the slabs in fixed order and applies the constants: no atomics, bitwise repeatable.
// What the kernels differ in stays in each of them: the pair evaluation (Gram chain and kappa_hot_*, kappa_hfac_hot_from_d2, cos_turns /
// sincos_turns), the weight prefetch of weighted_grad_kernel, the batches of the looping feature kernel.  Every array below is indexed
// statically after unrolling.  As pair_common.h: a kernel whose register allocation or schedule moves when it calls one of the device pieces
// keeps that piece written out and says so at the place.
#pragma once
#include <algorithm>

#include "devmath.h"
#include "dispatch.h"

// ---- layouts the files share ----
#ifndef CROSS_MULTI_SP
#define CROSS_MULTI_SP 8          // columns per group / interleave block of the cross product: the one instantiated width (16 was tried as a variant build: DESIGN.md section 4f)
#endif
#define FEATURE_SP 8              // columns per group / operand record of the feature product
#define FEATURE_REC(dp) (((dp) + 1 + FEATURE_SP + 1) & ~1)  // doubles per record { b_j | omega_j[dp] | W[8 g .. 8 g + 7, j] }, even: every record starts 16-byte aligned
#define FEATURE_MIN_CHUNK 64      // fewest features of a chunk (but the last): below it the slab traffic outweighs the accumulators a workgroup keeps
#define FEATURE_TARGET_WG 2048    // workgroups a feature launch aims at: 8 per CU
#define ROW_SLAB_SLOTS 256        // most chunks of one launch of the multi-column, feature and gradient products
#define ROW_SLAB_GRAD_DOUBLES (1 << 24)  // doubles of the slab of one gradient launch (128 MiB): caps the chunk count

// ---- geometry of the value-and-gradient products by padded width (mirrored by tests/input_grad_ref.py and tests/input_grad_mid_ref.py) ----
// Narrow (kernels_input_grad.hip): rows per lane and columns per group, chosen so that R (DP + G (DP + 1)) + DP row-resident doubles stay near 100
// (200 of the 256 VGPRs of two waves per SIMD): 2 x 8 up to width 4 (88 + 4), 1 x 8 up to 8 (80 + 8), 1 x 4 up to 16 (84 + 16), 1 x 2 beyond (98 + 32)
static constexpr int input_grad_rows_per_lane(int dp) { return dp <= 4 ? 2 : 1; }
static constexpr int input_grad_group_width(int dp) { return dp <= 8 ? 8 : (dp <= 16 ? 4 : 2); }
// The pair-weighted training-input gradient (kernels_train_input_grad.hip; mirrored by tests/train_input_grad_ref.py): rows per lane and vector pairs per
// group.  The column side is wave-uniform, 2 DP + 4 G SGPRs (x_j and the record u_.j | v_.j) of the 102 a wave has: 80 at width 32 with G = 4 (G = 8
// would need 96 and leave none for addresses and the loop), 64 at width 16 with G = 8.  Row-resident doubles R (2 DP + 2 G) + DP (coordinates,
// accumulators, both row-side vectors, the differences in flight): 2 x 8 up to width 8 (72 at 8), 1 x 8 up to 16 (64), 1 x 4 beyond (104 at 32)
static constexpr int train_input_grad_rows_per_lane(int dp) { return dp <= 8 ? 2 : 1; }
static constexpr int train_input_grad_group_width(int dp) { return dp <= 16 ? 8 : 4; }
// The single-pair instance of that kernel (G = 1: cglb_grad_x_kff_pair, the K_ff term of cglb_objective_and_grad_x; mirrored by
// tests/bound_input_grad_ref.py): the two row-side vectors shrink from 2 G to 2 doubles per row, which pays for more rows per lane.  Row-resident
// doubles R (2 DP + 2) + DP: 4 rows up to width 8 (80 at 8), 2 up to 16 (84), 1 beyond (98 at 32); 2 DP + 2 SGPR pairs on the column side
static constexpr int train_input_grad_pair_rows_per_lane(int dp) { return dp <= 8 ? 4 : (dp <= 16 ? 2 : 1); }
// The transposed panel pass (kernels_bound_input_grad.hip: grad_x_kuf_kernel; mirrored by tests/bound_input_grad_ref.py): a lane owns R training points,
// R (2 DP + 1) + DP row-resident doubles (coordinates, accumulators, w_n, the differences in flight) and R panel loads in flight per inducing point:
// 2 rows up to width 8 (42 at 8), 1 beyond (97 at 32).  The pass streams the panel once: more rows per lane buy nothing once the loads overlap
static constexpr int grad_x_kuf_rows_per_lane(int dp) { return dp <= 8 ? 2 : 1; }
#define GRAD_X_KUF_TARGET_WG 2048  // workgroups a launch of the transposed panel pass aims at: 8 per CU
#define GRAD_X_KUF_MIN_CHUNK 16    // the rule makes at most ceil(M / 16) chunks: more than 8 inducing points each
// Mid widths (kernels_input_grad_mid.hip, hot width dh in 48, 64, 80, 96): a new point is shared by SPLIT lanes of HD = dh / SPLIT coordinates each;
// (2 + G) HD + G row-resident doubles per lane (coordinates, differences, G x HD gradient sums, G values): 76, 100, 82, 98.  256 / SPLIT rows per workgroup
static constexpr int input_grad_mid_split(int dh) { return dh > 0 ? 4 : 0; }
static constexpr int input_grad_mid_group(int dh) { return dh <= 64 ? 4 : 2; }
// The row-weighted product at mid widths (kernels_predict_grad_mid.hip; mirrored by tests/predict_grad_mid_ref.py): the same sharing of a new point, two
// weight slots at every width: (2 + NW) HD + NW + 2 row-resident doubles per lane (the current and the next weight besides): 52, 68, 84, 100 at NW = 2
static constexpr int predict_grad_mid_split(int dh) { return input_grad_mid_split(dh); }

// ---- device pieces ----
// row k of the lane whose first row is rbase; rows past the end read the last row (and store nothing: row_slab_store)
__device__ __forceinline__ int64_t row_slab_clamped(int64_t rbase, int k, int64_t nrows) {
    const int64_t row = rbase + (int64_t)k * 256;
    return row < nrows ? row : nrows - 1;
}

template <int W>
__device__ __forceinline__ void row_slab_zero(double (&acc)[W]) {
#pragma unroll
    for (int b = 0; b < W; ++b) acc[b] = 0.0;
}
template <int G, int W>
__device__ __forceinline__ void row_slab_zero(double (&acc)[G][W]) {
#pragma unroll
    for (int b = 0; b < G; ++b) row_slab_zero(acc[b]);
}

// part[blockIdx.y][row][.] <- the accumulators of one row, when the row exists
template <int W>
__device__ __forceinline__ void row_slab_store(double* __restrict__ part, int64_t nrows, int64_t row, const double (&acc)[W]) {
    if (row < nrows) {
        double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * W;
#pragma unroll
        for (int b = 0; b < W; ++b) o[b] = acc[b];
    }
}
template <int G, int W>
__device__ __forceinline__ void row_slab_store(double* __restrict__ part, int64_t nrows, int64_t row, const double (&acc)[G][W]) {
    if (row < nrows) {
        double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (G * W);
#pragma unroll
        for (int b = 0; b < G; ++b)
#pragma unroll
            for (int d = 0; d < W; ++d) o[b * W + d] = acc[b][d];
    }
}

// one pair into one (row, column) accumulator set: acc[0 .. DP) += (hv w) vec, acc[DP] += kv w
template <int W>
__device__ __forceinline__ void row_slab_grad_acc(double (&acc)[W], double hv, double kv, double w, const double (&vec)[W - 1]) {
    const double t = hv * w;
#pragma unroll
    for (int d = 0; d < W - 1; ++d) acc[d] = __builtin_fma(t, vec[d], acc[d]);
    acc[W - 1] = __builtin_fma(kv, w, acc[W - 1]);
}

// (The hot-unit difference df = xi - xj with its d2 is NOT here: the register allocation of cross_grad_kernel and weighted_grad_kernel, its two
// users, moves when it is a function of its own.  weighted_grad_kernel keeps its accumulate and store written out for the same reason.)

// ---- the value finish kernel: out[i * ldo + b] = scale * sum_js part[js][i][b], b < sg <= SP; the slabs in fixed order ----
template <int SP>
__global__ __launch_bounds__(256) void row_slab_finish_kernel(const double* __restrict__ part, int jsplit, int64_t nrows, int sg, double scale,
                                                              double* __restrict__ out, int64_t ldo) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * SP) return;
    const int64_t i = idx / SP;
    const int b = (int)(idx - i * SP);
    if (b >= sg) return;
    double s = 0.0;
    for (int js = 0; js < jsplit; ++js) s += part[(int64_t)js * nrows * SP + idx];
    out[i * ldo + b] = scale * s;
}
template <int SP>
static int row_slab_finish(cglb_ctx* c, const double* part, int64_t jsplit, int64_t nrows, int sg, double scale, double* out, int64_t ldo) {
    hipLaunchKernelGGL(row_slab_finish_kernel<SP>, dim3((unsigned)((nrows * SP + 255) / 256)), dim3(256), 0, c->stream, part, (int)jsplit, nrows, sg, scale, out,
                       ldo);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// ---- host rules (mirrored by tests/slab_rules.py).  nrows >= 1, ncols / F >= 1: every launcher returns before them when there are no rows ----
// Column split of the pair kernels: jsplit = forced (c->kff_jsplit) or ceil(8192 / row blocks), within 1 .. min(slot_cap, ceil(ncols / 64)); chunks of
// ceil(ncols / jsplit) columns, rounded up to an even length where `even`; then the chunk count that length gives.
static inline void row_slab_pair_split(int64_t forced, int64_t row_blocks, int64_t ncols, int64_t slot_cap, bool even, int64_t* jsplit_out, int64_t* jchunk_out) {
    int64_t jsplit = forced > 0 ? forced : (8192 + row_blocks - 1) / row_blocks;
    if (jsplit > slot_cap) jsplit = slot_cap;
    if (jsplit > (ncols + 63) / 64) jsplit = (ncols + 63) / 64;
    if (jsplit < 1) jsplit = 1;
    int64_t jchunk = (ncols + jsplit - 1) / jsplit;
    if (even) jchunk = (jchunk + 1) & ~(int64_t)1;
    *jchunk_out = jchunk;
    *jsplit_out = (ncols + jchunk - 1) / jchunk;
}

// Feature split: jsplit = ceil(FEATURE_TARGET_WG / row blocks) within 1 .. min(slot_cap, ceil(F / FEATURE_MIN_CHUNK)); chunks of ceil(F / jsplit)
// features; then the chunk count that length gives.
static inline void row_slab_feature_split(int64_t rows_per_block, int64_t nrows, int64_t F, int64_t slot_cap, int64_t* jsplit_out, int64_t* jchunk_out) {
    const int64_t bx = (nrows + rows_per_block - 1) / rows_per_block;
    int64_t jsplit = (FEATURE_TARGET_WG + bx - 1) / bx;
    if (jsplit > slot_cap) jsplit = slot_cap;
    if (jsplit > (F + FEATURE_MIN_CHUNK - 1) / FEATURE_MIN_CHUNK) jsplit = (F + FEATURE_MIN_CHUNK - 1) / FEATURE_MIN_CHUNK;
    if (jsplit < 1) jsplit = 1;
    const int64_t jchunk = (F + jsplit - 1) / jsplit;
    *jchunk_out = jchunk;
    *jsplit_out = (F + jchunk - 1) / jchunk;
}

// Split of the inducing points of the transposed panel pass: msplit = forced (c->kuf_msplit) or ceil(GRAD_X_KUF_TARGET_WG / row blocks), within
// 1 .. min(slot_cap, ceil(M / GRAD_X_KUF_MIN_CHUNK)) (a forced count: within 1 .. min(slot_cap, M)); chunks of ceil(M / msplit) inducing points; then the chunk count that length gives.  A large N
// fills the device with its row blocks alone (one chunk, no slab traffic beyond the result); a small N is split over m.
static inline void row_slab_panel_split(int64_t forced, int64_t row_blocks, int64_t M, int64_t slot_cap, int64_t* msplit_out, int64_t* mchunk_out) {
    const int64_t min_chunk = forced > 0 ? 1 : GRAD_X_KUF_MIN_CHUNK;  // a forced count is held to M alone: the tests split a handful of points
    int64_t msplit = forced > 0 ? forced : (GRAD_X_KUF_TARGET_WG + row_blocks - 1) / row_blocks;
    if (msplit > slot_cap) msplit = slot_cap;
    if (msplit > (M + min_chunk - 1) / min_chunk) msplit = (M + min_chunk - 1) / min_chunk;
    if (msplit < 1) msplit = 1;
    const int64_t mchunk = (M + msplit - 1) / msplit;
    *mchunk_out = mchunk;
    *msplit_out = (M + mchunk - 1) / mchunk;
}

// most chunks of a gradient launch: ROW_SLAB_SLOTS, fewer where nrows rows of row_doubles partial sums each would exceed the slab
static inline int64_t row_slab_slot_cap(int64_t nrows, int64_t row_doubles) {
    return std::max<int64_t>(1, std::min<int64_t>(ROW_SLAB_SLOTS, (int64_t)ROW_SLAB_GRAD_DOUBLES / (nrows * row_doubles)));
}

// ---- kernel arguments by value ----
struct RowSlabCentre { double c[CGLB_MAX_D_NARROW]; };  // the centre the raw rows are taken about
static inline RowSlabCentre row_slab_centre(const cglb_ctx* c) {
    RowSlabCentre cen;
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) cen.c[k] = k < c->D ? c->xmean[k] : 0.0;
    return cen;
}

struct RowSlabGradScale { double g[CGLB_MAX_D_NARROW]; };  // constant of gradient component k
// of a cross product in hot units at the lengthscales ls (host, [D]): delta_hot = ks (x*_k - x_jk) / l_k, so d kappa / d x*_k = -var h delta_hot / (l_k ks)
static inline RowSlabGradScale row_slab_cross_grad_scale(const cglb_ctx* c, const double* ls, double var) {
    RowSlabGradScale gs;
    const double ks = cglb_kscale(c) * cglb_hot_scale(c);
    for (int k = 0; k < CGLB_MAX_D_NARROW; ++k) gs.g[k] = k < c->D ? -var / (ls[k] * ks) : 0.0;
    return gs;
}
