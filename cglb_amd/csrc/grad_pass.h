// The N^2 gradient passes over K_ff: grad_kff_kernel and grad_kff_gram_kernel (kernels_grad.hip), grad_kff_multi_kernel (kernels_grad_multi.hip),
// grad_kff_mid_kernel (kernels_grad_mid.hip) and grad_kff_multi_mid_kernel (kernels_grad_multi_mid.hip).  One decomposition:
//   * a workgroup owns a block of rows (256 R of the narrow kernels, 256 / SPLIT of the mid-width ones) whose operands and accumulators stay in VGPRs;
//   * the columns at or right of the row block are split over blockIdx.y in chunks of jchunk (grad_pass_split: host, below);
//   * workgroup (blockIdx.x, blockIdx.y) alone writes its partial sums to the slab part[blockIdx.y * gridDim.x + blockIdx.x][W], W = DP or DP + 1
//     (the multi-pair passes add the kappa sum as entry DP);
//   * grad_finish_kernel adds the slabs in fixed order and applies the constants: no atomics, bitwise repeatable.
// Here, once: the split rule, the finish kernel, the operand kernel of the multi-pair passes, the scale fill, the launch geometry of the mid widths
// and the device pieces the kernels can call without a change to their code.  As pair_common.h and row_slab.h: a kernel whose register allocation or
// schedule moves when it calls one of the device pieces keeps that piece written out and says so at the place.
#pragma once
#include "pair_common.h"

// ---- host rules (grad_pass_split is mirrored by tests/slab_rules.py) ----
#define GRAD_PASS_TARGET_WG 8192  // workgroups a launch aims at (twice that for the symmetric form)
// Column split: js = ceil(TARGET_WG / row blocks), doubled for the symmetric form (about half of the (row block, chunk) cells of the square are left
// of the diagonal and exit at once), within 1 .. min(1024, ceil(ncols / 64)); chunks of ceil(ncols / js) columns; then the chunk count that length
// gives.  A sibling of row_slab_pair_split (row_slab.h), not a call of it: 2 ceil(T / bx) is not ceil(2 T / bx) (bx = 5: 3278 against 3277).
static inline void grad_pass_split(int64_t row_blocks, int64_t ncols, bool sym, int64_t* jsplit_out, int64_t* jchunk_out) {
    int64_t js = (GRAD_PASS_TARGET_WG + row_blocks - 1) / row_blocks;
    if (sym) js *= 2;
    if (js > 1024) js = 1024;
    if (js > (ncols + 63) / 64) js = (ncols + 63) / 64;
    if (js < 1) js = 1;
    const int64_t jchunk = (ncols + js - 1) / js;
    *jchunk_out = jchunk;
    *jsplit_out = (ncols + jchunk - 1) / jchunk;
}
// row blocks of rank `rank` when the nb blocks are dealt cyclically to `world` ranks (0: the rank has none)
static inline int64_t grad_pass_dealt_blocks(int64_t nb, int world, int rank) { return rank < nb ? (nb - rank + world - 1) / world : 0; }

// 1 / (l_d kscale^2) in hot units (the N^2 passes run on the hot operand set), by value for grad_finish_kernel
static inline ScaleParams grad_scale_params(const cglb_ctx* c) {
    ScaleParams sp;
    const double ks = cglb_kscale(c) * cglb_hot_scale(c);
    for (int d = 0; d < CGLB_MAX_D_NARROW; ++d) {
        sp.center[d] = 0;
        sp.scale[d] = d < c->D ? 1.0 / (c->ls[d] * ks * ks) : 0.0;
    }
    return sp;
}

// ---- the finish kernel: out[d] (+)= ((sum_blk part[blk][d] fac) scale_d) tail, d < D, and with `extra` out[D] (+)= sum_blk part[blk][DP] (the
// kappa sum, unscaled); slabs of DP + extra doubles, one block per entry, the slabs in fixed order.  The products in exactly this order (a tail of
// 1.0 is exact), uncontracted: every caller's result is bitwise what a finish kernel of its own gave.  scale_d = 1 / (l_d kscale^2) by value
// (grad_scale_params) or from the device copy c->wsmall (kernels_wide.hip: upload_scales) ----
__device__ __forceinline__ double grad_scale_at(const ScaleParams& sp, int d) { return sp.scale[d]; }
__device__ __forceinline__ double grad_scale_at(const double* scale, int d) { return scale[d]; }
template <typename SCALE>
__global__ __launch_bounds__(256) void grad_finish_kernel(const double* __restrict__ part, int64_t nblk, int DP, int D, int extra, SCALE scale, double fac,
                                                          double tail, double* __restrict__ out, int accumulate) {
#pragma clang fp contract(off)
    __shared__ double smem[16];
    const int d = blockIdx.x;
    if (d >= D + extra) return;
    const int col = d < D ? d : DP;
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += blockDim.x) s += part[b * (DP + extra) + col];
    s = block_sum(s, smem);
    if (threadIdx.x == 0) {
        const double val = d < D ? s * fac * grad_scale_at(scale, d) * tail : s;
        out[d] = accumulate ? out[d] + val : val;
    }
}
template <typename SCALE>
static int grad_finish(cglb_ctx* c, int64_t nblk, int DP, int extra, SCALE scale, double fac, double tail, double* out, int accumulate) {
    hipLaunchKernelGGL(grad_finish_kernel<SCALE>, dim3(c->D + extra), dim3(256), 0, c->stream, (const double*)c->gpart, nblk, DP, c->D, extra, scale, fac, tail,
                       out, accumulate);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// ---- the column side of a multi-pair group, interleaved: UVi[j][b] = U[b][j] w_j, UVi[j][sp + b] = V[b][j] w_j (w = 1 without `wh`), zero for the
// padding pairs b >= s, so that the operands of a column are ONE contiguous load, as multi_operand_kernel does for the product ----
static __global__ __launch_bounds__(256) void grad_multi_operand_kernel(const double* __restrict__ U, const double* __restrict__ V, int s, int sp, int64_t n,
                                                                        const double* __restrict__ wh, double* __restrict__ UVi) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * 2 * sp) return;
    const int64_t j = idx / (2 * sp);
    const int q = (int)(idx - j * 2 * sp);
    const int b = q < sp ? q : q - sp;
    const double x = b < s ? (q < sp ? U : V)[(int64_t)b * n + j] : 0.0;
    UVi[idx] = wh ? x * wh[j] : x;
}
// c->gm_uv <- the interleaved column side of the s pairs (U, V: [s][N]) padded to sp
static int grad_multi_operands(cglb_ctx* c, const double* U, const double* V, int s, int sp, const double* wh) {
    CGLB_TRY(c->mem.reserve(c, &c->gm_uv, &c->gm_uv_cap, (size_t)c->N * 16 * sizeof(double)));
    hipLaunchKernelGGL(grad_multi_operand_kernel, dim3((unsigned)((c->N * 2 * sp + 255) / 256)), dim3(256), 0, c->stream, U, V, s, sp, c->N, wh, (double*)c->gm_uv);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// ---- mid widths (32 < D <= 96, fp64): launch geometry ----
// Lanes sharing a matrix row at padded width 96: 2 with the second moments in LDS (16.8 ms at N = 50k; 24.7 with 4).  The Matern-3/2
// instance of the exact level (two-step square root) does not fit 256 registers that way (101 spilled: 41 ms) and keeps 4 (25.5 ms); the
// Matern-5/2 instance has the same root and one more live constant, so the rule is "any Matern kind".
static inline int grad_mid_split(const cglb_ctx* c) {
    if (c->Dh != 96) return 2;
    return (c->kind != CGLB_RBF && c->precision == CGLB_PREC_EXACT) ? 4 : 2;
}
// The multi-pair pass: 2, and 4 at width 96, where every instance with 2 needs scratch (15 - 50 registers beyond 256 with the second moments in
// LDS); the single pass makes the same choice for its Matern instances of the exact level (above)
static constexpr int grad_multi_mid_split(int dp) { return dp == 96 ? 4 : 2; }

// Rows of a workgroup (256 / split), this rank's share of the row blocks (the cyclic deal; one rank: all), the column split of the symmetric
// form, and the slabs of `width` doubles reserved in c->gpart.  bx == 0: the rank has no row block and nothing is reserved.
struct GradMidGeom { int64_t bx, jsplit, jchunk, nblk; };
static int grad_mid_geometry(cglb_ctx* c, int split, int world, int rank, int width, GradMidGeom* g) {
    const int brows = 256 / split;
    g->bx = grad_pass_dealt_blocks((c->N + brows - 1) / brows, world, rank);
    g->jsplit = g->jchunk = g->nblk = 0;
    if (g->bx == 0) return CGLB_OK;
    grad_pass_split(g->bx, c->N, true, &g->jsplit, &g->jchunk);
    g->nblk = g->bx * g->jsplit;
    return c->mem.reserve(c, &c->gpart, &c->gpart_cap, (size_t)g->nblk * width * sizeof(double));
}

// ---- device pieces.  grad_kff_mid_kernel and grad_kff_multi_mid_kernel share their decomposition: a row over SPLIT lanes, the column operand in
// slice registers read through row_newbcast, two interleaved Gram chains, first moments in registers, second moments through wave_colsum8.  Only
// the pieces below can be shared as functions.  Each of the following was tried as a forceinline function (and the whole pass as one body with a
// policy per kernel) and moves the instruction stream of instances of one or both kernels, so both keep it written out: the Gram chains (the operands
// of the chain sum swap), the moment accumulation with the next-column request, the second-moment step, the slice prefetch, the zeroing of the
// second moments, the per-dimension sum of the final store; a body that calls block_sum also loses the fold of blockDim.x to the launch bound ----
// A matrix row is shared by SPLIT lanes (lane l of each half of the wave, SPLIT = 2; of each 16-lane row, SPLIT = 4), each holding HD = DP / SPLIT of
// the dimensions in NCH slices of CH = 8; WROWS rows to a wave; NQ second-moment accumulators per lane (dimensions (lane >> 3) + 8 q)
template <int DP, int SPLIT>
struct GradMidDims {
    static constexpr int HD = DP / SPLIT, CH = 8, NCH = HD / CH, NQ = (DP + 7) / 8, WROWS = 64 / SPLIT;
    static_assert((SPLIT == 2 || SPLIT == 4) && HD % CH == 0, "part width must be a multiple of 8");
};

// the lane's part of row rr into registers, its first moments zeroed
template <int DP, int HD>
__device__ __forceinline__ void grad_mid_row_load(const double* __restrict__ Xh, int64_t rr, int prt, double (&xi)[HD], double (&S1)[HD]) {
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        xi[d] = Xh[rr * DP + prt * HD + d];
        S1[d] = 0;
    }
}

// The columns of workgroup (blockIdx.x, blockIdx.y) of a symmetric pass whose row block is [rblock, rblock + brows): chunk blockIdx.y of jchunk columns,
// from the row block on ([j0, j1), empty left of the diagonal); columns from sym_from on are right of the diagonal block and carry both orientations
__device__ __forceinline__ void grad_pass_chunk(int64_t jchunk, int64_t n, int64_t rblock, int brows, int64_t& j0, int64_t& j1, int64_t& sym_from) {
    j0 = (int64_t)blockIdx.y * jchunk;
    j1 = (j0 + jchunk < n) ? j0 + jchunk : n;
    sym_from = rblock + brows;
    if (j0 < rblock) j0 = rblock;
}
