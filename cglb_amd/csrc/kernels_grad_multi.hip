// K5, multi-pair form: out[d] = sum_b u_b^T (dK_ff / dl_d) v_b for every d and out[D] = sum_b u_b^T kappa v_b (the variance entry), b < S
// pairs of vectors, every kernel value and derivative factor evaluated ONCE per unordered pair (i, j) for a group of up to 8 vector pairs.
// The gradient of the iterative exact-GP class (cglb_itergp_objective_and_grad) is 1 + t such bilinear forms per evaluation.
//
// The decomposition and the direct differences are those of grad_kff_kernel<..., SYM = true> (kernels_grad.hip): a lane owns R rows (x_i, the
// row-side values u_bi, v_bi and the R x (DP + 1) accumulators live in VGPRs) and streams the columns at or right of its row block; x_j and
// the column-side values are wave-uniform scalar loads.  The column side is interleaved to UVi[N][2 S_pad] = (u_0j .. u_{S_pad-1,j}, v_0j ..)
// by a prep kernel (grad_pass.h: grad_multi_operand_kernel, zero padded), so the operands of a column are ONE contiguous scalar load.
//   diagonal block, columns [rblock, rblock + 256 R): visited in full, w_ij = sum_b u_bi v_bj                      (S_pad fmas)
//   to its right:                                   visited once,  w_ij = sum_b (u_bi v_bj + u_bj v_bi)            (2 S_pad fmas)
// then hv = h_ij w_ij, acc_d += hv (x_id - x_jd)^2 and the kappa sum, as in the single pass: about 18 + 4 DP + 2 S_pad vector-fp64
// instructions per pair against S (18 + 4 DP + 2) for S single passes.
// Partial sums go to slabs, part[(blockIdx.y * gridDim.x + blockIdx.x) * (DP + 1) + d], written by exactly one workgroup each and summed in
// fixed order by the finish kernel (grad_pass.h): no atomics, bitwise reproducible.  S > 8 runs in groups of 8 whose sums are added in group order.
// The exponent runs through the range-clamped 2^x like the single direct-difference pass, so the clamped exponent range is native too.
// Native scope: fp64, one rank, one shard covering all rows, at Dp <= 32 (the kernel of this file) and at 32 < D <= 96 with the register-resident
// operand set (mid_reg; kernels_grad_multi_mid.hip, option "grad_multi_mid").  Elsewhere - fp32, D > 96, "wide_reg" 0, N ranks - S single
// launch_grad_kff passes and the kappa sums from one product (launch_grad_kff_multi below).
#include "grad_pass.h"

// rows per lane: 2 up to padded width 8 and 1 beyond, as the single pass.  The row-resident doubles are R (2 DP + 2 S_pad): at most 64 (DP = 8,
// S_pad = 8: 202 VGPRs, two waves per SIMD) with two rows and 80 (DP = 32, S_pad = 8: 256 VGPRs) with one; no instance spills.  Register use of
// every instance: DESIGN.md section 4d.
static constexpr int grad_multi_rows_per_lane(int dp) { return dp <= 8 ? 2 : 1; }

// Columns [j0, j1) against the R rows of a lane.  FULL: both orientations of the pair weight (columns right of the diagonal block).
template <int KIND, int DP, int R, int SP, int PREC, bool FULL>
__device__ __forceinline__ void grad_multi_cols(const double* __restrict__ Xh, const double* __restrict__ UVi, const double (&xi)[R][DP],
                                                const double (&ui)[R][SP], const double (&vi)[R][SP], double (&acc)[R][DP], double (&acck)[R],
                                                int64_t j0, int64_t j1, const double* __restrict__ tab) {
    for (int64_t j = j0; j < j1; ++j) {
        const double* __restrict__ cj = UVi + j * (2 * SP);  // wave-uniform: scalar loads
        double xj[DP], vj[SP], uj[SP];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Xh[j * DP + d];
#pragma unroll
        for (int b = 0; b < SP; ++b) {
            vj[b] = cj[SP + b];
            uj[b] = FULL ? cj[b] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double sq[DP], d2 = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const double df = xi[k][d] - xj[d];
                sq[d] = df * df;
                d2 += sq[d];
            }
            double w = ui[k][0] * vj[0];
#pragma unroll
            for (int b = 1; b < SP; ++b) w = __builtin_fma(ui[k][b], vj[b], w);
            if (FULL) {
#pragma unroll
                for (int b = 0; b < SP; ++b) w = __builtin_fma(vi[k][b], uj[b], w);
            }
            double hv;
            if constexpr (KIND == CGLB_RBF) {  // h = kappa
                hv = exp2_tab<true, PREC>(-0.5 * d2, tab) * w;
                acck[k] += hv;
            } else if constexpr (KIND == CGLB_MATERN32) {  // h = 3 e, kappa = (1 + sqrt3 r) e, e = 2^(-rr / T), sqrt3 r = rr ln 2 / T
                const double rr = 2.0 * sqrt_pos(d2);
                const double ew = exp2_tab<true, PREC>(-rr, tab) * w;
                hv = 3.0 * ew;
                acck[k] = __builtin_fma(ew, __builtin_fma(rr, CGLB_LN2 / CGLB_HOT_UNITS, 1.0), acck[k]);
            } else if constexpr (KIND == CGLB_MATERN52) {  // h = 5/3 (1 + s) e, kappa = (1 + s + s^2 / 3) e, s = sqrt5 r = rr ln 2 / T
                const double rr = 2.0 * sqrt_pos(d2);
                const double ew = exp2_tab<true, PREC>(-rr, tab) * w;
                hv = matern_hpoly<double, KIND>(rr, CGLB_LN2 / CGLB_HOT_UNITS) * ew;
                acck[k] = __builtin_fma(ew, matern_kpoly<double, KIND>(rr, CGLB_LN2 / CGLB_HOT_UNITS), acck[k]);
            } else {
                (void)cglb_kind_unknown<KIND>{};
            }
#pragma unroll
            for (int d = 0; d < DP; ++d) acc[k][d] = __builtin_fma(hv, sq[d], acc[k][d]);
        }
    }
}

// grid (row blocks of 256 R rows, column chunks of jchunk columns); U, V: [s][n] row side; UVi: interleaved column side
template <int KIND, int DP, int R, int SP, int PREC>
__global__ __launch_bounds__(256) void grad_kff_multi_kernel(const double* __restrict__ Xh, const double* __restrict__ U, const double* __restrict__ V,
                                                             int s, const double* __restrict__ UVi, int64_t n, int64_t jchunk,
                                                             double* __restrict__ part, const double* __restrict__ exp_tab) {
    __shared__ double smem[16];
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int64_t rblock = (int64_t)blockIdx.x * (256 * R);
    double xi[R][DP], acc[R][DP], ui[R][SP], vi[R][SP], acck[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = rblock + threadIdx.x + (int64_t)k * 256;
        const bool live = row < n;
        const int64_t rr = live ? row : n - 1;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            xi[k][d] = Xh[rr * DP + d];
            acc[k][d] = 0.0;
        }
#pragma unroll
        for (int b = 0; b < SP; ++b) {  // padded rows and padded pairs carry zero weight
            ui[k][b] = (live && b < s) ? U[(int64_t)b * n + rr] : 0.0;
            vi[k][b] = (live && b < s) ? V[(int64_t)b * n + rr] : 0.0;
        }
        acck[k] = 0.0;
    }
    // grad_pass_chunk of grad_pass.h, written out (calling it here moves two instructions of every instance)
    int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < n) ? j0 + jchunk : n;
    const int64_t sym_from = rblock + 256 * R;
    if (j0 < rblock) j0 = rblock;
    const int64_t jd = j1 < sym_from ? j1 : sym_from;  // end of the diagonal block's share of this chunk
    if (j0 < jd) grad_multi_cols<KIND, DP, R, SP, PREC, false>(Xh, UVi, xi, ui, vi, acc, acck, j0, jd, tab);
    const int64_t jf = j0 > sym_from ? j0 : sym_from;
    if (jf < j1) grad_multi_cols<KIND, DP, R, SP, PREC, true>(Xh, UVi, xi, ui, vi, acc, acck, jf, j1, tab);
    double* __restrict__ out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (DP + 1);
#pragma unroll
    for (int d = 0; d <= DP; ++d) {
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) sum += (d < DP) ? acc[k][d < DP ? d : 0] : acck[k];
        sum = block_sum(sum, smem);
        if (threadIdx.x == 0) out[d] = sum;
    }
}

template <int KIND, int DP, int SP>
static int grad_multi_group(cglb_ctx* c, const double* U, const double* V, int s, double* out, int accumulate) {
    constexpr int R = grad_multi_rows_per_lane(DP);
    const int64_t n = c->N;
    const int64_t bx = (n + 256 * R - 1) / (256 * R);
    int64_t jsplit, jchunk;
    grad_pass_split(bx, n, true, &jsplit, &jchunk);
    const int64_t nblk = bx * jsplit;
    CGLB_TRY(c->mem.reserve(c, &c->gpart, &c->gpart_cap, (size_t)nblk * (DP + 1) * sizeof(double)));
    CGLB_TRY(grad_multi_operands(c, U, V, s, SP, nullptr));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((grad_kff_multi_kernel<KIND, DP, R, SP, PREC>), dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream,
                                             (const double*)c->Xh, U, V, s, (const double*)c->gm_uv, n, jchunk, c->gpart, (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    return grad_finish(c, nblk, DP, 1, grad_scale_params(c), c->var, 1.0, out, accumulate);  // (s var) scale_d
}

static bool grad_multi_mid_native(const cglb_ctx* c) { return mid_reg(c) && c->grad_multi_mid != 0 && grad_multi_mid_group(c->Dh) >= 2; }
bool grad_multi_native(const cglb_ctx* c) {
    return c->dtype == CGLB_F64 && (!is_wide(c) || grad_multi_mid_native(c)) && c->par_world == 1 && !c->comm && c->r0 == 0 && c->r1 == c->N;
}

// fall-back pieces: out[d] += g[d], d < D;  out[D] += sum_i u_i (w_i - noise v_i) / var with w = (K_ff + noise I) v  (one block, fixed order)
template <typename T>
__global__ __launch_bounds__(256) void grad_multi_fallback_kernel(const double* __restrict__ g, int D, const T* __restrict__ u, const T* __restrict__ v,
                                                                  const T* __restrict__ w, int64_t n, double noise, double var, double* __restrict__ out,
                                                                  int accumulate) {
    __shared__ double smem[16];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += (double)u[i] * ((double)w[i] - noise * (double)v[i]);
    s = block_sum(s, smem);
    if (threadIdx.x == 0) {
        for (int d = 0; d < D; ++d) out[d] = accumulate ? out[d] + g[d] : g[d];
        out[D] = (accumulate ? out[D] : 0.0) + s / var;
    }
}

// S single passes added to out (overwritten first unless `accumulate`), and the kappa sums from one product:
// u_b^T kappa v_b = u_b^T ((K_ff + noise I) v_b - noise v_b) / variance
static int grad_multi_single_passes(cglb_ctx* c, const void* U, const void* V, int S, double* out, int accumulate) {
    const size_t stride = (size_t)c->N * c->esz;
    void* W = nullptr;
    double* g = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &W, (size_t)S * stride));
    CGLB_TRY(tmp.alloc(c, (void**)&g, sizeof(double) * c->D));
    auto body = [&]() -> int {
        CGLB_TRY(launch_kff_matmat(c, V, S, W));
        for (int b = 0; b < S; ++b) {
            CGLB_TRY(launch_grad_kff(c, (const char*)V + b * stride, (const char*)U + b * stride, g));
            CGLB_DISPATCH_T(c->dtype, hipLaunchKernelGGL((grad_multi_fallback_kernel<T>), dim3(1), dim3(256), 0, c->stream, (const double*)g, c->D,
                                                         (const T*)((const char*)U + b * stride), (const T*)((const char*)V + b * stride),
                                                         (const T*)((const char*)W + b * stride), c->N, c->noise, c->var, out, (accumulate || b > 0) ? 1 : 0));
            CGLB_LAUNCH_CHECK(c);
        }
        return CGLB_OK;
    };
    const int rc = body();
    (void)hipStreamSynchronize(c->stream);  // before `tmp` releases the buffers the kernels use
    return rc;
}

// out (device double[D + 1], overwritten): sum_b u_b^T (dK_ff/dl_d) v_b, d < D, and sum_b u_b^T kappa v_b.  U, V: device [S][N], pair b contiguous.
int launch_grad_kff_multi(cglb_ctx* c, const void* U, const void* V, int S, double* out) {
    if (!grad_multi_native(c) || (is_wide(c) && S == 1)) {  // a single pair of a mid-width context: the single pass, bitwise what it was
        if (c->r0 != 0 || c->r1 != c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the multi-pair gradient pass needs a single shard covering all rows");
        return grad_multi_single_passes(c, U, V, S, out, 0);
    }
    if (is_wide(c)) {  // mid widths: groups by the rule of pair_worklist.h (grad_multi_mid_group), added in group order; a single left-over pair last
        const int group = grad_multi_mid_group(c->Dh);
        for (int b0 = 0; b0 < S;) {
            const int sg = multi_next_group(S - b0, group);
            const double* Ug = (const double*)U + (size_t)b0 * c->N;
            const double* Vg = (const double*)V + (size_t)b0 * c->N;
            if (sg == 1) CGLB_TRY(grad_multi_single_passes(c, Ug, Vg, 1, out, b0 > 0 ? 1 : 0));
            else CGLB_TRY(launch_grad_kff_multi_mid(c, Ug, Vg, sg, out, b0 > 0 ? 1 : 0));
            b0 += sg;
        }
        return CGLB_OK;
    }
    for (int b0 = 0; b0 < S; b0 += 8) {
        const int sg = std::min(8, S - b0);
        const double* Ug = (const double*)U + (size_t)b0 * c->N;
        const double* Vg = (const double*)V + (size_t)b0 * c->N;
        const int sp = sg <= 1 ? 1 : (sg <= 2 ? 2 : (sg <= 4 ? 4 : 8));
        const int accumulate = b0 > 0 ? 1 : 0;
        CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, {
            if (sp == 1) CGLB_TRY((grad_multi_group<KIND, DP, 1>(c, Ug, Vg, sg, out, accumulate)));
            else if (sp == 2) CGLB_TRY((grad_multi_group<KIND, DP, 2>(c, Ug, Vg, sg, out, accumulate)));
            else if (sp == 4) CGLB_TRY((grad_multi_group<KIND, DP, 4>(c, Ug, Vg, sg, out, accumulate)));
            else CGLB_TRY((grad_multi_group<KIND, DP, 8>(c, Ug, Vg, sg, out, accumulate)));
        }));
    }
    return CGLB_OK;
}
