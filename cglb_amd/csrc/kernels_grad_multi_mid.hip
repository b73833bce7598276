// K5, multi-pair form at mid widths (32 < D <= 96, fp64): the contract of grad_kff_multi_kernel (kernels_grad_multi.hip),
//   out[d] = sum_b u_b^T (dK_ff / dl_d) v_b, d < D, and out[D] = sum_b u_b^T kappa v_b, for a group of up to SP = 4 or 8 vector pairs,
// on the decomposition of grad_kff_mid_kernel (kernels_grad_mid.hip): a matrix row shared by SPLIT lanes, the column operand in slice
// registers read through row_newbcast, two interleaved Gram chains, S1 in registers, the second moments through wave_colsum8, the same
// row-block deal and jchunk rule.  Only the pair weight differs:
//   diagonal block: w_ij = sum_b u_bi v_bj            to its right: w_ij = sum_b (u_bi v_bj + v_bi u_bj)
// The two orientations are dealt to the two halves of the wave, which hold the same rows: a lane of the lower half keeps u_bi (SP registers)
// and one of the upper half v_bi, the column side UVi[j][2 SP] = (u_0j .. | v_0j ..) is loaded as ONE register per column, lane l of the lower
// half taking v_{l % SP, j} and of the upper half u_{l % SP, j}, and SP v_fmac_f64 row_newbcast form each half's sum (the upper half's is
// dropped inside the diagonal block) - the operand path of the Gram chain.  sum_halves adds the two: SP + 5 lane-instructions per pair
// against the 2 a single pass spends, and SP + 1 registers for the operands of both sides.  The folded column weight 2^(a_j / T) (RBF,
// unclamped range) rides in UVi, as grad_fold_operands puts it into the column-side copies of the single pass; the constant of the gradient
// profile (hfac_scale) is applied by the finish kernel, so that the kappa sum needs no division.
// kappa: RBF kappa = h, the entry is the sum of S0 over the rows; the Matern kinds take P(r) from the root that is the exponent argument
// (kappa = P(r) e, h = hscale L(r) e, e = 2^(-r / T)) and keep one more accumulator.
// Slabs part[(by * gridDim.x + bx) * (DP + 1) + d], entry DP the kappa sum, one workgroup each, summed in fixed order by the finish
// kernel; groups are added in group order: no atomics, bitwise repeatable.  Registers of every instance: DESIGN.md section 4d.
#include "grad_pass.h"

template <int KIND, int DP, int PREC, bool CLAMP, int SPLIT, int SP>
__global__ __launch_bounds__(256, 2) void grad_kff_multi_mid_kernel(const double* __restrict__ Xh, const double* __restrict__ ah, const double* __restrict__ U,
                                                                    const double* __restrict__ V, int s, const double* __restrict__ UVi, int64_t n,
                                                                    int64_t jchunk, double* __restrict__ part, const double* __restrict__ exp_tab,
                                                                    double bias) {
    using T = double;
    using G = GradMidDims<DP, SPLIT>;
    constexpr int HD = G::HD, CH = G::CH, NCH = G::NCH, NQ = G::NQ, WROWS = G::WROWS;
    static_assert(SP == 2 || SP == 4 || SP == 8, "the column operands of a group fill at most half of a 16-lane row");
    constexpr bool FOLD = pair_fold<KIND, CLAMP>(), BIASED = pair_biased<T, KIND, CLAMP, PREC>(), MATERN = cglb_kind_matern<KIND>();
    __shared__ double smem[16];
    __shared__ double tab[CGLB_TAB_SIZE];
    __shared__ T trbuf[4 * 8 * PAIR_TR_LD];
    // the second moments in a private LDS column per lane, as grad_kff_mid_kernel keeps them at width 96: here from width 80 on, where the S_pad = 8
    // instance with them in VGPRs needs 5 - 7 registers more than the 256 of two waves per SIMD
    constexpr bool G2LDS = (DP >= 80 && SPLIT == 2);
    __shared__ T g2buf[G2LDS ? 4 * NQ * 64 : 1];
    load_exp_table(tab, exp_tab);
    const int lane = threadIdx.x & 63, prt = lane / WROWS, l8 = lane & 7;
    const int role = lane >> 5;   // 0: this lane holds u_bi and meets v_bj; 1: v_bi and u_bj
    T* __restrict__ g2 = g2buf + (G2LDS ? (threadIdx.x >> 6) * (NQ * 64) + lane : 0);
    T* __restrict__ tr = trbuf + (threadIdx.x >> 6) * (8 * PAIR_TR_LD);
    const int64_t rblock = (int64_t)blockIdx.x * (4 * WROWS);
    const int64_t row = rblock + (threadIdx.x >> 6) * WROWS + (lane & (WROWS - 1));
    const int64_t rr = row < n ? row : n - 1;
    T xi[HD], S1[HD], G2[G2LDS ? 1 : NQ], rw[SP];
    grad_mid_row_load<DP>(Xh, rr, prt, xi, S1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if constexpr (G2LDS) g2[q * 64] = 0;
        else G2[q] = 0;
    }
#pragma unroll
    for (int b = 0; b < SP; ++b) rw[b] = (row < n && b < s) ? (role ? V : U)[(int64_t)b * n + rr] : T(0);  // padded rows and pairs carry zero weight
    T S0 = 0, acck = 0;
    const T a = ah[rr];
    // from here on the text of grad_kff_mid_kernel but for the pair weight and the kappa sum, written out: as functions the shared steps move
    // instances of this kernel (grad_pass.h lists what was tried)
    const T aseed = prt ? T(0) : ((KIND == CGLB_RBF) ? a : (BIASED ? T(-0.5) * (a + bias) : T(-0.5) * a));
    int64_t j0, j1, sym_from;
    grad_pass_chunk(jchunk, n, rblock, 4 * WROWS, j0, j1, sym_from);
    const T* __restrict__ xcol = Xh + prt * HD + l8;   // + j * DP + 8 s: this lane's element of slice s of column j
    const T* __restrict__ wcol = UVi + (role ? 0 : SP) + (lane & (SP - 1));   // + j * 2 SP: this lane's column-side value of column j
    T xsl[NCH], uvj = 0;
    if (j0 < j1) {
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) xsl[sl] = xcol[j0 * DP + sl * CH];
        uvj = wcol[j0 * (2 * SP)];
    }
    for (int64_t jb = j0; jb < j1; jb += 8) {
        T t[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int64_t jc = jb + jj;
            t[jj] = 0;
            if (jc < j1) {  // wave-uniform: only the last batch of a chunk is short
                const int64_t jn = (jc + 1 < j1) ? jc + 1 : jc;  // next column (or a harmless re-read)
                const T aj = FOLD ? T(0) : ah[jc];
                T w = T(0), w1 = T(0);
                BcastChain2<0, SP>::run(w, w1, uvj, rw);   // the broadcast source comes straight from its load, as the slices of the Gram chain do
                uvj = wcol[jn * (2 * SP)];
                T g = aseed, g1 = T(0);
#pragma unroll
                for (int sl = 0; sl < NCH; ++sl) BcastChain2<0, CH>::run(g, g1, xsl[sl], &xi[sl * CH]);
                g += g1;
                w = (role && jc < sym_from) ? T(0) : w + w1;  // the diagonal block is visited in full: one orientation
                if constexpr (SPLIT == 4) g = sum_row_pairs(g);
                g = sum_halves(g);
                w = sum_halves(w);
                const T earg[1] = {(KIND == CGLB_RBF) ? (FOLD ? g : g + aj) : sqrt_hot<PREC, BIASED>(tfma<T>(T(-2), g, aj))};
                T e[1];
                exp2_tab_batch<CLAMP, MATERN, PREC, 1>(earg, tab, e);
                const T ew = e[0] * w;
                T hv = ew;
                if constexpr (KIND == CGLB_MATERN52) hv = ew * matern52_hlin<T>(earg[0], CGLB_LN2 / CGLB_HOT_UNITS);
                if constexpr (MATERN) acck = tfma<T>(ew, matern_kpoly<T, KIND>(earg[0], CGLB_LN2 / CGLB_HOT_UNITS), acck);
                S0 += hv;
                t[jj] = prt ? T(0) : hv;
#pragma unroll
                for (int sl = 0; sl < NCH; ++sl) {
                    BcastAxpy<0, CH>::run(&S1[sl * CH], xsl[sl], hv);
                    xsl[sl] = xcol[jn * DP + sl * CH];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const T cs = wave_colsum8<T>(t, tr, lane);
        const int64_t jcol = jb + (lane & 7);
        const T* __restrict__ xq = Xh + (jcol < j1 ? jcol : j1 - 1) * DP;  // columns past the chunk carry cs == 0
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int d = (lane >> 3) + 8 * q;
            if (d < DP) {
                const T x = xq[d];
                if constexpr (G2LDS) g2[q * 64] = tfma<T>(cs, x * x, g2[q * 64]);
                else G2[q] = tfma<T>(cs, x * x, G2[q]);
            }
        }
    }
    double* __restrict__ out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (DP + 1);
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        double sum = ((lane >> 3) == (d & 7)) ? (G2LDS ? g2[(d >> 3) * 64] : G2[G2LDS ? 0 : (d >> 3)]) : 0.0;
        const int dl = d % HD;     // the part that holds dimension d adds the row terms
        if (prt == d / HD) sum += xi[dl] * (xi[dl] * S0 - 2.0 * S1[dl]);
        sum = block_sum(sum, smem);
        if (threadIdx.x == 0) out[d] = sum;
    }
    double ks = prt ? 0.0 : (MATERN ? acck : S0);   // every row once
    ks = block_sum(ks, smem);
    if (threadIdx.x == 0) out[DP] = ks;
}

template <int KIND, int DP, int SP>
static int grad_multi_mid_generic(cglb_ctx* c, const double* U, const double* V, int s, double* out, int accumulate) {
    static_assert(SP <= grad_multi_mid_group(DP), "an instance the register budget of this width does not hold");
    const int64_t n = c->N;
    constexpr int SPLIT = grad_multi_mid_split(DP);
    GradMidGeom gm;   // one rank: every row block
    CGLB_TRY(grad_mid_geometry(c, SPLIT, 1, 0, DP + 1, &gm));
    const bool fold = KIND == CGLB_RBF && !c->exp_clamp;
    CGLB_TRY(grad_multi_operands(c, U, V, s, SP, fold ? (const double*)c->wh : (const double*)nullptr));
    dim3 grid((unsigned)gm.bx, (unsigned)gm.jsplit);
    const bool lowprec = c->precision != CGLB_PREC_EXACT;   // level 2 runs as level 1 here, as in the single pass
#define GMM_LAUNCH1(PR, CL)                                                                                                                              \
    hipLaunchKernelGGL((grad_kff_multi_mid_kernel<KIND, DP, PR, CL, SPLIT, SP>), grid, dim3(256), 0, c->stream, (const double*)c->Xh, (const double*)c->xah, U, V, \
                       s, (const double*)c->gm_uv, n, gm.jchunk, c->gpart, (const double*)c->exp_tab, c->m32_bias)
    if (c->exp_clamp) { if (lowprec) GMM_LAUNCH1(CGLB_PREC_FAST, true); else GMM_LAUNCH1(CGLB_PREC_EXACT, true); }
    else { if (lowprec) GMM_LAUNCH1(CGLB_PREC_FAST, false); else GMM_LAUNCH1(CGLB_PREC_EXACT, false); }
#undef GMM_LAUNCH1
    CGLB_LAUNCH_CHECK(c);
    const double hot = cglb_hot_scale(c);
    const double hscale = KIND == CGLB_RBF ? 1.0 : (KIND == CGLB_MATERN32 ? 3.0 : 5.0 / 3.0);  // devmath.h: hfac_scale
    // (s (hscale var / hot^2)) scale_d, scale_d from the device copy
    return grad_finish(c, gm.nblk, DP, 1, (const double*)c->wsmall, hscale * c->var / (hot * hot), 1.0, out, accumulate);
}

// one group of 2 <= sg <= grad_multi_mid_group(Dh) pairs of a context with mid_reg(c)
template <int KIND>
static int grad_multi_mid_kind(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate) {
    const int sp = grad_multi_mid_pad(sg);
#define GMM_CASE(DH)                                                                                                                              \
    case DH:                                                                                                                                      \
        if constexpr (grad_multi_mid_group(DH) >= 4) { if (sp == 4) return grad_multi_mid_generic<KIND, DH, 4>(c, U, V, sg, out, accumulate); }   \
        if constexpr (grad_multi_mid_group(DH) >= 8) { if (sp == 8) return grad_multi_mid_generic<KIND, DH, 8>(c, U, V, sg, out, accumulate); }   \
        break;
    switch (c->Dh) {
        GMM_CASE(48)
        GMM_CASE(64)
        GMM_CASE(80)
        GMM_CASE(96)
    }
#undef GMM_CASE
    return cglb_fail(c, CGLB_ERR_BAD_ARG, "no multi-pair gradient instance for this width and group");
}

#if defined(CGLB_GRAD_MULTI_MID_M32)
int grad_multi_mid_m32(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate) {
    return grad_multi_mid_kind<CGLB_MATERN32>(c, U, V, sg, out, accumulate);
}
#elif defined(CGLB_GRAD_MULTI_MID_M52)
int grad_multi_mid_m52(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate) {
    return grad_multi_mid_kind<CGLB_MATERN52>(c, U, V, sg, out, accumulate);
}
#else
int grad_multi_mid_m32(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate);
int grad_multi_mid_m52(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate);
int launch_grad_kff_multi_mid(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate) {
    if (sg < 2 || sg > grad_multi_mid_group(c->Dh)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "group outside the mid-width multi-pair gradient pass's");
    if (c->kind == CGLB_RBF) return grad_multi_mid_kind<CGLB_RBF>(c, U, V, sg, out, accumulate);
    if (c->kind == CGLB_MATERN32) return grad_multi_mid_m32(c, U, V, sg, out, accumulate);
    if (c->kind == CGLB_MATERN52) return grad_multi_mid_m52(c, U, V, sg, out, accumulate);
    return cglb_fail(c, CGLB_ERR_BAD_ARG, "unsupported kernel kind");
}
#endif
