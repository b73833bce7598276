// K1, symmetric multi-right-hand-side form for mid-width inputs (32 < D <= 96, fp64): Out[b] = (K_ff + noise I) V[b], b < S columns, every
// kernel value evaluated ONCE.  The decomposition is that of kff_multi_kernel (kernels_kff_multi.hip), the operands are those of the
// broadcast-operand branch of the single kernel (kernels_kff_sym.hip, MID):
//   * a workgroup is four waves = four consecutive 64-row blocks (one row per lane) against a SPAN of Q LDS chunks; the row sums stay in
//     registers across the span, the column sums of a chunk are staged in LDS and stored as one vector per right-hand side; the slabs
//     Prow / Pcol, the work list and the combine kernel are the narrow product's own (multi_prepare, multi_combine);
//   * the row operand x_i fills 2 DP VGPRs; a column's coordinates travel as DP / CH slice registers (vector loads, lane l holding
//     coordinate CH s + l % CH) and reach the fma through row_newbcast (devmath.h: fmac_bcast).  Slice s of the NEXT column is requested
//     into the register pair slice s of this column just left;
//   * a_j and the S_pad column-side values Vi[j][0 .. S_pad) stay one contiguous scalar load, as in the narrow kernel;
//   * at these widths the Gram chain is most of a pair's cost: about DP + 14 + 2 S_pad vector-fp64 instructions per pair against
//     S (DP + 17) for S mat-vecs (instruction model).
// The group width S_pad and the number of per-lane partials follow the register budget of each width (pair_worklist.h: multi_mid_group,
// multi_mid_partials; the table of every instance is in DESIGN.md section 4b).  Both exponent ranges are instantiated: at the usual
// initial hyper-parameters (l = 1 on standardised data) a mid-width context is range-clamped.
// No atomics: results are bitwise reproducible, equal columns of V give bitwise equal columns of Out, and a permutation of the columns
// inside one group permutes the output columns bitwise.
// The three kinds are compiled in translation units of their own (kernels_kff_multi_mid_m32.hip and _m52.hip include this file).
#include "pair_common.h"

// Columns [j0, j1) of one LDS chunk (first column c0) against the 64 rows of one block; the row sums continue in acc.
template <int KIND, int DP, int SP, int PART, bool CLAMP, int PREC>
__device__ __forceinline__ void kff_multi_mid_cols(const double* __restrict__ Xs, const double* __restrict__ xa, const double* __restrict__ Vi,
                                                   const double (&xi)[DP], const double ai, const double (&pr)[SP], double (&acc)[SP], int64_t j0,
                                                   int64_t j1, int64_t c0, int64_t sym_from, double* __restrict__ cs, double* __restrict__ tr,
                                                   const double* __restrict__ tab, int lane) {
    constexpr bool FOLD = pair_fold<KIND, CLAMP>(), BIASED = pair_biased<double, KIND, CLAMP, PREC>();
    constexpr int NB = PART / SP;                                              // columns per batch
    constexpr int CH = DP % 16 == 0 ? 16 : (DP % 8 == 0 ? 8 : 4), NCH = DP / CH;  // coordinates per slice register, slices per column
    static_assert(PART % 8 == 0 && PART % SP == 0 && 16 % NB == 0 && DP % CH == 0, "batch geometry");
    const int l16 = lane & (CH - 1);
    const int64_t jfull = j0 + ((j1 - j0) / NB) * NB;  // j0 and the chunk are multiples of 16: only the last batch of the matrix is short
    double xsl[NCH], aj = 0.0;
    if (j0 < jfull) {
        if (!FOLD) aj = xa[j0];
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) xsl[sl] = Xs[j0 * DP + sl * CH + l16];
    }
    for (int64_t jb = j0; jb < jfull; jb += NB) {
        const double* __restrict__ xsj = Xs + jb * DP;  // wave-uniform bases
        const double* __restrict__ xaj = xa + jb;
        const double* __restrict__ vij = Vi + jb * SP;
        const int64_t nb = (jb + NB < jfull) ? NB : 0;  // first column of the next batch (or a harmless re-read)
        double t[PART];
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) {
            // the S_pad column-side values of THIS column: requested before the Gram chain, first used after the 2^x
            double pj[SP], an = 0.0;
            const int64_t o = (jj + 1 < NB) ? jj + 1 : nb;
#pragma unroll
            for (int b = 0; b < SP; ++b) pj[b] = vij[jj * SP + b];
            if (!FOLD) an = xaj[o];
            double gram[1];
            {
                double g0 = ai, g1 = 0.0;
#pragma unroll
                for (int sl = 0; sl < NCH; ++sl) {
                    BcastChain2<0, CH>::run(g0, g1, xsl[sl], &xi[sl * CH]);
                    xsl[sl] = xsj[o * DP + sl * CH + l16];
                }
                gram[0] = g0 + g1;
            }
            __builtin_amdgcn_sched_barrier(0);
            KappaPend<double> kp[1];
            kappa_hot_begin_batch<double, KIND, CLAMP, FOLD || BIASED, PREC, 1>(gram, aj, tab, kp);
            __builtin_amdgcn_sched_barrier(0);
            kappa_hot_poly<double, KIND, PREC>(kp[0]);
            __builtin_amdgcn_sched_barrier(0);
            const double kap = kappa_hot_end<double, KIND>(kp[0]);
            // pin the accumulators at the end of every column (kernels_kff_sym.hip: the optimizer otherwise sinks the fmas of the whole
            // batch below it and hoists the loads of all its columns)
#pragma unroll
            for (int b = 0; b < SP; ++b) {
                acc[b] = __builtin_fma(kap, pj[b], acc[b]);
                t[jj * SP + b] = kap * pr[b];
                asm volatile("" : "+v"(t[jj * SP + b]));
                asm volatile("" : "+v"(acc[b]));
            }
            __builtin_amdgcn_sched_barrier(0);
            aj = an;
        }
        if (jb >= sym_from) {  // wave-uniform; sym_from is a multiple of 64, so a batch never straddles it
            // column sums of the batch = sums across the 64 lanes of the partials; partial q = (column q / SP, right-hand side q % SP)
            // lands at cs[(jb - c0) * SP + q]
#pragma unroll
            for (int part = 0; part < PART / 8; ++part) {
                const double v = wave_colsum8<double>(t + 8 * part, tr, lane);
                if (lane < 8) cs[(jb - c0) * SP + 8 * part + lane] = v;
            }
        }
    }
    // ragged tail of the matrix (fewer than a batch of columns): one column at a time, plain wave reductions
    for (int64_t jc = jfull; jc < j1; ++jc) {
        const double ajc = FOLD ? 0.0 : xa[jc];
        double ct[NCH], pj[SP];
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) ct[sl] = Xs[jc * DP + sl * CH + l16];
#pragma unroll
        for (int b = 0; b < SP; ++b) pj[b] = Vi[jc * SP + b];
        double g0 = ai, g1 = 0.0;
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) BcastChain2<0, CH>::run(g0, g1, ct[sl], &xi[sl * CH]);
        const double kap = kappa_hot_single<double, KIND, CLAMP, FOLD || BIASED, PREC>(g0 + g1, ajc, tab);
#pragma unroll
        for (int b = 0; b < SP; ++b) {
            acc[b] = __builtin_fma(kap, pj[b], acc[b]);
            const double tj = kap * pr[b];
            if (jc >= sym_from) {
                const double v = wave_sum(tj);
                if (lane == 0) cs[(jc - c0) * SP + b] = v;
            }
        }
    }
}

// A workgroup = 4 waves = the row blocks 4g .. 4g+3 against the span K = Q consecutive LDS chunks of `chunk` columns
// (groups[blockIdx.x] = (g, K) or (-1, -1) for a padding workgroup of the XCD-aware order): kff_multi_kernel with one row per lane.
// Waves per SIMD asked of the compiler: two up to the hot width 80 (every instance then fits 256 VGPRs without a spill); at 96 the row
// operand alone takes 192 and a two-wave instance spills, so those run one wave per SIMD with the overflow in the accumulation registers.
template <int KIND, int DP, int SP, int PART, bool CLAMP, int PREC>
__global__ __launch_bounds__(256, (DP <= 80 ? 2 : 1)) void kff_multi_mid_kernel(const double* __restrict__ Xs, const double* __restrict__ xa, const double* __restrict__ V, int s,
                                                            const double* __restrict__ Vi, const double* __restrict__ wcol, int64_t n, int64_t chunk, int Q,
                                                            int nrb, const int2* __restrict__ groups, int64_t prow_ld, double* __restrict__ Prow,
                                                            double* __restrict__ Pcol, const double* __restrict__ exp_tab, double bias) {
    __shared__ double tab[CGLB_TAB_SIZE];
    __shared__ double csum[4 * MULTI_CS_MAX];
    __shared__ double trbuf[4 * 8 * PAIR_TR_LD];
    load_exp_table(tab, exp_tab);  // before the early exit below: every thread reaches the barrier inside
    constexpr bool FOLD = pair_fold<KIND, CLAMP>(), BIASED = pair_biased<double, KIND, CLAMP, PREC>();
    const int lane = threadIdx.x & 63;
    const int2 grp = groups[blockIdx.x];
    if (__builtin_amdgcn_readfirstlane(grp.x) < 0) return;  // padding workgroup: the whole block leaves together
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t g = __builtin_amdgcn_readfirstlane(grp.x), K = __builtin_amdgcn_readfirstlane(grp.y);
    const int64_t rb = 4 * g + wave;           // this wave's row block
    const bool have_rows = rb < nrb;           // wave-uniform
    const int64_t rbase = rb * 64, gbase = 4 * g * 64;
    const int64_t sym_from = rbase + 64;       // columns at or beyond this get the transposed contribution
    double* __restrict__ cs = csum + wave * MULTI_CS_MAX;
    double* __restrict__ tr = trbuf + wave * 8 * PAIR_TR_LD;
    double xi[DP], pr[SP], acc[SP];
    const int64_t row = rbase + lane;
    const bool live = have_rows && row < n;
    const int64_t rr = live ? row : n - 1;
#pragma unroll
    for (int d = 0; d < DP; ++d) xi[d] = Xs[rr * DP + d];
    const double ai = pair_row_seed<double, KIND, BIASED>(xa[rr], bias);
#pragma unroll
    for (int b = 0; b < SP; ++b) {
        pr[b] = (live && b < s) ? V[(int64_t)b * n + rr] : 0.0;
        acc[b] = 0.0;
    }
    for (int q = 0; q < Q; ++q) {
        const int64_t c0 = (K * Q + q) * chunk;
        if (c0 >= n) break;                               // workgroup-uniform
        int64_t c1 = c0 + chunk;
        if (c1 > n) c1 = n;
        if (c1 <= gbase) continue;                        // chunk wholly left of the group: nobody reads its column sums (workgroup-uniform)
        for (int64_t cidx = lane; cidx < chunk * SP; cidx += 64) cs[cidx] = 0.0;  // columns this wave does not reach contribute nothing
        if (have_rows && c1 > rbase) {
            const int64_t j0 = c0 < rbase ? rbase : c0;
            kff_multi_mid_cols<KIND, DP, SP, PART, CLAMP, PREC>(Xs, xa, Vi, xi, ai, pr, acc, j0, c1, c0, sym_from, cs, tr, tab, lane);
        }
        __syncthreads();
        for (int64_t idx = threadIdx.x; idx < chunk * SP; idx += 256) {
            const int64_t b = idx / chunk, cidx = idx - b * chunk;  // consecutive threads: consecutive columns of one right-hand side
            const int64_t j = c0 + cidx;
            if (j < n) {
                const int64_t e = cidx * SP + b;
                const double sum = (csum[e] + csum[MULTI_CS_MAX + e]) + (csum[2 * MULTI_CS_MAX + e] + csum[3 * MULTI_CS_MAX + e]);
                Pcol[(g * SP + b) * n + j] = FOLD ? sum * wcol[j] : sum;
            }
        }
        __syncthreads();  // the staging arrays are zeroed again for the next chunk
    }
    // a block whose first row lies right of the span visited nothing and is not read for this span (combine: K >= K0(i))
    if (have_rows && rbase < (K + 1) * Q * chunk && row < n) {
#pragma unroll
        for (int b = 0; b < SP; ++b) Prow[(K * SP + b) * prow_ld + row] = acc[b];
    }
}

template <int KIND, int DP, int SP>
static int kff_multi_mid_generic(cglb_ctx* c, const double* V, int s, double* Out) {
    constexpr int PART = multi_mid_partials(DP, SP);
    static_assert(SP <= multi_mid_group(DP) && PART > 0, "an instance the register budget of this width does not hold");
    const int64_t n = c->N;
    multi_geometry geo;
    CGLB_TRY(multi_prepare(c, V, s, SP, 64, !c->exp_clamp && KIND == CGLB_RBF, &geo));
    using T = double;
    CGLB_DISPATCH_PREC(c, {
        if (c->exp_clamp)
            hipLaunchKernelGGL((kff_multi_mid_kernel<KIND, DP, SP, PART, true, PREC>), dim3(geo.nwg), dim3(256), 0, c->stream, (const double*)c->Xh,
                               (const double*)c->xah, V, s, (const double*)c->mm_vi, (const double*)nullptr, n, geo.chunk, geo.Q, geo.nrb,
                               (const int2*)c->mm_list.dev, geo.prow_ld, geo.Prow, geo.Pcol, (const double*)c->exp_tab, 0.0);
        else
            hipLaunchKernelGGL((kff_multi_mid_kernel<KIND, DP, SP, PART, false, PREC>), dim3(geo.nwg), dim3(256), 0, c->stream, (const double*)c->Xh,
                               (const double*)c->xah, V, s, (const double*)c->mm_vi, (const double*)c->wh, n, geo.chunk, geo.Q, geo.nrb,
                               (const int2*)c->mm_list.dev, geo.prow_ld, geo.Prow, geo.Pcol, (const double*)c->exp_tab, c->m32_bias);
    });
    CGLB_LAUNCH_CHECK(c);
    if (c->kff_skip_combine) return CGLB_OK;
    return multi_combine(c, geo, 64, SP, V, s, Out);
}

// one group of 2 <= sg <= multi_mid_group(Dh) columns of a context with mid_reg(c)
template <int KIND>
static int kff_multi_mid_kind(cglb_ctx* c, const double* V, int sg, double* Out) {
    const int sp = multi_group_pad(sg);
#define MULTI_MID_CASE(DH)                                                                                                    \
    case DH:                                                                                                                  \
        if constexpr (multi_mid_group(DH) >= 2) { if (sp == 2) return kff_multi_mid_generic<KIND, DH, 2>(c, V, sg, Out); }    \
        if constexpr (multi_mid_group(DH) >= 4) { if (sp == 4) return kff_multi_mid_generic<KIND, DH, 4>(c, V, sg, Out); }    \
        if constexpr (multi_mid_group(DH) >= 8) { if (sp == 8) return kff_multi_mid_generic<KIND, DH, 8>(c, V, sg, Out); }    \
        break;
    switch (c->Dh) {
        MULTI_MID_CASE(48)
        MULTI_MID_CASE(64)
        MULTI_MID_CASE(80)
        MULTI_MID_CASE(96)
    }
#undef MULTI_MID_CASE
    return cglb_fail(c, CGLB_ERR_BAD_ARG, "no shared-kernel product instance for this width and group");
}

#if defined(CGLB_MULTI_MID_M32)
int kff_multi_mid_m32(cglb_ctx* c, const double* V, int sg, double* Out) { return kff_multi_mid_kind<CGLB_MATERN32>(c, V, sg, Out); }
#elif defined(CGLB_MULTI_MID_M52)
int kff_multi_mid_m52(cglb_ctx* c, const double* V, int sg, double* Out) { return kff_multi_mid_kind<CGLB_MATERN52>(c, V, sg, Out); }
#else
int kff_multi_mid_m32(cglb_ctx* c, const double* V, int sg, double* Out);
int kff_multi_mid_m52(cglb_ctx* c, const double* V, int sg, double* Out);
int launch_kff_multi_mid(cglb_ctx* c, const double* V, int sg, double* Out) {
    if (sg < 2 || sg > multi_mid_group(c->Dh)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "group width outside the mid-width product's");
    if (c->kind == CGLB_RBF) return kff_multi_mid_kind<CGLB_RBF>(c, V, sg, Out);
    if (c->kind == CGLB_MATERN32) return kff_multi_mid_m32(c, V, sg, Out);
    if (c->kind == CGLB_MATERN52) return kff_multi_mid_m52(c, V, sg, Out);
    return cglb_fail(c, CGLB_ERR_BAD_ARG, "unsupported kernel kind");
}
#endif
