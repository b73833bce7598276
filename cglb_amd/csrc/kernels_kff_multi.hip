// K1, symmetric multi-right-hand-side form: Out[b] = (K_ff + noise I) V[b] for b < S columns, every kernel value evaluated ONCE.
//
// The single-column symmetric kernel (kernels_kff_sym.hip) spends ~18 vector-fp64 instructions on a kernel value and ~3 on using it.
// Here the value is used for S_pad columns: 2 S_pad fmas per pair (row sums and transposed column sums), so a product with S columns
// costs about 18 + 3 S instructions per pair against 21 S for S mat-vecs.  Same decomposition as the single kernel:
//   * a wave owns 64*R rows (R per lane: the row operand x_i, the row-side values V[b][i] and the R x S_pad row sums live in VGPRs)
//     and streams the columns j >= its first row; x_j / a_j and the S_pad column-side values of column j are wave-uniform scalar
//     loads.  The column-side values are interleaved to Vi[N][S_pad] by a small prep kernel (multi_operand_kernel: zero padded, and
//     pre-weighted with 2^(a_j) for the folded RBF column norm), so the S_pad operands of a column are ONE contiguous scalar load;
//   * the cross-lane transposition unit stays at 16 partial sums per lane: a batch is 16 / S_pad columns x S_pad right-hand sides,
//     transposed through the same 8 x 64 LDS scratch as in the single kernel - the per-lane partials do not grow with S;
//   * rows per lane R shrink where R (Dp + 2 S_pad) operands would not fit the VGPR budget (multi_rows_per_lane);
//   * the column sums of a work item are staged in LDS, interleaved [chunk][S_pad]; the LDS holds 1024 of them per wave, so the LDS
//     chunk is at most 1024 / S_pad columns.  A workgroup (4 waves = 4 consecutive row blocks) sweeps a SPAN of Q such chunks in
//     lockstep and keeps its row sums in registers across them: the row-sum slab has one slot per span, as many as the single kernel;
//   * no atomics: every (slot, column, element) of the slabs is written by exactly one workgroup and the combine adds the valid
//     slots in fixed order.  Results are bitwise reproducible, equal columns of V give bitwise equal columns of Out, and a
//     permutation of the columns inside one S_pad group permutes the output columns bitwise.
// Slab layout (double), n = N:
//   Prow[K][b][li], K < nspan : row sums of span K (valid for K >= the span that holds the first row of block rb(i)), ld prow_ld
//   Pcol[g][b][j], g < ceil(nrb / 4) : column sums produced by the group of row blocks 4g .. 4g+3 (valid where the group starts left of j)
// Scope: fp64, Dp <= 32, unclamped exponent range, one rank, full square; the mid widths (32 < D <= 96) have a pair kernel of their own
// (kernels_kff_multi_mid.hip) behind the same geometry, operand and combine.  Everything else falls back to S single mat-vecs
// (launch_kff_matmat below).
#include "pair_common.h"

#define MULTI_PART 16        // partial sums per lane and batch: 16 / S_pad columns x S_pad right-hand sides
#define MULTI_LATE_DP 24     // padded width from which the next column's x operand is fetched after the Gram chain (SGPR budget)

// rows per lane: at most 4 (the single kernel's 8 at Dp <= 4 left the Matern instances 10 VGPRs over the 256 of two waves per SIMD),
// halved while the R (Dp + 2 S_pad) row-resident doubles would exceed 64 (128 VGPRs; the rest of the budget goes to the 16 partials,
// the R kernel-value temporaries and the addresses).  Register use of every instance: DESIGN.md section 4b.
static constexpr int multi_rows_per_lane(int dp, int sp) {
    int r = dp <= 12 ? 4 : (dp <= 16 ? 2 : 1);
    while (r > 1 && r * (dp + 2 * sp) > 64) r /= 2;
    return r;
}

// Vi[j][b] = V[b][j] (* wh[j] for the folded RBF column norm), zero for the padding columns b >= s
__global__ __launch_bounds__(256) void multi_operand_kernel(const double* __restrict__ V, int s, int sp, int64_t n, const double* __restrict__ wh,
                                                            double* __restrict__ Vi) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * sp) return;
    const int64_t j = idx / sp;
    const int b = (int)(idx - j * sp);
    double v = b < s ? V[(int64_t)b * n + j] : 0.0;
    if (wh) v *= wh[j];
    Vi[idx] = v;
}

// Columns [j0, j1) of one LDS chunk (first column c0) against the rows of one block; the row sums continue in acc.
template <int KIND, int DP, int R, int SP, int PREC>
__device__ __forceinline__ void kff_multi_cols(const double* __restrict__ Xs, const double* __restrict__ xa, const double* __restrict__ Vi,
                                               const double (&xi)[R][DP], const double (&ai)[R], const double (&pr)[R][SP], double (&acc)[R][SP],
                                               int64_t j0, int64_t j1, int64_t c0, int64_t sym_from, double* __restrict__ cs,
                                               double* __restrict__ tr, const double* __restrict__ tab, int lane) {
    constexpr bool FOLD = pair_fold<KIND, false>(), BIASED = pair_biased<double, KIND, false, PREC>();  // fp64, unclamped range
    constexpr int NB = MULTI_PART / SP;  // columns per batch
    constexpr bool LATE = DP >= MULTI_LATE_DP;
    const int64_t jfull = j0 + ((j1 - j0) / NB) * NB;  // j0 and the chunk are multiples of 16: only the last batch of the matrix is short
    double xj[DP], aj = 0.0;
    if (j0 < jfull) {
        if (!FOLD) aj = xa[j0];
#pragma unroll
        for (int d = 0; d < DP; ++d) xj[d] = Xs[j0 * DP + d];
    }
    for (int64_t jb = j0; jb < jfull; jb += NB) {
        const double* __restrict__ xsj = Xs + jb * DP;  // wave-uniform bases: scalar loads with immediate offsets
        const double* __restrict__ xaj = xa + jb;
        const double* __restrict__ vij = Vi + jb * SP;
        const int64_t nb = (jb + NB < jfull) ? NB : 0;  // first column of the next batch (or a harmless re-read)
        double t[MULTI_PART];
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) {
            // the S_pad column-side values of THIS column: requested before the Gram chain, first used after the 2^x (a whole chain and
            // polynomial later); the x operand of the NEXT column one column ahead, as in the single kernel
            double pj[SP], xn[DP], an = 0.0;
            const int64_t o = (jj + 1 < NB) ? jj + 1 : nb;
#pragma unroll
            for (int b = 0; b < SP; ++b) pj[b] = vij[jj * SP + b];
            if (!LATE) {
                if (!FOLD) an = xaj[o];
#pragma unroll
                for (int d = 0; d < DP; ++d) xn[d] = xsj[o * DP + d];
            }
            __builtin_amdgcn_sched_barrier(0);
            double gram[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double g = ai[r];
#pragma unroll
                for (int d = 0; d < DP; ++d) g = __builtin_fma(xi[r][d], xj[d], g);
                gram[r] = g;
            }
            if (LATE) {
                __builtin_amdgcn_sched_barrier(0);
                if (!FOLD) an = xaj[o];
#pragma unroll
                for (int d = 0; d < DP; ++d) xn[d] = xsj[o * DP + d];
                __builtin_amdgcn_sched_barrier(0);
            }
            KappaPend<double> kp[R];
            kappa_hot_begin_batch<double, KIND, false, FOLD || BIASED, PREC, R>(gram, aj, tab, kp);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < R; ++r) kappa_hot_poly<double, KIND, PREC>(kp[r]);
            __builtin_amdgcn_sched_barrier(0);
            double tj[SP];
#pragma unroll
            for (int b = 0; b < SP; ++b) tj[b] = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double kap = kappa_hot_end<double, KIND>(kp[r]);
#pragma unroll
                for (int b = 0; b < SP; ++b) {
                    acc[r][b] = __builtin_fma(kap, pj[b], acc[r][b]);
                    tj[b] = __builtin_fma(kap, pr[r][b], tj[b]);
                }
            }
            // pin the accumulators at the end of every column (kernels_kff_sym.hip: the optimizer otherwise sinks the fmas of the whole
            // batch below it and hoists the scalar loads of all its columns)
#pragma unroll
            for (int b = 0; b < SP; ++b) {
                t[jj * SP + b] = tj[b];
                asm volatile("" : "+v"(t[jj * SP + b]));
#pragma unroll
                for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[r][b]));
            }
            __builtin_amdgcn_sched_barrier(0);
            aj = an;
#pragma unroll
            for (int d = 0; d < DP; ++d) xj[d] = xn[d];
        }
        if (jb >= sym_from) {  // wave-uniform; sym_from is a multiple of 64, so a batch never straddles it
            // column sums of the batch = sums across the 64 lanes of the 16 partials; partial q = (column q / SP, right-hand side q % SP)
            // lands at cs[(jb - c0) * SP + q]: with the interleaved layout the single kernel's two 8-wide transpositions (wave_colsum8) fit
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const double v = wave_colsum8<double>(t + 8 * half, tr, lane);
                if (lane < 8) cs[(jb - c0) * SP + 8 * half + lane] = v;
            }
        }
    }
    // ragged tail of the matrix (fewer than a batch of columns): one column at a time, plain wave reductions
    for (int64_t jc = jfull; jc < j1; ++jc) {
        const double ajc = FOLD ? 0.0 : xa[jc];
        double xc[DP], pj[SP], tj[SP];
#pragma unroll
        for (int d = 0; d < DP; ++d) xc[d] = Xs[jc * DP + d];
#pragma unroll
        for (int b = 0; b < SP; ++b) { pj[b] = Vi[jc * SP + b]; tj[b] = 0.0; }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double g = ai[r];
#pragma unroll
            for (int d = 0; d < DP; ++d) g = __builtin_fma(xi[r][d], xc[d], g);
            const double kap = kappa_hot_single<double, KIND, false, FOLD || BIASED, PREC>(g, ajc, tab);
#pragma unroll
            for (int b = 0; b < SP; ++b) {
                acc[r][b] = __builtin_fma(kap, pj[b], acc[r][b]);
                tj[b] = __builtin_fma(kap, pr[r][b], tj[b]);
            }
        }
        if (jc >= sym_from) {
#pragma unroll
            for (int b = 0; b < SP; ++b) {
                const double v = wave_sum(tj[b]);
                if (lane == 0) cs[(jc - c0) * SP + b] = v;
            }
        }
    }
}

// A workgroup = 4 waves = the row blocks 4g .. 4g+3 against the span K = Q consecutive LDS chunks of `chunk` columns
// (groups[blockIdx.x] = (g, K) or (-1, -1) for a padding workgroup of the XCD-aware order).  The four waves walk the chunks of the span in
// lockstep: after each chunk the workgroup adds the four staged column-sum arrays in fixed order and stores one vector per right-hand side.
template <int KIND, int DP, int R, int SP, int PREC>
__global__ __launch_bounds__(256, 2) void kff_multi_kernel(const double* __restrict__ Xs, const double* __restrict__ xa, const double* __restrict__ V, int s,
                                                           const double* __restrict__ Vi, const double* __restrict__ wcol, int64_t n, int64_t chunk, int Q,
                                                           int nrb, const int2* __restrict__ groups, int64_t prow_ld, double* __restrict__ Prow,
                                                           double* __restrict__ Pcol, const double* __restrict__ exp_tab, double bias) {
    __shared__ double tab[CGLB_TAB_SIZE];
    __shared__ double csum[4 * MULTI_CS_MAX];
    __shared__ double trbuf[4 * 8 * PAIR_TR_LD];
    load_exp_table(tab, exp_tab);  // before the early exit below: every thread reaches the barrier inside
    constexpr bool FOLD = pair_fold<KIND, false>(), BIASED = pair_biased<double, KIND, false, PREC>();
    constexpr int RBROWS = 64 * R;
    const int lane = threadIdx.x & 63;
    const int2 grp = groups[blockIdx.x];
    if (__builtin_amdgcn_readfirstlane(grp.x) < 0) return;  // padding workgroup: the whole block leaves together
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t g = __builtin_amdgcn_readfirstlane(grp.x), K = __builtin_amdgcn_readfirstlane(grp.y);
    const int64_t rb = 4 * g + wave;           // this wave's row block
    const bool have_rows = rb < nrb;           // wave-uniform
    const int64_t rbase = rb * RBROWS, gbase = 4 * g * RBROWS;
    const int64_t sym_from = rbase + RBROWS;   // columns at or beyond this get the transposed contribution
    double* __restrict__ cs = csum + wave * MULTI_CS_MAX;
    double* __restrict__ tr = trbuf + wave * 8 * PAIR_TR_LD;
    double xi[R][DP], ai[R], pr[R][SP], acc[R][SP];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = rbase + r * 64 + lane;
        const bool live = have_rows && row < n;
        const int64_t rr = live ? row : n - 1;
#pragma unroll
        for (int d = 0; d < DP; ++d) xi[r][d] = Xs[rr * DP + d];
        ai[r] = pair_row_seed<double, KIND, BIASED>(xa[rr], bias);
#pragma unroll
        for (int b = 0; b < SP; ++b) {
            pr[r][b] = (live && b < s) ? V[(int64_t)b * n + rr] : 0.0;
            acc[r][b] = 0.0;
        }
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
            kff_multi_cols<KIND, DP, R, SP, PREC>(Xs, xa, Vi, xi, ai, pr, acc, j0, c1, c0, sym_from, cs, tr, tab, lane);
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
    if (have_rows && rbase < (K + 1) * Q * chunk) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = rbase + r * 64 + lane;
            if (row < n) {
#pragma unroll
                for (int b = 0; b < SP; ++b) Prow[(K * SP + b) * prow_ld + row] = acc[r][b];
            }
        }
    }
}

// Out[b][i] = var * ( sum_{K >= K0(i)} Prow[K][b][i] + sum_{g < ceil(rb(i) / 4)} Pcol[g][b][i] ) + noise * V[b][i];  blockIdx.y = b.
// Block = 64 elements x 4 slot groups, the four group sums added in fixed order through LDS (as kff_sym_combine_kernel).
__global__ __launch_bounds__(256) void kff_multi_combine_kernel(const double* __restrict__ Prow, int nspan, int64_t prow_ld, const double* __restrict__ Pcol,
                                                                int64_t n, int64_t span, int rbrows, int sp, double var, double noise,
                                                                const double* __restrict__ V, double* __restrict__ Out) {
    __shared__ double gsum[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
        const int64_t rbi = i / rbrows;
        const int64_t K0 = (rbi * rbrows) / span;
        int u = 0;
        for (int64_t K = K0 + g; K < nspan; K += 4, u = (u + 1) & 7) a[u] += CGLB_STREAM_LOAD(Prow + (K * sp + b) * prow_ld + i);
        const int64_t ns = (rbi + 3) / 4;  // groups that hold a row block left of block rbi
        for (int64_t c = g; c < ns; c += 4, u = (u + 1) & 7) a[u] += CGLB_STREAM_LOAD(Pcol + (c * sp + b) * n + i);
    }
    gsum[g][lane] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (g == 0 && i < n) {
        const double sum = (gsum[0][lane] + gsum[1][lane]) + (gsum[2][lane] + gsum[3][lane]);
        Out[(int64_t)b * n + i] = __builtin_fma(noise, V[(int64_t)b * n + i], var * sum);
    }
}

// Work list: one entry (g, K) per workgroup, for every group g of four row blocks and every span K the group's first block reaches, in the
// order of the single kernel (option "sym_order"; pair_worklist.h: pair_work_order).
static int ensure_multi_items(cglb_ctx* c, int64_t n, int rbrows, int64_t span, int* nwg_out) {
    const int64_t key[6] = {n, span, rbrows, 1, 0, c->sym_order};
    if (!c->mm_list.holds(key)) {
        const int nrb = (int)((n + rbrows - 1) / rbrows), nspan = (int)((n + span - 1) / span);
        auto first_span = [&](int g) { return (int)(((int64_t)4 * g * rbrows) / span); };
        CGLB_TRY(pair_list_store(c, &c->mm_list, key, {}, pair_work_order((nrb + 3) / 4, nspan, first_span, c->sym_order)));
    }
    *nwg_out = c->mm_list.nwg;
    return CGLB_OK;
}

// Geometry, work list, slabs and the interleaved operand of one group of the product (both pair kernels: this file and kernels_kff_multi_mid.hip)
int multi_prepare(cglb_ctx* c, const double* V, int s, int sp, int rbrows, bool fold, multi_geometry* geo) {
    const int64_t n = c->N;
    // span: the column chunk rule of the single kernel (option "sym_chunk"); LDS chunk: at most MULTI_CS_MAX / sp columns of it, Q to the span
    int64_t span = pair_column_chunk(n, rbrows, 1, c->sym_chunk_opt);
    const int64_t chunk = std::min<int64_t>(span, MULTI_CS_MAX / sp);  // 512 / 256 / 128: multiples of 16
    const int Q = (int)((span + chunk - 1) / chunk);
    span = (int64_t)Q * chunk;
    int nwg = 0;
    CGLB_TRY(ensure_multi_items(c, n, rbrows, span, &nwg));
    const int nrb = (int)((n + rbrows - 1) / rbrows), ngroups = (nrb + 3) / 4, nspan = (int)((n + span - 1) / span);
    const int64_t prow_ld = (int64_t)nrb * rbrows;
    const size_t need = ((size_t)ngroups * n + (size_t)nspan * prow_ld) * sp * sizeof(double);
    CGLB_TRY(pair_reserve_slabs(c, &c->mm_part, &c->mm_part_cap, need, "K_ff mat-mat", "", "multiply fewer columns at a time"));
    CGLB_TRY(c->mem.reserve(c, &c->mm_vi, &c->mm_vi_cap, (size_t)n * 8 * sizeof(double)));
    hipLaunchKernelGGL(multi_operand_kernel, dim3((unsigned)((n * sp + 255) / 256)), dim3(256), 0, c->stream, V, s, sp, n,
                       fold ? (const double*)c->wh : (const double*)nullptr, (double*)c->mm_vi);
    CGLB_LAUNCH_CHECK(c);
    geo->span = span; geo->chunk = chunk; geo->prow_ld = prow_ld;
    geo->Q = Q; geo->nwg = nwg; geo->nrb = nrb; geo->nspan = nspan;
    geo->Prow = (double*)c->mm_part;
    geo->Pcol = geo->Prow + (size_t)nspan * prow_ld * sp;
    return CGLB_OK;
}

int multi_combine(cglb_ctx* c, const multi_geometry& geo, int rbrows, int sp, const double* V, int s, double* Out) {
    hipLaunchKernelGGL(kff_multi_combine_kernel, dim3((unsigned)((c->N + 63) / 64), (unsigned)s), dim3(256), 0, c->stream, (const double*)geo.Prow, geo.nspan,
                       geo.prow_ld, (const double*)geo.Pcol, c->N, geo.span, rbrows, sp, c->var, c->noise, V, Out);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

template <int KIND, int DP, int SP>
static int kff_multi_generic(cglb_ctx* c, const double* V, int s, double* Out, bool skip_combine) {
    constexpr int R = multi_rows_per_lane(DP, SP);
    constexpr int RBROWS = 64 * R;
    multi_geometry geo;
    CGLB_TRY(multi_prepare(c, V, s, SP, RBROWS, pair_fold<KIND, false>(), &geo));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((kff_multi_kernel<KIND, DP, R, SP, PREC>), dim3(geo.nwg), dim3(256), 0, c->stream, (const double*)c->Xh,
                                             (const double*)c->xah, V, s, (const double*)c->mm_vi, (const double*)c->wh, c->N, geo.chunk, geo.Q, geo.nrb,
                                             (const int2*)c->mm_list.dev, geo.prow_ld, geo.Prow, geo.Pcol, (const double*)c->exp_tab, c->m32_bias));
    CGLB_LAUNCH_CHECK(c);
    if (skip_combine) return CGLB_OK;
    return multi_combine(c, geo, RBROWS, SP, V, s, Out);
}

// the shared-kernel product exists for fp64, the symmetric variant, one rank owning every row, and: Dp <= 32 with the unclamped exponent
// range; 32 < D <= 96 with the register-resident operand set (mid_reg), both ranges, at the widths that have an instance (multi_mid_group)
bool kff_multi_native(const cglb_ctx* c) {
    if (c->dtype != CGLB_F64 || c->kff_variant != 2 || c->par_world != 1 || c->comm || c->r0 != 0 || c->r1 != c->N) return false;
    if (!is_wide(c)) return !c->exp_clamp;
    return mid_reg(c) && multi_mid_group(c->Dh) >= 2;
}

// Out[b] = (K_ff + noise I) V[b], b < s; V, Out: [s][N] (column b contiguous).  Groups of up to 8 columns (mid widths: multi_mid_group) through
// the shared-kernel product, a single left-over column and every context outside its scope through the single mat-vec.
int launch_kff_matmat(cglb_ctx* c, const void* V, int s, void* Out) {
    const size_t stride = (size_t)c->N * c->esz, ostride = (size_t)c->nloc * c->esz;
    if (!kff_multi_native(c)) {
        for (int b = 0; b < s; ++b) CGLB_TRY(launch_kff_matvec(c, (const char*)V + b * stride, (char*)Out + b * ostride, nullptr));
        return CGLB_OK;
    }
    c->pwh_src = nullptr;  // the weighted copy a PCG update may have left belongs to no operand of this product
    const bool mid = is_wide(c);
    const int group = mid ? multi_mid_group(c->Dh) : MULTI_GROUP_NARROW;
    for (int b0 = 0, sg = 0; b0 < s; b0 += sg) {
        sg = multi_next_group(s - b0, group);
        const double* Vg = (const double*)V + (size_t)b0 * c->N;
        double* Og = (double*)Out + (size_t)b0 * c->N;
        if (sg == 1) { CGLB_TRY(launch_kff_matvec(c, Vg, Og, nullptr)); continue; }
        if (mid) { CGLB_TRY(launch_kff_multi_mid(c, Vg, sg, Og)); continue; }
        const int sp = multi_group_pad(sg);
        const bool skip = c->kff_skip_combine;
        CGLB_DISPATCH_KIND(c->kind, CGLB_DISPATCH_DP(c->Dp, {
            if (sp == 2) CGLB_TRY((kff_multi_generic<KIND, DP, 2>(c, Vg, sg, Og, skip)));
            else if (sp == 4) CGLB_TRY((kff_multi_generic<KIND, DP, 4>(c, Vg, sg, Og, skip)));
            else CGLB_TRY((kff_multi_generic<KIND, DP, 8>(c, Vg, sg, Og, skip)));
        }));
    }
    return CGLB_OK;
}
