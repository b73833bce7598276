// Value AND input gradient of the cross product at mid widths (32 < D <= 96, fp64; option "input_grad_mid"): cross_grad_kernel's contract
// (kernels_input_grad.hip) for one group of G columns,
//   out[i, s] = var sum_j kappa(x*_i, x_j) V[s, j],   gout[i, s, k] = -var sum_j h(x*_i, x_j) (x*_ik - x_jk) / l_k^2 V[s, j],
// with a new point shared by SPLIT lanes as in the mid-width gradient pass (kernels_grad_mid.hip):
//   * lane l of a wave holds part l / WROWS (HD = Dh / SPLIT coordinates) of row l % WROWS, WROWS = 64 / SPLIT; a workgroup has 256 / SPLIT rows;
//   * a training point's coordinates travel as NCH = HD / CH slice registers per lane (vector loads: lane l holds coordinate CH s + l % CH of ITS part,
//     CH = 8, or 4 where HD is no multiple of 8) and reach the arithmetic through v_fmac_f64 row_newbcast (devmath.h: BcastDiff); slice s of the NEXT
//     column is requested into the registers of slice s as soon as the differences have been taken;
//   * DIRECT differences delta_k = xh*_k - xh_jk, each one fmac with the multiplier -1 (rounded once, like the subtraction: v_add_f64 has no DPP form);
//     the per-lane partial of d2 = sum delta_k^2 runs in two interleaved chains and meets the other parts through sum_row_pairs / sum_halves - the
//     same sum in every part, bit for bit; kappa and h from that d2 once per pair (kappa_hfac_hot_from_d2: always the range-clamped 2^x, so one
//     instance per kind, width and precision level), redundantly in the SPLIT lanes;
//   * delta form, in-lane: per column of the group one multiply t = h v_s and HD fma acc[s][k] += t delta_k; one fma for the value.  A coincident
//     pair has delta = 0 exactly and adds exactly zero; the zero padding Dh - D of both operands adds exactly zero to d2;
//   * the slabs, the split rule, the slot cap of row_slab.h: part[blockIdx.y][row][G][Dh + 1] (part p writes its HD components, part 0 the value);
//     ONE finish kernel adds the slabs in fixed order and applies -var / (l_k hot scale) from the device copy of the scales.  No atomics.
// The feature product (feature_grad_kernel's contract: out[i, s] = amp sum_j W[s, j] cos(phi_ij), gout[i, s, k] = -amp sum_j W[s, j] sin(phi_ij) omega_jk / l_k)
// is the same machine with a feature in the column's place: the slices are read per lane from the existing operand records (FEATURE_REC(D) doubles:
// { b_j | omega'_j[D] | W[8] } in turns, omega' = omega / (2 pi l)); the phase is a BcastChain2 over the lane's part of the centred row, summed over the
// parts like d2 (part 0 carries b_j); one sincos_turns per pair; per column one multiply t = sin w_s and HD row_newbcast fmas acc[s][k] += omega'_jk t
// (BcastAxpy), one fma for the value; -2 pi amp in the finish.  The slices of the coordinates D .. Dh - 1 re-read the record's last frequency: the row
// holds zeros there, the phase gains exactly zero, and their sums are never stored.
// Every lane takes part in row_newbcast and the permlane swaps: rows past nrows are clamped (row_slab_clamped's rule) and carry their sums unstored;
// the column loop has wave-uniform bounds and nothing in it is divergent.  Geometry: input_grad_mid_split / input_grad_mid_group (row_slab.h);
// registers of every instance: DESIGN.md section 4h.
#include "pair_common.h"
#include "row_slab.h"

#define INPUT_GRAD_MID_ROWS 4096            // new points per launch

// grid (row blocks of 256 / SPLIT new points, column chunks of jchunk training points); Vi points at the first column of the group
template <int KIND, int DP, int SPLIT, int G, int PREC>
__global__ __launch_bounds__(256, 2) void cross_grad_mid_kernel(const double* __restrict__ XhRow, int64_t nrows, const double* __restrict__ Xh,
                                                                const double* __restrict__ Vi, int64_t ldv, int64_t ncols, int64_t jchunk,
                                                                double* __restrict__ part, const double* __restrict__ exp_tab) {
    constexpr int HD = DP / SPLIT, CH = HD % 8 == 0 ? 8 : 4, NCH = HD / CH, WROWS = 64 / SPLIT;
    static_assert((SPLIT == 2 || SPLIT == 4) && DP % SPLIT == 0 && HD % CH == 0, "part width must be a multiple of 4");
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int lane = threadIdx.x & 63, prt = lane / WROWS;   // prt: which 1 / SPLIT of the dimensions this lane holds
    const int64_t row = (int64_t)blockIdx.x * (4 * WROWS) + (threadIdx.x >> 6) * WROWS + (lane & (WROWS - 1));
    const int64_t rr = row < nrows ? row : nrows - 1;
    double xi[HD], acc[G][HD], val[G];
#pragma unroll
    for (int d = 0; d < HD; ++d) xi[d] = XhRow[rr * DP + prt * HD + d];
    row_slab_zero(acc);
    row_slab_zero(val);
    double m1 = -1.0;
    asm volatile("" : "+v"(m1));   // the multiplier of the differences stays in one register pair
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < ncols) ? j0 + jchunk : ncols;
    const double* __restrict__ xcol = Xh + prt * HD + (lane & (CH - 1));   // + j * DP + CH s: this lane's element of slice s of column j
    double xsl[NCH];
    if (j0 < j1) {
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) xsl[sl] = xcol[j0 * DP + sl * CH];
    }
    for (int64_t j = j0; j < j1; ++j) {
        const int64_t jn = (j + 1 < j1) ? j + 1 : j;   // next column (or a harmless re-read)
        const double* __restrict__ cj = Vi + j * ldv;  // wave-uniform: one scalar load of G doubles
        double vj[G], df[HD];
#pragma unroll
        for (int b = 0; b < G; ++b) vj[b] = cj[b];
        double d2 = 0.0, d2b = 0.0;
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) {
            BcastDiff<0, CH>::run(&df[sl * CH], xsl[sl], &xi[sl * CH], m1);
            xsl[sl] = xcol[jn * DP + sl * CH];
#pragma unroll
            for (int k = 0; k < CH; k += 2) {
                d2 = __builtin_fma(df[sl * CH + k], df[sl * CH + k], d2);
                d2b = __builtin_fma(df[sl * CH + k + 1], df[sl * CH + k + 1], d2b);
            }
        }
        d2 += d2b;
        if constexpr (SPLIT == 4) d2 = sum_row_pairs(d2);
        d2 = sum_halves(d2);
        double kv, hv;
        kappa_hfac_hot_from_d2<KIND, PREC>(d2, tab, kv, hv);
#pragma unroll
        for (int b = 0; b < G; ++b) {
            const double t = hv * vj[b];
#pragma unroll
            for (int k = 0; k < HD; ++k) acc[b][k] = __builtin_fma(t, df[k], acc[b][k]);
            val[b] = __builtin_fma(kv, vj[b], val[b]);
        }
    }
    if (row < nrows) {   // after the last cross-lane operation: clamped rows store nothing
        double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (G * (DP + 1));
#pragma unroll
        for (int b = 0; b < G; ++b) {
#pragma unroll
            for (int k = 0; k < HD; ++k) o[b * (DP + 1) + prt * HD + k] = acc[b][k];
            if (prt == 0) o[b * (DP + 1) + DP] = val[b];
        }
    }
}

// grid (row blocks of 256 / SPLIT rows, feature chunks of jchunk); rec points at the first record of the block of 8 columns (rl doubles each), sub at the
// group inside it; X raw rows [nrows][d], cen the centre (device)
template <int DP, int SPLIT, int G>
__global__ __launch_bounds__(256, 2) void feature_grad_mid_kernel(const double* __restrict__ X, int d, const double* __restrict__ cen, int64_t nrows,
                                                                  const double* __restrict__ rec, int rl, int sub, int64_t F, int64_t jchunk,
                                                                  double* __restrict__ part) {
    constexpr int HD = DP / SPLIT, CH = HD % 8 == 0 ? 8 : 4, NCH = HD / CH, WROWS = 64 / SPLIT;
    static_assert((SPLIT == 2 || SPLIT == 4) && DP % SPLIT == 0 && HD % CH == 0, "part width must be a multiple of 4");
    const int lane = threadIdx.x & 63, prt = lane / WROWS;
    const int64_t row = (int64_t)blockIdx.x * (4 * WROWS) + (threadIdx.x >> 6) * WROWS + (lane & (WROWS - 1));
    const int64_t rr = row < nrows ? row : nrows - 1;
    double z[HD], acc[G][HD], val[G];
#pragma unroll
    for (int k = 0; k < HD; ++k) {
        const int q = prt * HD + k;
        const int qq = q < d ? q : d - 1;
        const double v = X[rr * d + qq] - cen[qq];
        z[k] = q < d ? v : 0.0;
    }
    row_slab_zero(acc);
    row_slab_zero(val);
    int off[NCH];   // this lane's element of slice s inside a record: 1 + coordinate, clamped to the last real one
#pragma unroll
    for (int sl = 0; sl < NCH; ++sl) {
        const int q = prt * HD + sl * CH + (lane & (CH - 1));
        off[sl] = 1 + (q < d ? q : d - 1);
    }
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < F) ? j0 + jchunk : F;
    double xsl[NCH];
    if (j0 < j1) {
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) xsl[sl] = rec[j0 * rl + off[sl]];
    }
    for (int64_t j = j0; j < j1; ++j) {
        const int64_t jn = (j + 1 < j1) ? j + 1 : j;   // next feature (or a harmless re-read)
        const double* __restrict__ rj = rec + j * rl;  // wave-uniform: scalar loads of the phase and the G weights
        double wj[G];
        const double bj = rj[0];
#pragma unroll
        for (int b = 0; b < G; ++b) wj[b] = rj[1 + d + sub + b];
        double ph = prt ? 0.0 : bj, ph1 = 0.0;   // the phase offset enters the sum of the parts once
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) BcastChain2<0, CH>::run(ph, ph1, xsl[sl], &z[sl * CH]);
        ph += ph1;
        if constexpr (SPLIT == 4) ph = sum_row_pairs(ph);
        ph = sum_halves(ph);
        double cv, sv;
        sincos_turns(ph, cv, sv);
#pragma unroll
        for (int b = 0; b < G; ++b) {
            const double t = sv * wj[b];
#pragma unroll
            for (int sl = 0; sl < NCH; ++sl) BcastAxpy<0, CH>::run(&acc[b][sl * CH], xsl[sl], t);
            val[b] = __builtin_fma(cv, wj[b], val[b]);
        }
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) xsl[sl] = rec[jn * rl + off[sl]];
    }
    if (row < nrows) {   // after the last cross-lane operation: clamped rows store nothing
        double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (G * (DP + 1));
#pragma unroll
        for (int b = 0; b < G; ++b) {
#pragma unroll
            for (int k = 0; k < HD; ++k) o[b * (DP + 1) + prt * HD + k] = acc[b][k];
            if (prt == 0) o[b * (DP + 1) + DP] = val[b];
        }
    }
}

// the slabs in fixed order, then the constants, per slot b < g (InputGradMidOut, cglb_internal.h): gout[b][i * ldg + k] = (gfac[b] scale[k]) sum_js
// part[js][i][b][k] (k < d; added to what is there for slot 0 under add0), out[b][i * ldo] = vscale * sum_js part[js][i][b][dp]; a slot whose pointer is NULL
// is not stored.  scale: the device copy of kscale / l_k (NULL: 1, the feature product).  One thread per (i, b, k <= dp).  The cross and feature products
// (slot b = column b of the group: out + b, gout + b d, ldg = S d) and the row-weighted product (kernels_predict_grad_mid.hip: one array per slot) share it
__global__ __launch_bounds__(256) void input_grad_mid_finish_kernel(const double* __restrict__ part, int jsplit, int64_t nrows, int g, int dp, int d, double vscale,
                                                                    const double* __restrict__ scale, InputGradMidOut o) {
    const int64_t per = (int64_t)g * (dp + 1);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * per) return;
    const int64_t i = idx / per;
    const int e = (int)(idx - i * per);
    const int b = e / (dp + 1), k = e - b * (dp + 1);
    double* __restrict__ dst = k == dp ? o.out[b] : o.gout[b];
    if (!dst || (k >= d && k < dp)) return;
    double s = 0.0;
    for (int js = 0; js < jsplit; ++js) s += part[(int64_t)js * nrows * per + idx];
    if (k == dp) dst[i * o.ldo] = vscale * s;
    else {
        const double gv = (scale ? o.gfac[b] * scale[k] : o.gfac[b]) * s;
        dst[i * o.ldg + k] = (o.add0 && b == 0) ? dst[i * o.ldg + k] + gv : gv;
    }
}

int launch_input_grad_mid_finish(cglb_ctx* c, const double* part, int64_t jsplit, int64_t nrows, int g, double vscale, const double* scale, const InputGradMidOut& o) {
    if (g < 1 || g > INPUT_GRAD_MID_SLOTS) return cglb_fail(c, CGLB_ERR_BAD_ARG, "slot count outside the mid-width input-gradient finish kernel's");
    const int64_t total = nrows * g * (c->Dh + 1);
    hipLaunchKernelGGL(input_grad_mid_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, part, (int)jsplit, nrows, g, c->Dh, c->D, vscale,
                       scale, o);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// the slots of one group of sg <= g columns of a product with S columns: column b at out + b (row stride ldo; NULL: no values) and gout + b d (row stride S d)
static InputGradMidOut input_grad_mid_columns(int sg, int d, double gfac, double* out, int64_t ldo, double* gout, int64_t S) {
    InputGradMidOut o;
    for (int b = 0; b < INPUT_GRAD_MID_SLOTS; ++b) {
        o.out[b] = (b < sg && out) ? out + b : nullptr;
        o.gout[b] = b < sg ? gout + (int64_t)b * d : nullptr;
        o.gfac[b] = gfac;
    }
    o.ldo = ldo;
    o.ldg = S * d;
    o.add0 = 0;
    return o;
}

int input_grad_mid_rows_per_block(const cglb_ctx* c) { return 256 / input_grad_mid_split(c->Dh); }
int input_grad_mid_width(const cglb_ctx* c) { return input_grad_mid_group(c->Dh); }

// one group of G columns for the rows (XhRow, nrows <= INPUT_GRAD_MID_ROWS)
template <int KIND, int DP>
static int cross_grad_mid_group(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int sg, double* out, int64_t ldo, double* gout,
                                int64_t S) {
    constexpr int SPLIT = input_grad_mid_split(DP), G = input_grad_mid_group(DP), B = 256 / SPLIT;
    const int64_t ncols = c->N;
    const int64_t bx = (nrows + B - 1) / B;
    int64_t jsplit = 0, jchunk = 0;
    row_slab_pair_split(c->kff_jsplit, bx, ncols, row_slab_slot_cap(nrows, G * (DP + 1)), true, &jsplit, &jchunk);
    CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nrows * G * (DP + 1) * sizeof(double)));
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((cross_grad_mid_kernel<KIND, DP, SPLIT, G, PREC>), dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream, XhRow,
                                             nrows, (const double*)c->Xh, Vi, ldv, ncols, jchunk, (double*)c->ig_part, (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    // delta_hot = ks hot (x*_k - x_jk) / l_k, so d kappa / d x*_k = -var h delta_hot / (l_k ks hot) = -var h delta_hot (ks / l_k) / (ks^2 hot)
    const double ks = cglb_kscale(c);
    return launch_input_grad_mid_finish(c, c->ig_part, jsplit, nrows, G, c->var, (const double*)c->wscale,
                                        input_grad_mid_columns(sg, c->D, -c->var / (ks * ks * cglb_hot_scale(c)), out, ldo, gout, S));
}

template <int KIND>
static int cross_grad_mid_kind(cglb_ctx* c, const double* xh, int64_t nr, const double* Vi, int64_t ldv, int sg, double* out, int64_t ldo, double* gout, int64_t S) {
    switch (c->Dh) {
        case 48: return cross_grad_mid_group<KIND, 48>(c, xh, nr, Vi, ldv, sg, out, ldo, gout, S);
        case 64: return cross_grad_mid_group<KIND, 64>(c, xh, nr, Vi, ldv, sg, out, ldo, gout, S);
        case 80: return cross_grad_mid_group<KIND, 80>(c, xh, nr, Vi, ldv, sg, out, ldo, gout, S);
        case 96: return cross_grad_mid_group<KIND, 96>(c, xh, nr, Vi, ldv, sg, out, ldo, gout, S);
    }
    return cglb_fail(c, CGLB_ERR_BAD_ARG, "unsupported mid width");
}

// launch_cross_grad's contract at mid widths: XhRow [nrows][Dh] hot rows (wide_prep_hot_rows).  Rows in blocks of INPUT_GRAD_MID_ROWS, columns in groups of
// input_grad_mid_group; a group never straddles an interleave block of 8, so any ldv that is a multiple of 8 serves
int launch_cross_grad_mid(cglb_ctx* c, const void* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo, double* gout) {
    if (!input_grad_mid_on(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the mid-width input-gradient cross product needs an fp64 context of 33 to 96 input dimensions with the options input_grad_mid and wide_reg on");
    if (S < 1 || ldv < S || (ldv % CROSS_MULTI_SP) || !gout || (out && ldo < S))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad column count, leading dimension or output of the input-gradient cross product");
    const int G = input_grad_mid_group(c->Dh);
    for (int64_t i0 = 0; i0 < nrows; i0 += INPUT_GRAD_MID_ROWS) {
        const int64_t nr = std::min<int64_t>(INPUT_GRAD_MID_ROWS, nrows - i0);
        const double* xh = (const double*)XhRow + i0 * c->Dh;
        for (int b0 = 0; b0 < S; b0 += G) {
            const int sg = std::min(G, S - b0);
            CGLB_DISPATCH_KIND(c->kind, CGLB_TRY((cross_grad_mid_kind<KIND>(c, xh, nr, Vi + b0, ldv, sg, out ? out + i0 * ldo + b0 : nullptr, ldo,
                                                                            gout + (i0 * S + b0) * c->D, S))));
        }
    }
    return CGLB_OK;
}

template <int DP>
static int feature_grad_mid_group(cglb_ctx* c, const double* X, int64_t nrows, const double* rec, int sub, int64_t F, int64_t jsplit, int64_t jchunk, unsigned bx) {
    constexpr int SPLIT = input_grad_mid_split(DP), G = input_grad_mid_group(DP);
    hipLaunchKernelGGL((feature_grad_mid_kernel<DP, SPLIT, G>), dim3(bx, (unsigned)jsplit), dim3(256), 0, c->stream, X, c->D, (const double*)(c->ft_par + c->D), nrows,
                       rec, (int)FEATURE_REC(c->Dp), sub, F, jchunk, (double*)c->ig_part);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// launch_feature_grad's contract at mid widths, from the records launch_feature_operand left (FEATURE_REC(D) doubles each, centre in c->ft_par).  X: dev
// [nrows][D] raw rows.  The feature rule (row_slab_feature_split) at this kernel's rows per block, capped by the slab
int launch_feature_grad_mid(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo, double* gout) {
    if (!input_grad_mid_on(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the mid-width input-gradient feature product needs an fp64 context of 33 to 96 input dimensions with the options input_grad_mid and wide_reg on");
    if (S < 1 || F < 1 || !gout || (out && ldo < S)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad feature count, column count or output of the input-gradient feature product");
    const int G = input_grad_mid_group(c->Dh), Dh = c->Dh;
    const double amp = std::sqrt(2.0 * c->var / (double)F);
    const int64_t rl = FEATURE_REC(c->Dp);
    const int64_t rb = input_grad_mid_rows_per_block(c);
    for (int64_t i0 = 0; i0 < nrows; i0 += INPUT_GRAD_MID_ROWS) {
        const int64_t nr = std::min<int64_t>(INPUT_GRAD_MID_ROWS, nrows - i0);
        const int64_t bx = (nr + rb - 1) / rb;
        int64_t jsplit = 0, jchunk = 0;
        row_slab_feature_split(rb, nr, F, row_slab_slot_cap(nr, G * (Dh + 1)), &jsplit, &jchunk);
        CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nr * G * (Dh + 1) * sizeof(double)));
        for (int b0 = 0; b0 < S; b0 += G) {
            const int sg = std::min(G, S - b0);
            const double* rec = c->ft_rec + (int64_t)(b0 / FEATURE_SP) * F * rl;
            switch (Dh) {
                case 48: CGLB_TRY(feature_grad_mid_group<48>(c, X + i0 * c->D, nr, rec, b0 % FEATURE_SP, F, jsplit, jchunk, (unsigned)bx)); break;
                case 64: CGLB_TRY(feature_grad_mid_group<64>(c, X + i0 * c->D, nr, rec, b0 % FEATURE_SP, F, jsplit, jchunk, (unsigned)bx)); break;
                case 80: CGLB_TRY(feature_grad_mid_group<80>(c, X + i0 * c->D, nr, rec, b0 % FEATURE_SP, F, jsplit, jchunk, (unsigned)bx)); break;
                case 96: CGLB_TRY(feature_grad_mid_group<96>(c, X + i0 * c->D, nr, rec, b0 % FEATURE_SP, F, jsplit, jchunk, (unsigned)bx)); break;
                default: return cglb_fail(c, CGLB_ERR_BAD_ARG, "unsupported mid width");
            }
            // the records hold omega / (2 pi l): the constant of every gradient component is -2 pi amp
            CGLB_TRY(launch_input_grad_mid_finish(c, c->ig_part, jsplit, nr, G, amp, nullptr,
                                                  input_grad_mid_columns(sg, c->D, -6.283185307179586476925286766559 * amp, out ? out + i0 * ldo + b0 : nullptr, ldo,
                                                                         gout + (i0 * S + b0) * c->D, (int64_t)S)));
        }
    }
    return CGLB_OK;
}
