// Row-weighted value AND input gradient of a cross product at mid widths (32 < D <= 96, fp64; option "input_grad_mid"): weighted_grad_kernel's contract
// (kernels_predict_grad.hip) against any hot-unit point set Ph [npts][Dh],
//   out_u[i] =  f sum_m u[m]     kappa(x*_i, p_m)     gout_u[i, k] = -f sum_m u[m]     h_im delta_imk / l_k
//   out_w[i] =  f sum_m Wt[m, i] kappa(x*_i, p_m)     gout_w[i, k] = -f sum_m Wt[m, i] h_im delta_imk / l_k
// on the machine of cross_grad_mid_kernel (kernels_input_grad_mid.hip), with weight slots in the place of its group of columns:
//   * a new point is shared by SPLIT lanes (predict_grad_mid_split, row_slab.h): lane l of a wave holds part l / WROWS (HD = Dh / SPLIT coordinates) of row
//     l % WROWS, WROWS = 64 / SPLIT; a workgroup has 256 / SPLIT rows;
//   * a point's coordinates travel as NCH = HD / CH slice registers per lane and reach the arithmetic through v_fmac_f64 row_newbcast (BcastDiff); slice s
//     of the NEXT point is requested into the registers of slice s as soon as the differences have been taken;
//   * DIRECT differences; the per-lane partial of d2 runs in two interleaved chains and meets the other parts through sum_row_pairs / sum_halves - the same
//     sum in every part, bit for bit; ONE kappa_hfac_hot_from_d2 per pair (always the range-clamped 2^x: no exp_clamp instances), redundantly in the parts;
//   * NW x HD gradient accumulators and NW value accumulators per lane, NW = 2 or 1 by the template flags; per slot one multiply t = h w and HD fma
//     acc[b][k] += t delta_k, one fma for the value.  A coincident pair has delta = 0 exactly and adds exactly zero; the zero padding Dh - D of both
//     operands adds exactly zero to d2;
//   * weights: u[m] is a wave-uniform scalar load; Wt[m * ldw + row] (new-point index fastest, ldw >= nrows) is read by the lanes of a row, 64 / SPLIT
//     consecutive doubles per wave and point, and the next point's weight is requested before the current pair's profile;
//   * rows past nrows are clamped to the last row: they take part in every cross-lane operation, never read the padding columns [nrows, ldw) and
//     store nothing;
//   * the slabs, the split rule, the slot cap of row_slab.h: part[blockIdx.y][row][NW][Dh + 1] (part p writes its HD components, part 0 the value), the
//     cap that of the two-weight slab whichever instance runs, so the split never depends on NW and the u sums of the two-weight instance are the
//     operations of the one-weight instance: every output is bitwise the same whichever of the others are requested;
//   * the finish kernel of kernels_input_grad_mid.hip adds the slabs in fixed order and applies f, the constant -f wscale / (ks^2 hot) times the device
//     copy of ks / l_k, and add_u.  No atomics.
// The column loop has wave-uniform bounds and nothing in it is divergent.  Registers of every instance: DESIGN.md section 4i.
#include "pair_common.h"
#include "row_slab.h"

#if !defined(CGLB_PREDICT_GRAD_MID_M32) && !defined(CGLB_PREDICT_GRAD_MID_M52)
// out[i * dh + k] = (x[i * d + k] - centre_k) * (scale_k * hot), zero in the padding d .. dh - 1; cs: device [centre (d) | scale (d)] (the exact GPR class
// stages X and its batches at its own lengthscales; the operation order of wide_prep_hot_kernel)
__global__ __launch_bounds__(256) void hot_points_mid_kernel(const double* __restrict__ x, int64_t n, int d, int dh, const double* __restrict__ cs, double hot,
                                                             double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * dh) return;
    const int64_t i = idx / dh;
    const int k = (int)(idx - i * dh);
    out[idx] = k < d ? (x[i * d + k] - cs[k]) * (cs[d + k] * hot) : 0.0;
}
#endif

// grid (row blocks of 256 / SPLIT new points, chunks of jchunk points)
template <int KIND, int DH, int SPLIT, bool HAS_U, bool HAS_W, int PREC>
__global__ __launch_bounds__(256, 2) void weighted_grad_mid_kernel(const double* __restrict__ XhRow, int64_t nrows, const double* __restrict__ Ph, int64_t npts,
                                                                   const double* __restrict__ u, const double* __restrict__ Wt, int64_t ldw, int64_t jchunk,
                                                                   double* __restrict__ part, const double* __restrict__ exp_tab) {
    static_assert(HAS_U || HAS_W, "no weight");
    constexpr int NW = (HAS_U ? 1 : 0) + (HAS_W ? 1 : 0), IW = HAS_U ? 1 : 0;
    constexpr int HD = DH / SPLIT, CH = HD % 8 == 0 ? 8 : 4, NCH = HD / CH, WROWS = 64 / SPLIT;
    static_assert((SPLIT == 2 || SPLIT == 4) && DH % SPLIT == 0 && HD % CH == 0, "part width must be a multiple of 4");
    __shared__ double tab[CGLB_TAB_SIZE];
    load_exp_table(tab, exp_tab);
    const int lane = threadIdx.x & 63, prt = lane / WROWS;   // prt: which 1 / SPLIT of the dimensions this lane holds
    const int64_t row = (int64_t)blockIdx.x * (4 * WROWS) + (threadIdx.x >> 6) * WROWS + (lane & (WROWS - 1));
    const int64_t rr = row < nrows ? row : nrows - 1;
    double xi[HD], acc[NW][HD], val[NW];
#pragma unroll
    for (int d = 0; d < HD; ++d) xi[d] = XhRow[rr * DH + prt * HD + d];
    row_slab_zero(acc);
    row_slab_zero(val);
    double m1 = -1.0;
    asm volatile("" : "+v"(m1));   // the multiplier of the differences stays in one register pair
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < npts) ? j0 + jchunk : npts;
    const double* __restrict__ pcol = Ph + prt * HD + (lane & (CH - 1));   // + j * DH + CH s: this lane's element of slice s of point j
    const double* __restrict__ wrow = HAS_W ? Wt + rr : nullptr;           // + j * ldw: this row's weight of point j
    double xsl[NCH], wn = 0.0;
    if (j0 < j1) {
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) xsl[sl] = pcol[j0 * DH + sl * CH];
        if (HAS_W) wn = wrow[j0 * ldw];
    }
    for (int64_t j = j0; j < j1; ++j) {
        const int64_t jn = (j + 1 < j1) ? j + 1 : j;   // next point (or a harmless re-read)
        const double uj = HAS_U ? u[j] : 0.0;          // wave-uniform: one scalar load
        const double wj = wn;
        if (HAS_W) wn = wrow[jn * ldw];                // in flight during this pair's profile
        double df[HD];
        double d2 = 0.0, d2b = 0.0;
#pragma unroll
        for (int sl = 0; sl < NCH; ++sl) {
            BcastDiff<0, CH>::run(&df[sl * CH], xsl[sl], &xi[sl * CH], m1);
            xsl[sl] = pcol[jn * DH + sl * CH];
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
        if (HAS_U) {
            const double t = hv * uj;
#pragma unroll
            for (int k = 0; k < HD; ++k) acc[0][k] = __builtin_fma(t, df[k], acc[0][k]);
            val[0] = __builtin_fma(kv, uj, val[0]);
        }
        if (HAS_W) {
            const double t = hv * wj;
#pragma unroll
            for (int k = 0; k < HD; ++k) acc[IW][k] = __builtin_fma(t, df[k], acc[IW][k]);
            val[IW] = __builtin_fma(kv, wj, val[IW]);
        }
    }
    if (row < nrows) {   // after the last cross-lane operation: clamped rows store nothing
        double* __restrict__ o = part + ((int64_t)blockIdx.y * nrows + row) * (NW * (DH + 1));
#pragma unroll
        for (int b = 0; b < NW; ++b) {
#pragma unroll
            for (int k = 0; k < HD; ++k) o[b * (DH + 1) + prt * HD + k] = acc[b][k];
            if (prt == 0) o[b * (DH + 1) + DH] = val[b];
        }
    }
}

template <int KIND, int DH, bool HAS_U, bool HAS_W>
static int weighted_grad_mid_pairs(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw,
                                   unsigned bx, int64_t jsplit, int64_t jchunk) {
    constexpr int SPLIT = predict_grad_mid_split(DH);
    using T = double;
    CGLB_DISPATCH_PREC(c, hipLaunchKernelGGL((weighted_grad_mid_kernel<KIND, DH, SPLIT, HAS_U, HAS_W, PREC>), dim3(bx, (unsigned)jsplit), dim3(256), 0, c->stream,
                                             XhRow, nrows, Ph, npts, u, Wt, ldw, jchunk, (double*)c->ig_part, (const double*)c->exp_tab));
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

template <int KIND, int DH>
static int weighted_grad_mid_width(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw,
                                   unsigned bx, int64_t jsplit, int64_t jchunk) {
    if (u && Wt) return weighted_grad_mid_pairs<KIND, DH, true, true>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
    if (u) return weighted_grad_mid_pairs<KIND, DH, true, false>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
    return weighted_grad_mid_pairs<KIND, DH, false, true>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
}

template <int KIND>
static int weighted_grad_mid_kind(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw,
                                  unsigned bx, int64_t jsplit, int64_t jchunk) {
    switch (c->Dh) {
        case 48: return weighted_grad_mid_width<KIND, 48>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
        case 64: return weighted_grad_mid_width<KIND, 64>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
        case 80: return weighted_grad_mid_width<KIND, 80>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
        case 96: return weighted_grad_mid_width<KIND, 96>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
    }
    return cglb_fail(c, CGLB_ERR_BAD_ARG, "unsupported mid width");
}

#if defined(CGLB_PREDICT_GRAD_MID_M32)
int weighted_grad_mid_m32(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw, unsigned bx,
                          int64_t jsplit, int64_t jchunk) {
    return weighted_grad_mid_kind<CGLB_MATERN32>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
}
#elif defined(CGLB_PREDICT_GRAD_MID_M52)
int weighted_grad_mid_m52(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw, unsigned bx,
                          int64_t jsplit, int64_t jchunk) {
    return weighted_grad_mid_kind<CGLB_MATERN52>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, bx, jsplit, jchunk);
}
#else
int weighted_grad_mid_m32(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw, unsigned bx,
                          int64_t jsplit, int64_t jchunk);
int weighted_grad_mid_m52(cglb_ctx* c, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u, const double* Wt, int64_t ldw, unsigned bx,
                          int64_t jsplit, int64_t jchunk);

int predict_grad_mid_rows_per_block(const cglb_ctx* c) { return 256 / predict_grad_mid_split(c->Dh); }

// One block of nrows <= PREDICT_GRAD_ROWS rows of launch_weighted_grad on a context with input_grad_mid_on(c): XhRow [nrows][Dh] and Ph [npts][Dh] in hot
// units, scale: the device copy of ks / l_k at the lengthscales both sets were staged with, var the variance.  The outputs (any may be NULL) point at the
// block's first row
int launch_weighted_grad_mid(cglb_ctx* c, const double* scale, double var, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u,
                             const double* Wt, int64_t ldw, double* out_u, double* gout_u, bool add_u, double* out_w, double* gout_w, double wscale) {
    if (!input_grad_mid_on(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the mid-width row-weighted gradient product needs an fp64 context of 33 to 96 input dimensions with the options input_grad_mid and wide_reg on");
    if (!scale || (!u && !Wt) || npts < 1 || nrows < 1 || (Wt && ldw < nrows))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad weights, leading dimension or scales of the mid-width row-weighted gradient product");
    const int Dh = c->Dh, nw = (u ? 1 : 0) + (Wt ? 1 : 0), iw = u ? 1 : 0;
    const int64_t rb = predict_grad_mid_rows_per_block(c);
    const int64_t bx = (nrows + rb - 1) / rb;
    // capped by the slab of the two-weight instance whatever nw is
    int64_t jsplit = 0, jchunk = 0;
    row_slab_pair_split(c->kff_jsplit, bx, npts, row_slab_slot_cap(nrows, 2 * (Dh + 1)), true, &jsplit, &jchunk);
    CGLB_TRY(c->mem.reserve(c, &c->ig_part, &c->ig_part_cap, (size_t)jsplit * nrows * nw * (Dh + 1) * sizeof(double)));
    if (c->kind == CGLB_RBF) CGLB_TRY(weighted_grad_mid_kind<CGLB_RBF>(c, XhRow, nrows, Ph, npts, u, Wt, ldw, (unsigned)bx, jsplit, jchunk));
    else if (c->kind == CGLB_MATERN32) CGLB_TRY(weighted_grad_mid_m32(c, XhRow, nrows, Ph, npts, u, Wt, ldw, (unsigned)bx, jsplit, jchunk));
    else if (c->kind == CGLB_MATERN52) CGLB_TRY(weighted_grad_mid_m52(c, XhRow, nrows, Ph, npts, u, Wt, ldw, (unsigned)bx, jsplit, jchunk));
    else return cglb_fail(c, CGLB_ERR_BAD_ARG, "unsupported kernel kind");
    // delta_hot = ks hot (x*_k - p_mk) / l_k, so d kappa / d x*_k = -var h delta_hot (ks / l_k) / (ks^2 hot) (cross_grad_mid_group), times the slot's factor
    const double ks = cglb_kscale(c);
    const double gfac = -var / (ks * ks * cglb_hot_scale(c));
    InputGradMidOut o;
    for (int b = 0; b < INPUT_GRAD_MID_SLOTS; ++b) { o.out[b] = o.gout[b] = nullptr; o.gfac[b] = gfac; }
    o.ldo = 1;
    o.ldg = c->D;
    o.add0 = (int)(add_u && u);
    if (u) { o.out[0] = out_u; o.gout[0] = gout_u; }
    if (Wt) { o.out[iw] = out_w; o.gout[iw] = gout_w; o.gfac[iw] = wscale * gfac; }
    return launch_input_grad_mid_finish(c, c->ig_part, jsplit, nrows, nw, var, scale, o);
}

// out [n][Dh] <- x (dev [n][D]) in hot units; cs: device [centre (D) | ks / l_k (D)]
int launch_hot_points_mid(cglb_ctx* c, const double* cs, const double* x, int64_t n, double* out) {
    if (n == 0) return CGLB_OK;
    if (c->Dh == 0) return cglb_fail(c, CGLB_ERR_BAD_ARG, "no mid-width hot operand set on this context");
    hipLaunchKernelGGL(hot_points_mid_kernel, dim3((unsigned)((n * c->Dh + 255) / 256)), dim3(256), 0, c->stream, x, n, c->D, c->Dh, cs, cglb_hot_scale(c), out);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// c->Zhm [M][Dh]: the inducing points in hot units at the context's lengthscales, for the row-weighted product of a mid-width context.  Built on the first
// call after set_hypers / set_data that needs it (the device copies of centre and scale are current after set_hypers)
int predict_grad_mid_inducing(cglb_ctx* c) {
    if (c->Zhm && c->Zhm_valid) return CGLB_OK;
    void* zah = nullptr;  // |zh|^2 term of the Gram form: written by the kernel, not read by the direct-difference product
    DevTemps tmp;
    CGLB_TRY(c->mem.alloc(c, &c->Zhm, (size_t)c->M * c->Dh * sizeof(double)));
    CGLB_TRY(tmp.alloc(c, &zah, (size_t)c->M * sizeof(double)));
    CGLB_TRY(wide_prep_hot_rows(c, c->Z, c->M, c->Zhm, zah));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));  // before `tmp` frees
    c->Zhm_valid = true;
    return CGLB_OK;
}
#endif
