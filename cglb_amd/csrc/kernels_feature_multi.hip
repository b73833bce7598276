// Random-Fourier-feature product  out[i, s] = sqrt(2 var / F) * sum_{j < F} W[s, j] cos( sum_k omega[j, k] (x_ik - c_k) / l_k + b_j ):  the prior
// term Phi(.) w of a pathwise posterior sample (cglb_itergp_sample; Wilson et al. 2020), exposed on its own as cglb_feature_matmat.  The N x F
// feature matrix is never formed: every cosine is evaluated ONCE per group of 8 columns and consumed from a register.
//
// A row-slab product (row_slab.h) with a feature in the place of a training point: a lane keeps x_i - c and R x 8 accumulators; feature j's
// operand record
//   { b_j / 2 pi | omega_j[k] / (2 pi l_k), k < DP (zero padded) | W[8 g .. 8 g + 7, j] }          (FEATURE_REC(DP) doubles, one record per group g)
// is ONE contiguous run of scalar loads; the feature range is split by row_slab_feature_split; slab [jsplit][nrows][8].  S > 8 runs in groups of
// 8; a short group reads the zero padding of its records.
// The records are in TURNS, so the range reduction of cos_turns (devmath.h) is exact at any magnitude.  Per (row, feature, group): DP fma for the
// phase, 14 for the cosine, 8 for the columns.  Instances: the padded widths of dispatch.h (rows register-resident) and ONE looping instance
// for wider inputs, which reads x_ik in the k-loop (once per batch of 16 features, whose phases it advances together) and keeps the
// scalar-side features.  Register use of every instance: DESIGN.md section 4g.
#include "pair_common.h"
#include "row_slab.h"

// rows per lane: the rule of cross_multi_rows_per_lane (4 up to padded width 8, 2 up to 16, 1 beyond, halved while the R (DP + 8) row-resident
// doubles exceed 64, half of the 256 VGPRs): a row keeps DP centred coordinates and 8 accumulators here as there, and no seed
static constexpr int feature_rows_per_lane(int dp) {
    int r = dp <= 8 ? 4 : (dp <= 16 ? 2 : 1);
    while (r > 1 && r * (dp + FEATURE_SP) > 64) r /= 2;
    return r;
}

// rec[g][j] = { phase[j] / 2 pi | omega[j][k] * inv[k], k < d; 0, d <= k < dp | W[8 g + b][j], 8 g + b < S; 0 beyond }.  inv[k] = 1 / (2 pi l_k) and
// 1 / 2 pi are rounded once on the host: a coordinate term carries three roundings (inv, this product, x - c), the phase term two
__global__ __launch_bounds__(256) void feature_operand_kernel(const double* __restrict__ omega, const double* __restrict__ phase, const double* __restrict__ W,
                                                              const double* __restrict__ inv, double inv2pi, int d, int dp, int64_t F, int S, int groups,
                                                              double* __restrict__ rec) {
    const int rl = FEATURE_REC(dp);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)groups * F * rl) return;
    const int64_t gj = idx / rl;
    const int e = (int)(idx - gj * rl);
    const int g = (int)(gj / F);
    const int64_t j = gj - (int64_t)g * F;
    double v = 0.0;
    if (e == 0) v = phase[j] * inv2pi;
    else if (e <= d) v = omega[j * d + (e - 1)] * inv[e - 1];
    else if (e > dp && e <= dp + FEATURE_SP) {
        const int b = g * FEATURE_SP + (e - dp - 1);
        if (b < S) v = W[(int64_t)b * F + j];
    }
    rec[idx] = v;
}

// grid (row blocks of 256 R rows, feature chunks of jchunk); rec points at the first record of the group
template <int DP, int R>
__global__ __launch_bounds__(256) void feature_multi_kernel(const double* __restrict__ X, int d, RowSlabCentre cen, int64_t nrows, const double* __restrict__ rec,
                                                            int64_t F, int64_t jchunk, double* __restrict__ part) {
    constexpr int SP = FEATURE_SP, RL = FEATURE_REC(DP);
    const int64_t rbase = (int64_t)blockIdx.x * (256 * R) + threadIdx.x;
    double z[R][DP], acc[R][SP];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int64_t row = row_slab_clamped(rbase, k, nrows);
#pragma unroll
        for (int q = 0; q < DP; ++q) z[k][q] = q < d ? X[row * d + q] - cen.c[q] : 0.0;
        row_slab_zero(acc[k]);
    }
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < F) ? j0 + jchunk : F;
    for (int64_t j = j0; j < j1; ++j) {
        const double* __restrict__ rj = rec + j * RL;  // wave-uniform: one run of scalar loads
        double om[DP], wj[SP];
        const double bj = rj[0];
#pragma unroll
        for (int q = 0; q < DP; ++q) om[q] = rj[1 + q];
#pragma unroll
        for (int b = 0; b < SP; ++b) wj[b] = rj[1 + DP + b];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            double ph = bj;
#pragma unroll
            for (int q = 0; q < DP; ++q) ph = __builtin_fma(z[k][q], om[q], ph);
            const double cv = cos_turns(ph);
#pragma unroll
            for (int b = 0; b < SP; ++b) acc[k][b] = __builtin_fma(cv, wj[b], acc[k][b]);
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) row_slab_store(part, nrows, rbase + (int64_t)k * 256, acc[k]);
}

// the looping instance (d > 32): one row per lane, its coordinates read in the k-loop - once per FEATURE_LOOP_JC features, whose phases advance
// together in registers (a coordinate costs a strided vector load: read per feature, the loads were 50 times the arithmetic); the features stay
// on the scalar side.  A short last batch re-reads the chunk's last record with its cosine replaced by 0.  cen: device [d]; records of
// FEATURE_REC(d) doubles
#define FEATURE_LOOP_JC 16
__global__ __launch_bounds__(256) void feature_multi_loop_kernel(const double* __restrict__ X, int d, const double* __restrict__ cen, int64_t nrows,
                                                                 const double* __restrict__ rec, int64_t F, int64_t jchunk, double* __restrict__ part) {
    constexpr int SP = FEATURE_SP, JC = FEATURE_LOOP_JC;
    const int rl = FEATURE_REC(d);
    const int64_t row0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double* __restrict__ xi = X + (row0 < nrows ? row0 : nrows - 1) * d;  // one row per lane: the clamp of row_slab_clamped
    double acc[SP];
    row_slab_zero(acc);
    const int64_t j0 = (int64_t)blockIdx.y * jchunk;
    const int64_t j1 = (j0 + jchunk < F) ? j0 + jchunk : F;
    for (int64_t jb = j0; jb < j1; jb += JC) {
        const double* rj[JC];  // wave-uniform, as cen
        double ph[JC];
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) {
            rj[jj] = rec + (jb + jj < j1 ? jb + jj : j1 - 1) * rl;
            ph[jj] = rj[jj][0];
        }
        for (int q = 0; q < d; ++q) {
            const double zq = xi[q] - cen[q];
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) ph[jj] = __builtin_fma(zq, rj[jj][1 + q], ph[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) {
            const double cv = jb + jj < j1 ? cos_turns(ph[jj]) : 0.0;
#pragma unroll
            for (int b = 0; b < SP; ++b) acc[b] = __builtin_fma(cv, rj[jj][1 + d + b], acc[b]);
        }
    }
    row_slab_store(part, nrows, row0, acc);
}

int feature_rows_per_block(const cglb_ctx* c) { return is_wide(c) ? 256 : 256 * feature_rows_per_lane(c->Dp); }

// c->ft_rec <- the records of (omega, phase, W) at the current lengthscales, c->ft_par <- {1 / (2 pi l_k), c_k}.  omega [F][d] and phase [F]: host or
// device; W: dev [S][F]
int launch_feature_operand(cglb_ctx* c, const void* omega, const void* phase, const void* W, int64_t F, int S) {
    const int d = c->D, dp = c->Dp, groups = (S + FEATURE_SP - 1) / FEATURE_SP;
    const int64_t nrec = (int64_t)groups * F * FEATURE_REC(dp);
    CGLB_TRY(c->mem.reserve(c, &c->ft_rec, &c->ft_rec_cap, (size_t)nrec * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->ft_in, &c->ft_in_cap, (size_t)F * (d + 1) * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->ft_par, &c->ft_par_cap, (size_t)2 * d * sizeof(double)));
    const long double two_pi = 6.283185307179586476925286766559L;
    c->ft_host.resize((size_t)2 * d);  // a member: the asynchronous copy below reads it after this function has returned
    for (int k = 0; k < d; ++k) {
        c->ft_host[k] = (double)(1.0L / (two_pi * (long double)c->ls[k]));
        c->ft_host[d + k] = c->xmean[k];
    }
    HIP_CHECK(c, hipStreamSynchronize(c->stream));  // an earlier copy out of ft_host has completed
    HIP_CHECK(c, hipMemcpyAsync(c->ft_par, c->ft_host.data(), (size_t)2 * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(c->ft_in, omega, (size_t)F * d * sizeof(double), hipMemcpyDefault, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(c->ft_in + F * d, phase, (size_t)F * sizeof(double), hipMemcpyDefault, c->stream));
    hipLaunchKernelGGL(feature_operand_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->ft_in,
                       (const double*)(c->ft_in + F * d), (const double*)W, (const double*)c->ft_par, (double)(1.0L / two_pi), d, dp, F, S, groups, c->ft_rec);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

template <int DP>
static int feature_group(cglb_ctx* c, const double* X, int64_t nrows, const double* rec, int64_t F, int64_t jsplit, int64_t jchunk, unsigned bx) {
    constexpr int R = feature_rows_per_lane(DP);
    hipLaunchKernelGGL((feature_multi_kernel<DP, R>), dim3(bx, (unsigned)jsplit), dim3(256), 0, c->stream, X, c->D, row_slab_centre(c), nrows, rec, F, jchunk,
                       c->ft_part);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// out[i * ldo + s] = sqrt(2 var / F) sum_j W[s][j] cos(phase of row i and feature j), s < S <= ldo, from the records launch_feature_operand left.
// X: dev [nrows][D] raw rows (the training rows: c->X)
int launch_feature_multi(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo) {
    if (c->dtype != CGLB_F64) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the feature product needs an fp64 context");
    if (S < 1 || F < 1 || ldo < S) return cglb_fail(c, CGLB_ERR_BAD_ARG, "bad feature count, column count or leading dimension of the feature product");
    if (nrows == 0) return CGLB_OK;
    int64_t jsplit = 0, jchunk = 0;
    const int64_t rb = feature_rows_per_block(c), bx = (nrows + rb - 1) / rb;
    row_slab_feature_split(rb, nrows, F, ROW_SLAB_SLOTS, &jsplit, &jchunk);
    if (bx > 0x7fffffffLL) return cglb_fail(c, CGLB_ERR_BAD_ARG, "too many rows for one launch of the feature product");
    CGLB_TRY(c->mem.reserve(c, &c->ft_part, &c->ft_part_cap, (size_t)jsplit * nrows * FEATURE_SP * sizeof(double)));
    const double amp = std::sqrt(2.0 * c->var / (double)F);
    const int64_t rl = FEATURE_REC(c->Dp);
    for (int b0 = 0; b0 < S; b0 += FEATURE_SP) {
        const int sg = std::min(FEATURE_SP, S - b0);
        const double* rec = c->ft_rec + (int64_t)(b0 / FEATURE_SP) * F * rl;
        if (is_wide(c)) {
            hipLaunchKernelGGL(feature_multi_loop_kernel, dim3((unsigned)bx, (unsigned)jsplit), dim3(256), 0, c->stream, X, c->D,
                               (const double*)(c->ft_par + c->D), nrows, rec, F, jchunk, c->ft_part);
            CGLB_LAUNCH_CHECK(c);
        } else {
            CGLB_DISPATCH_DP(c->Dp, CGLB_TRY((feature_group<DP>(c, X, nrows, rec, F, jsplit, jchunk, (unsigned)bx))));
        }
        CGLB_TRY(row_slab_finish<FEATURE_SP>(c, (const double*)c->ft_part, jsplit, nrows, sg, amp, out + b0, ldo));
    }
    return CGLB_OK;
}
