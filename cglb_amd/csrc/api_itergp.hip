// The iterative exact-GP class of libcglb_hip.so (batched CG with Lanczos log-det; include/cglb_hip.h, "iterative exact GP"): its small kernels,
// helpers and C entry points, on top of the PCG loop and the preconditioner of cglb_api.hip (api_core.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "api_core.h"
#include "lanczos_host.h"
#include "slq_host.h"

namespace {

// ================================ iterative exact GP: batched CG with Lanczos log-det (include/cglb_hip.h) ================================
__global__ __launch_bounds__(256) void negate_kernel(const double* __restrict__ x, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = -x[i];
}
// U[b] = a_b V[b] with a_0 = a0 and a_b = a for the probe columns: the left vectors (alpha / 2, -a_i / (2 t)) of the gradient's bilinear forms
__global__ __launch_bounds__(256) void itergp_left_kernel(const double* __restrict__ V, int64_t n, int s, double a0, double a, double* __restrict__ U) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n * s) U[idx] = (idx < n ? a0 : a) * V[idx];
}
// out[0] = sum_i x_i (one block, fixed order)
__global__ __launch_bounds__(256) void vec_sum_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
    __shared__ double smem[16];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
    s = block_sum(s, smem);
    if (threadIdx.x == 0) out[0] = s;
}
// x += a (prediction mean);  out[b] = f - q[b] (prediction variance of one group of new points)
__global__ __launch_bounds__(256) void add_scalar_kernel(double* __restrict__ x, int64_t n, double a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += a;
}
__global__ void itergp_var_kernel(const double* __restrict__ q, int n, double f, double* __restrict__ out) {
    if ((int)threadIdx.x < n) out[threadIdx.x] = f - q[threadIdx.x];
}

// the scope of the class: what more than one column needs (one shard, one rank, the default bound), fp64, one target column, the stored panel
int require_itergp_ok(cglb_ctx* c) {
    CGLB_TRY(require_multi_ok(c));
    if (c->dtype != CGLB_F64)
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the iterative exact GP class needs an fp64 context (-t fp64): its Lanczos coefficients are differences of fp64 recurrences");
    if (c->p != 1) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the iterative exact GP class takes one target column");
    if (c->precond_mode != 0) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the iterative exact GP class needs the stored panel A (precond_mode 0): its probes are formed from it");
    if (c->M > c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the preconditioner rank (the context's m) must not exceed the number of training points");
    if (!c->have_data || !c->have_hypers) return cglb_fail(c, CGLB_ERR_STATE, "set_data and set_hypers must precede the iterative exact GP class");
    return CGLB_OK;
}

int itergp_mark(cglb_ctx* c, int k) {
    if (!c->it_ev[k]) HIP_CHECK(c, hipEventCreate(&c->it_ev[k]));
    HIP_CHECK(c, hipEventRecord(c->it_ev[k], c->stream));
    c->it_ev_last = k;
    return CGLB_OK;
}

// *value = ms from event a to event b, read once `last` (b, or an event recorded after it) has completed; 0 where the pair is not set
int event_pair_ms(cglb_ctx* c, bool set, hipEvent_t a, hipEvent_t b, hipEvent_t last, double* value) {
    *value = 0.0;
    if (!set) return CGLB_OK;
    float ms = 0.f;
    HIP_CHECK(c, hipEventSynchronize(last));
    HIP_CHECK(c, hipEventElapsedTime(&ms, a, b));
    *value = ms;
    return CGLB_OK;
}

// P = Q_ff + noise I under the current hyper-parameters: Z = the M greedily selected training points (the pivoted Cholesky of K_ff of rank M,
// kernels_select.hip, reading the scaled inputs set_hypers left), then the common terms of the Nystrom preconditioner
int itergp_common_terms(cglb_ctx* c) {
    {
        long long* chosen_dev = nullptr;
        double* trace_dev = nullptr;
        DevTemps tmp;
        CGLB_TRY(tmp.alloc(c, (void**)&chosen_dev, (size_t)c->M * sizeof(long long)));
        CGLB_TRY(tmp.alloc(c, (void**)&trace_dev, sizeof(double)));
        CGLB_TRY(launch_select_inducing(c, c->var, c->jitter, chosen_dev, c->Z, trace_dev));  // blocking
    }
    if (is_wide(c)) {
        CGLB_TRY(wide_after_hypers(c));
    } else {
        CGLB_TRY(launch_prep_scaled(c, c->Z, c->M, c->Zs, c->za));
        CGLB_TRY(launch_prep_scaled(c, c->Z, c->M, c->Zh, c->zah, true));
    }
    c->have_local = c->have_terms = false;
    return cglb_setup(c);
}

int itergp_reserve(cglb_ctx* c, int s, size_t eps_doubles) {
    const size_t col = (size_t)c->N * sizeof(double);
    CGLB_TRY(c->mem.reserve(c, &c->it_V, &c->it_V_cap, (size_t)s * col));
    CGLB_TRY(c->mem.reserve(c, &c->it_eps, &c->it_eps_cap, eps_doubles * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->it_scal, &c->it_scal_cap, (size_t)(c->D + 3 + s + 8) * sizeof(double)));
    CGLB_TRY(c->mem.alloc(c, &c->it_alpha, col));
    if (c->it_log.host_cap < s) {
        if (c->it_log.host_pap) (void)hipHostFree(c->it_log.host_pap);
        c->it_log.host_pap = nullptr; c->it_log.host_cap = 0;
        HIP_CHECK(c, hipHostMalloc((void**)&c->it_log.host_pap, (size_t)s * sizeof(double), hipHostMallocDefault));
        c->it_log.host_cap = s;
    }
    return CGLB_OK;
}

// alpha = K^-1 e at the tolerance of a predictive call, warm-started at the alpha of the last evaluation (both predictives)
int itergp_predict_alpha(cglb_ctx* c, double max_error, int max_cg_iter, multi_work* w) {
    const size_t col = (size_t)c->N * sizeof(double);
    CGLB_TRY(multi_reserve(c, 8, w));
    CGLB_TRY(itergp_reserve(c, 8, 0));
    if (!(c->it_valid && c->have_terms)) {  // no evaluation at the current data and hyper-parameters: the preconditioner first, alpha from zero
        CGLB_TRY(itergp_common_terms(c));
        HIP_CHECK(c, hipMemsetAsync(c->it_alpha, 0, col, c->stream));
    }
    CGLB_TRY(launch_sub_scalar(c, c->w_e, c->y, c->mean, c->N));
    CGLB_TRY(pcg_solve(c, fused_ops(c), c->w_e, c->it_alpha, max_error, max_cg_iter, 40, nullptr, nullptr));
    c->it_valid = true;
    return CGLB_OK;
}

// f_mean = mean + K_*f alpha; leaves the hot-scaled new points in pts
int itergp_predict_mean(cglb_ctx* c, const void* xnew, int64_t n_new, StagedPoints& pts, void* f_mean) {
    CGLB_TRY(pts.stage(xnew, true));                                           // hot units for the pair kernel
    CGLB_TRY(launch_cross_matvec(c, pts.xs, pts.xa, n_new, c->it_alpha, f_mean));  // K_*f alpha
    hipLaunchKernelGGL(add_scalar_kernel, dim3(grid1d_full(n_new)), dim3(256), 0, c->stream, (double*)f_mean, n_new, c->mean);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// ---- Lanczos variance cache (cglb_itergp_var_cache): fixed-order Gram-Schmidt kernels over the row-major [N][ld] basis ----
#define LANCZOS_QTW_ROWS 512
// part[blk][k] = sum over the rows of block blk of Q[i][k] w[i]: lane = column (coalesced along a row), the 4 waves interleave the rows and are
// added in fixed order
__global__ __launch_bounds__(256) void lanczos_qtw_kernel(const double* __restrict__ Q, int64_t ld, const double* __restrict__ w, int64_t n, int ncols,
                                                          double* __restrict__ part) {
    __shared__ double sm[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.y * 64 + lane;
    const int64_t i0 = (int64_t)blockIdx.x * LANCZOS_QTW_ROWS;
    const int64_t i1 = i0 + LANCZOS_QTW_ROWS < n ? i0 + LANCZOS_QTW_ROWS : n;
    double s = 0.0;
    if (k < ncols)
        for (int64_t i = i0 + wv; i < i1; i += 4) s = __builtin_fma(Q[i * ld + k], w[i], s);
    sm[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && k < ncols) part[(int64_t)blockIdx.x * ld + k] = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
}
// coef[k] = sum_blk part[blk][k] in block order
__global__ __launch_bounds__(256) void lanczos_qtw_sum_kernel(const double* __restrict__ part, int64_t nblk, int64_t ld, int ncols, double* __restrict__ coef) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncols) return;
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += part[b * ld + k];
    coef[k] = s;
}
// w[i] -= sum_k Q[i][k] coef[k]: a wave takes 16 rows in turn, lane = column, one wave sum per row
__global__ __launch_bounds__(256) void lanczos_sub_kernel(const double* __restrict__ Q, int64_t ld, const double* __restrict__ coef, int64_t n, int ncols,
                                                          double* __restrict__ w) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    for (int64_t i = r0; i < r0 + 16 && i < n; ++i) {
        double s = 0.0;
        for (int k = lane; k < ncols; k += 64) s = __builtin_fma(Q[i * ld + k], coef[k], s);
        s = wave_sum(s);
        if (lane == 0) w[i] -= s;
    }
}
// q = w / beta, also stored as column j of Q
__global__ __launch_bounds__(256) void lanczos_next_kernel(const double* __restrict__ w, double beta, int64_t n, double* __restrict__ q, double* __restrict__ Q,
                                                           int64_t ld, int j) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = w[i] / beta;
    q[i] = v;
    Q[i * ld + j] = v;
}
// R = Q L^-T in place, row by row: R_j = (Q_j - l_{j-1} R_{j-1}) / d_j
__global__ __launch_bounds__(256) void lanczos_factor_apply_kernel(double* __restrict__ Q, int64_t ld, int64_t n, int J, const double* __restrict__ d,
                                                                   const double* __restrict__ l) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double* __restrict__ row = Q + i * ld;
    double prev = 0.0;
    for (int j = 0; j < J; ++j) {
        const double r = (j > 0 ? row[j] - l[j - 1] * prev : row[j]) / d[j];
        row[j] = r;
        prev = r;
    }
}

// coef = Q[:, :ncols]^T w, then w -= Q[:, :ncols] coef
int lanczos_orthogonalise(cglb_ctx* c, int ncols, double* coef) {
    const int64_t N = c->N, ld = c->it_cache_ld;
    const int64_t nblk = (N + LANCZOS_QTW_ROWS - 1) / LANCZOS_QTW_ROWS;
    hipLaunchKernelGGL(lanczos_qtw_kernel, dim3((unsigned)nblk, (unsigned)((ncols + 63) / 64)), dim3(256), 0, c->stream, (const double*)c->it_cache, ld,
                       (const double*)c->it_lw, N, ncols, c->it_lpart);
    CGLB_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(lanczos_qtw_sum_kernel, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->it_lpart, nblk, ld, ncols, coef);
    CGLB_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(lanczos_sub_kernel, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, c->stream, (const double*)c->it_cache, ld, (const double*)coef, N, ncols,
                       c->it_lw);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

int itergp_cache_mark(cglb_ctx* c, int k) {
    if (!c->it_cev[k]) HIP_CHECK(c, hipEventCreate(&c->it_cev[k]));
    HIP_CHECK(c, hipEventRecord(c->it_cev[k], c->stream));
    return CGLB_OK;
}

// the scope of the cache: the class's own, at any width (wide inputs apply it through the Gram tiles of kernels_wide.hip)
int require_var_cache_ok(cglb_ctx* c) { return require_itergp_ok(c); }
// the scope of the register-resident multi-column cross product behind cglb_cross_matmat (kernels_cross_multi.hip)
int require_cross_multi_ok(cglb_ctx* c) {
    CGLB_TRY(require_itergp_ok(c));
    if (is_wide(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the register-resident multi-column cross product is available up to 32 input dimensions");
    return CGLB_OK;
}

// ---- pathwise posterior samples (cglb_itergp_sample) and the feature product under them (kernels_feature_multi.hip) ----
// B[s][i] = (y_i - mean) - G[i][s] - sn eps[s][i]: the right-hand sides of Matheron's rule, G row-major [n][S]
__global__ __launch_bounds__(256) void sample_rhs_kernel(const double* __restrict__ y, double mean, const double* __restrict__ G, const double* __restrict__ eps,
                                                         double sn, int64_t n, int S, double* __restrict__ B) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * S) return;
    const int64_t s = idx / n, i = idx - s * n;
    B[idx] = ((y[i] - mean) - G[i * S + s]) - sn * eps[idx];
}
// f[s][i] = (mean + G[i][s]) + KU(i, s), KU(i, s) at KU[i * ki + s * ks]
__global__ __launch_bounds__(256) void sample_combine_kernel(double mean, const double* __restrict__ G, const double* __restrict__ KU, int64_t ki, int64_t ks,
                                                             int64_t n, int S, double* __restrict__ f) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * S) return;
    const int64_t s = idx / n, i = idx - s * n;
    f[idx] = (mean + G[i * S + s]) + KU[i * ki + s * ks];
}

// the feature product of one call between the two events of "feature_ms"
int feature_product(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out) {
    for (int k = 0; k < 2; ++k)
        if (!c->ft_ev[k]) HIP_CHECK(c, hipEventCreate(&c->ft_ev[k]));
    c->ft_ev_set = false;
    HIP_CHECK(c, hipEventRecord(c->ft_ev[0], c->stream));
    CGLB_TRY(launch_feature_multi(c, X, nrows, F, S, out, S));
    HIP_CHECK(c, hipEventRecord(c->ft_ev[1], c->stream));
    c->ft_ev_set = true;
    return CGLB_OK;
}

// dst[0 .. n) = src[0 .. m) repeated (operands of a timed launch: values do not change a branch-free instruction stream)
int fill_cyclic(cglb_ctx* c, double* dst, int64_t n, const double* src, int64_t m) {
    for (int64_t o = 0; o < n; o += m)
        HIP_CHECK(c, hipMemcpyAsync(dst + o, src, (size_t)std::min(m, n - o) * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return CGLB_OK;
}

// the two halves of a pathwise sample, shared by cglb_itergp_sample and cglb_itergp_paths_solve / cglb_itergp_paths_eval
// buffers of the solve (w, it_V, it_eps, ft_G for max(N, rows_G) rows) and the preconditioner of the last evaluation at the current data and
// hyper-parameters; without one it is built first.  it_alpha and it_valid stay as they are: the next predictive call finds what it would have found
int sample_reserve(cglb_ctx* c, int S, int64_t rows_G, multi_work* w) {
    CGLB_TRY(multi_reserve(c, S, w));
    CGLB_TRY(itergp_reserve(c, S, (size_t)S * c->N));
    CGLB_TRY(c->mem.reserve(c, &c->ft_G, &c->ft_G_cap, (size_t)std::max(c->N, rows_G) * S * sizeof(double)));
    if (!(c->it_valid && c->have_terms)) CGLB_TRY(itergp_common_terms(c));
    return CGLB_OK;
}
// c->it_V <- U = K^-1 B, B_s = e - Phi(X) w_s - sqrt(noise) eps_s; leaves the operand records of (omega, phase, W) in c->ft_rec
int sample_solve(cglb_ctx* c, const multi_work& w, const void* omega, const void* phase, const void* W, const void* eps, int64_t F, int S, double max_error,
                 int max_cg_iter, int* st, double* half) {
    const int64_t N = c->N;
    const size_t col = (size_t)N * sizeof(double);
    CGLB_TRY(launch_feature_operand(c, omega, phase, W, F, S));
    CGLB_TRY(feature_product(c, (const double*)c->X, N, F, S, c->ft_G));
    HIP_CHECK(c, hipMemcpyAsync(c->it_eps, eps, (size_t)S * col, hipMemcpyDefault, c->stream));
    hipLaunchKernelGGL(sample_rhs_kernel, dim3(grid1d_full((int64_t)S * N)), dim3(256), 0, c->stream, (const double*)c->y, c->mean, (const double*)c->ft_G,
                       (const double*)c->it_eps, std::sqrt(c->noise), N, S, (double*)w.b);
    CGLB_LAUNCH_CHECK(c);
    // U = K^-1 B: one batched solve from zero, no restart steps, stopped on 1/2 sum_s r_s^T P^-1 r_s <= max_error
    HIP_CHECK(c, hipMemsetAsync(c->it_V, 0, (size_t)S * col, c->stream));
    if (S == 1) CGLB_TRY(pcg_solve(c, fused_ops(c), w.b, c->it_V, max_error, max_cg_iter, 0, st, half));
    else CGLB_TRY(pcg_solve(c, multi_ops(c, w, S), w.b, c->it_V, max_error, max_cg_iter, 0, st, half));
    return CGLB_OK;
}
// f_s = mean + Phi(X*) w_s + K_*f U_s through the value kernels, from the records in c->ft_rec and the solves U (dev [S][N]); pts: the
// caller's buffers for n_new points
int sample_eval(cglb_ctx* c, const void* xnew, int64_t n_new, StagedPoints& pts, const double* U, int64_t F, int S, void* f_out) {
    const int64_t N = c->N;
    CGLB_TRY(pts.stage(xnew, true));  // hot units for the pair kernels
    CGLB_TRY(feature_product(c, (const double*)pts.xr, n_new, F, S, c->ft_G));
    int64_t ki = S, ks = 1;
    if (is_wide(c)) {  // column by column, as the predictive mean of a wide context
        for (int s = 0; s < S; ++s) CGLB_TRY(launch_cross_matvec(c, pts.xs, pts.xa, n_new, U + (size_t)s * N, c->ft_KU + (size_t)s * n_new));
        ki = 1; ks = n_new;
    } else {
        int64_t ldv = 0;
        CGLB_TRY(launch_cross_multi_operand(c, U, S, &ldv));
        CGLB_TRY(launch_cross_multi(c, pts.xs, pts.xa, n_new, (const double*)c->cm_vi, ldv, S, c->ft_KU, S));
    }
    hipLaunchKernelGGL(sample_combine_kernel, dim3(grid1d_full((int64_t)S * n_new)), dim3(256), 0, c->stream, c->mean, (const double*)c->ft_G,
                       (const double*)c->ft_KU, ki, ks, n_new, S, (double*)f_out);
    CGLB_LAUNCH_CHECK(c);
    return CGLB_OK;
}

// the width part of the scope of every input-gradient entry: up to 32 input dimensions, or a mid-width context (33 .. 96, wide_reg on) with the option
// "input_grad_mid"
static int require_input_grad_width(cglb_ctx* c) {
    if (is_wide(c) && !input_grad_mid_on(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the input-gradient products have no wide path yet: they are available up to 32 input dimensions, and at 33 to 96 with the "
                                              "option input_grad_mid 1 (fp64, wide_reg on)");
    return CGLB_OK;
}
// cglb_cross_grad_matmat, its timer, cglb_itergp_predict_grad: the class's own scope and the cross product's width (kernels_input_grad.hip,
// kernels_input_grad_mid.hip)
int require_cross_grad_ok(cglb_ctx* c) {
    CGLB_TRY(require_itergp_ok(c));
    return require_input_grad_width(c);
}
// cglb_feature_grad_matmat, its timer, cglb_itergp_paths_solve / _eval: the class's own scope (the value kernels of cglb_itergp_sample run at any width)
// and the width of the two gradient products
int require_feature_grad_ok(cglb_ctx* c) {
    CGLB_TRY(require_itergp_ok(c));
    return require_input_grad_width(c);
}
// the rows launch_cross_grad takes (input_grad_row_stride(c) doubles each): the hot-scaled set as staged; on a mid-width context under "input_grad_mid" the hot
// set at width Dh, formed here from the staged raw rows (StagedPoints stages the plain scaled set alone on wide contexts)
int input_grad_rows(cglb_ctx* c, StagedPoints& pts, const void** rows) {
    if (input_grad_mid_on(c)) {
        CGLB_TRY(pts.stage_hot_mid());
        *rows = pts.xh;
    } else {
        *rows = pts.xs;
    }
    return CGLB_OK;
}

// cglb_grad_x_kff_multi, its timer, cglb_itergp_objective_and_grad_x: fp64, one rank, one target column, at most 32 input dimensions
// (kernels_train_input_grad.hip)
int require_train_input_grad_ok(cglb_ctx* c) {
    CGLB_TRY(require_multi_ok(c));
    if (c->dtype != CGLB_F64) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient needs an fp64 context (-t fp64): it has no fp32 path yet");
    if (c->p != 1) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient takes one target column");
    if (is_wide(c))
        return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient has no wide path yet: it is available up to 32 input dimensions");
    if (!train_input_grad_native(c)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient needs a single shard covering all rows on one rank");
    if (!c->have_data || !c->have_hypers) return cglb_fail(c, CGLB_ERR_STATE, "set_data and set_hypers must precede the training-input gradient");
    return CGLB_OK;
}

// ---- what the value entries and their input-gradient twins share ----
// the columns of the variance cache rounded up to the group width of the cross product
int cache_cols_padded(const cglb_ctx* c) {
    const int gw = cross_multi_width();
    return (c->it_cache_rank + gw - 1) / gw * gw;
}

// f_var = f - |R^T k_*|^2 for the hot-scaled points in pts: one multi-column product B = K_*f R over the r_pad padded columns of the cache into
// c->it_blk, then the row norms of the summed block
int itergp_cached_var(cglb_ctx* c, const StagedPoints& pts, int64_t n_new, int r_pad, void* f_var) {
    if (is_wide(c)) CGLB_TRY(wide_cross_multi(c, pts.xs, pts.xa, n_new, c->it_cache, c->it_cache_ld, r_pad, c->it_blk, r_pad));  // Gram tiles + one GEMM each
    else CGLB_TRY(launch_cross_multi(c, pts.xs, pts.xa, n_new, c->it_cache, c->it_cache_ld, r_pad, c->it_blk, r_pad));
    return launch_cross_multi_var(c, c->it_blk, n_new, r_pad, r_pad, (double*)f_var);
}

// cglb_cross_matmat / cglb_cross_grad_matmat after their checks: the new points in hot units (rows of the pair kernel), V interleaved into
// c->cm_vi, then product(pts, ldv)
template <typename F>
int cross_product(cglb_ctx* c, const void* xnew, int64_t n_new, const void* V, int S, F product) {
    if (n_new == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    StagedPoints pts(c);
    CGLB_TRY(pts.alloc(n_new, sizeof(double)));
    CGLB_TRY(pts.stage(xnew, true));
    int64_t ldv = 0;
    CGLB_TRY(launch_cross_multi_operand(c, V, S, &ldv));
    return product(pts, ldv);
}

// cglb_feature_matmat / cglb_feature_grad_matmat after their checks: the rows x staged as given (NULL: the training rows, nothing staged), the
// operand records, then product(rows).  The stream is idle on return, so the caller's omega and phase are its own again.
template <typename P>
int feature_rows_product(cglb_ctx* c, const void* x, int64_t n_rows, const void* omega, const void* phase, const void* W, int64_t F, int S, P product) {
    if (!x && n_rows != c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the feature product of the training rows (x NULL) has n_rows = n_total");
    if (n_rows == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    StagedPoints pts(c);
    if (x) {
        CGLB_TRY(pts.alloc(n_rows, sizeof(double), false));
        CGLB_TRY(pts.stage(x));
    }
    CGLB_TRY(launch_feature_operand(c, omega, phase, W, F, S));
    return product(x ? (const double*)pts.xr : (const double*)c->X);
}

// operands of the timed feature products: the training inputs as frequencies, the targets as phases and weights; out [n_rows][S]
int timed_feature_operands(cglb_ctx* c, DevTemps& tmp, int64_t n_rows, int64_t F, int S, void** om, void** ph, void** W, void** out) {
    CGLB_TRY(tmp.alloc(c, om, (size_t)F * c->D * sizeof(double)));
    CGLB_TRY(tmp.alloc(c, ph, (size_t)F * sizeof(double)));
    CGLB_TRY(tmp.alloc(c, W, (size_t)S * F * sizeof(double)));
    CGLB_TRY(tmp.alloc(c, out, (size_t)n_rows * S * sizeof(double)));
    CGLB_TRY(fill_cyclic(c, (double*)*om, F * c->D, (const double*)c->X, c->N * c->D));
    CGLB_TRY(fill_cyclic(c, (double*)*ph, F, (const double*)c->y, c->N));
    return fill_cyclic(c, (double*)*W, (int64_t)S * F, (const double*)c->y, c->N);
}

// step count and 1/2 r^T P r of a solve into the caller's optional slots
void put_solve_stats(int st, double half, int* steps, double* half_rz) {
    if (steps) *steps = st;
    if (half_rz) *half_rz = half;
}

}  // namespace

// "itergp_select_ms" | "itergp_solve_ms" | "itergp_grad_ms" of the last evaluation (0 for a phase it did not run), the statistics of the variance
// cache; -1: not one of these names
int itergp_stat(cglb_ctx* c, const char* name, double* value) {
    static const char* names[] = {"itergp_select_ms", "itergp_solve_ms", "itergp_grad_ms"};
    for (int k = 0; k < 3; ++k)
        if (!strcmp(name, names[k])) return event_pair_ms(c, c->it_ev_last > k, c->it_ev[k], c->it_ev[k + 1], c->it_ev[c->it_ev_last], value);
    // "itergp_cache_ms" | "itergp_var_ms": device time of the last cache build / of the variance part of the last cached predictive
    static const char* cnames[] = {"itergp_cache_ms", "itergp_var_ms"};
    for (int k = 0; k < 2; ++k)
        if (!strcmp(name, cnames[k])) return event_pair_ms(c, c->it_cev_set[k], c->it_cev[2 * k], c->it_cev[2 * k + 1], c->it_cev[2 * k + 1], value);
    if (!strcmp(name, "itergp_cache_request")) { *value = (double)c->it_cache_request; return CGLB_OK; }  // 0: no valid cache
    // "feature_ms": device time of the last feature product (pair kernel and slab sums of every group; not the operand records) of
    // cglb_feature_matmat or cglb_itergp_sample
    if (!strcmp(name, "feature_ms")) return event_pair_ms(c, c->ft_ev_set, c->ft_ev[0], c->ft_ev[1], c->ft_ev[1], value);
    return -1;
}

extern "C" {

// ---- iterative exact GP (include/cglb_hip.h) -----------------------------------------------------------------------------
// the one implementation of cglb_itergp_objective_and_grad (gx_out NULL) and cglb_itergp_objective_and_grad_x: gx_out, dev [N][D], comes from one
// further pass over the vectors of the kernel gradient, inside the "itergp_grad_ms" bracket; nothing else of the evaluation knows of it
static int itergp_objective(cglb_ctx* c, const void* eps, int t, void* v_inout, double max_error, int max_cg_iter, int lanczos_iter, double* out4, double* grad,
                            int* steps, double* half_rz, void* gx_out) {
    if (c) c->obj_valid = false;
    if (!c || !eps || !v_inout || !out4 || t < 1 || max_cg_iter < 0 || lanczos_iter < 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_itergp_ok(c));
    if (gx_out) CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    c->it_valid = false;
    c->it_ev_last = 0;
    const int64_t N = c->N;
    const int k = c->M, s = 1 + t, D = c->D;
    const size_t col = (size_t)N * sizeof(double);
    CGLB_TRY(itergp_mark(c, 0));
    CGLB_TRY(itergp_common_terms(c));
    CGLB_TRY(itergp_mark(c, 1));
    multi_work w;
    CGLB_TRY(multi_reserve(c, s, &w));
    CGLB_TRY(itergp_reserve(c, s, (size_t)t * (k + N)));
    HIP_CHECK(c, hipMemcpyAsync(c->it_eps, eps, (size_t)t * (k + N) * sizeof(double), hipMemcpyDefault, c->stream));
    // right-hand sides: e = y - mean, then the probes z_i = sqrt(s) (A^T eps_i[:k] + eps_i[k:]) through the A^T product of the preconditioner,
    // (r - A^T t) / s at r = eps_i[k:], t = -eps_i[:k], times s sqrt(s)
    CGLB_TRY(launch_sub_scalar(c, w.b, c->y, c->mean, N));
    for (int i = 0; i < t; ++i) {
        const double* ei = c->it_eps + (size_t)i * (k + N);
        hipLaunchKernelGGL(negate_kernel, dim3((k + 255) / 256), dim3(256), 0, c->stream, ei, k, (double*)c->w_t);
        CGLB_LAUNCH_CHECK(c);
        CGLB_TRY(launch_precond_z(c, ei + k, c->w_t, w.b + (size_t)(i + 1) * col, nullptr));
    }
    CGLB_TRY(launch_scale(c, w.b + col, c->noise * std::sqrt(c->noise), (int64_t)t * N));
    // one batched solve: column 0 warm-started, the probe columns from zero, no restart steps (a restart breaks the three-term recurrence)
    HIP_CHECK(c, hipMemcpyAsync(c->it_V, v_inout, col, hipMemcpyDeviceToDevice, c->stream));
    HIP_CHECK(c, hipMemsetAsync(c->it_V + N, 0, (size_t)t * col, c->stream));
    pcg_ops o = multi_ops(c, w, s);
    o.log = &c->it_log;
    int st = 0;
    double half = 0.0;
    CGLB_TRY(pcg_solve(c, o, w.b, c->it_V, max_error, max_cg_iter, 0, &st, &half));
    HIP_CHECK(c, hipMemcpyAsync(v_inout, c->it_V, col, hipMemcpyDeviceToDevice, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(c->it_alpha, c->it_V, col, hipMemcpyDeviceToDevice, c->stream));
    CGLB_TRY(itergp_mark(c, 2));
    // device scalars: [0, D] the kernel part of the gradient | [D + 1, D + 1 + s) u_b . v_b | e . alpha | sum alpha
    double* sc = c->it_scal;
    const int nsc = D + 3 + s;
    HIP_CHECK(c, hipMemsetAsync(sc, 0, (size_t)nsc * sizeof(double), c->stream));
    CGLB_TRY(launch_dot(c, w.b, c->it_V, N, sc + D + 1 + s));
    if (grad) {
        // right vectors in w.z: alpha and b_i = P^-1 z_i; left vectors in w.p: alpha / 2 and -a_i / (2 t)
        HIP_CHECK(c, hipMemcpyAsync(w.z, c->it_V, col, hipMemcpyDeviceToDevice, c->stream));
        for (int i = 1; i < s; ++i) CGLB_TRY(precond_single(c, w.b + (size_t)i * col, w.z + (size_t)i * col, c->scal + S_TMP));
        hipLaunchKernelGGL(itergp_left_kernel, dim3(grid1d_full((int64_t)s * N)), dim3(256), 0, c->stream, (const double*)c->it_V, N, s, 0.5, -0.5 / t,
                           (double*)w.p);
        CGLB_LAUNCH_CHECK(c);
        CGLB_TRY(launch_grad_kff_multi(c, w.p, w.z, s, sc));
        CGLB_TRY(launch_dot(c, w.p, w.z, N, sc + D + 1, s));
        hipLaunchKernelGGL(vec_sum_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->it_V, N, sc + D + 2 + s);
        CGLB_LAUNCH_CHECK(c);
        if (gx_out) CGLB_TRY(launch_grad_x_kff_multi(c, w.p, w.z, s, (double*)gx_out));  // the same pairs, differentiated in x_i
        CGLB_TRY(itergp_mark(c, 3));
    }
    std::vector<double> host((size_t)nsc);
    CGLB_TRY(read_scalars(c, sc, host.data(), nsc));
    // stochastic Lanczos quadrature on the host (csrc/slq_host.h)
    int status = 0;
    const double corr = slq_logdet_correction(c->it_log.rz.data(), c->it_log.pap.data(), st, t, lanczos_iter, &status);
    if (status != 0)
        return cglb_fail(c, CGLB_ERR_NOT_PD, status == 1 ? "Lanczos quadrature: the eigenvalue iteration did not converge"
                                                         : "Lanczos quadrature: a tridiagonal of the CG coefficients is not positive definite");
    const double logP = (double)N * std::log(c->noise) + 2.0 * c->sum_log_diag_LB;
    out4[1] = -0.5 * host[D + 1 + s];
    out4[2] = -0.5 * (logP + corr);
    out4[3] = logP;
    out4[0] = out4[1] + out4[2] - 0.5 * (double)N * std::log(2.0 * 3.14159265358979323846);
    if (grad) {
        for (int d = 0; d <= D; ++d) grad[d] = host[d];
        double gs = 0.0;
        for (int b = 0; b < s; ++b) gs += host[D + 1 + b];  // in column order
        grad[D + 1] = gs;
        grad[D + 2] = host[D + 2 + s];
    }
    put_solve_stats(st, half, steps, half_rz);
    c->it_steps = st;
    c->it_t = t;
    c->it_valid = true;
    return CGLB_OK;
}

int cglb_itergp_objective_and_grad(cglb_ctx* c, const void* eps, int t, void* v_inout, double max_error, int max_cg_iter, int lanczos_iter, double* out4,
                                   double* grad, int* steps, double* half_rz) {
    return itergp_objective(c, eps, t, v_inout, max_error, max_cg_iter, lanczos_iter, out4, grad, steps, half_rz, nullptr);
}

int cglb_itergp_objective_and_grad_x(cglb_ctx* c, const void* eps, int t, void* v_inout, double max_error, int max_cg_iter, int lanczos_iter, double* out4,
                                     double* grad, int* steps, double* half_rz, void* gx_out) {
    if (c && (!grad || !gx_out)) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the training-input gradient comes with the hyper-parameter gradient: grad and gx_out must be set");
    return itergp_objective(c, eps, t, v_inout, max_error, max_cg_iter, lanczos_iter, out4, grad, steps, half_rz, gx_out);
}

int cglb_itergp_get_coefficients(cglb_ctx* c, double* rz_log, double* pap_log) {
    if (!c || !rz_log || !pap_log) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "NULL argument") : CGLB_ERR_BAD_ARG;
    const size_t s = (size_t)1 + c->it_t;
    if (c->it_t < 1 || c->it_log.rz.size() != ((size_t)c->it_steps + 1) * s || c->it_log.pap.size() != (size_t)c->it_steps * s)
        return cglb_fail(c, CGLB_ERR_STATE, "cglb_itergp_get_coefficients must follow cglb_itergp_objective_and_grad");
    std::copy(c->it_log.rz.begin(), c->it_log.rz.end(), rz_log);
    std::copy(c->it_log.pap.begin(), c->it_log.pap.end(), pap_log);
    return CGLB_OK;
}

int cglb_itergp_predict(cglb_ctx* c, const void* xnew, int64_t n_new, double max_error, int max_cg_iter, void* f_mean, void* f_var) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !f_mean || !f_var || n_new < 0 || max_cg_iter < 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_itergp_ok(c));
    if (n_new == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    const int64_t N = c->N;
    const size_t col = (size_t)N * sizeof(double);
    multi_work w;
    CGLB_TRY(itergp_predict_alpha(c, max_error, max_cg_iter, &w));
    StagedPoints pts(c);
    CGLB_TRY(pts.alloc(n_new, sizeof(double)));
    CGLB_TRY(itergp_predict_mean(c, xnew, n_new, pts, f_mean));
    CGLB_TRY(pts.scale(false));                                                    // plain scaled units for the panel fill
    // f_var = f - k_*^T K^-1 k_*: batched solves on the columns of K_f*, 8 new points at a time (n_new / 8 solves)
    for (int64_t g0 = 0; g0 < n_new; g0 += 8) {
        const int sg = (int)std::min<int64_t>(8, n_new - g0);
        // the panel of the group's new points as its rows, the training rows as its column side
        CGLB_TRY(launch_kpanel(c, (const double*)pts.xs + g0 * c->Dp, sg, c->Xs, N, N, w.b));
        HIP_CHECK(c, hipMemsetAsync(c->it_V, 0, (size_t)sg * col, c->stream));
        if (sg == 1) CGLB_TRY(pcg_solve(c, fused_ops(c), w.b, c->it_V, max_error, max_cg_iter, 40, nullptr, nullptr));
        else CGLB_TRY(pcg_solve(c, multi_ops(c, w, sg), w.b, c->it_V, max_error, max_cg_iter, 40, nullptr, nullptr));
        CGLB_TRY(launch_dot(c, w.b, c->it_V, N, c->it_scal, sg));
        hipLaunchKernelGGL(itergp_var_kernel, dim3(1), dim3(64), 0, c->stream, (const double*)c->it_scal, sg, c->var, (double*)f_var + g0);
        CGLB_LAUNCH_CHECK(c);
    }
    return CGLB_OK;
}

int cglb_itergp_var_cache(cglb_ctx* c, int rank, int* rank_out) {
    if (c) c->obj_valid = false;
    if (!c || !rank_out) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    *rank_out = 0;
    CGLB_TRY(require_var_cache_ok(c));
    if (rank < 1 || rank > 1024 || rank > c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the rank of the variance cache must lie in 1 .. min(n_total, 1024)");
    HIP_CHECK(c, hipSetDevice(c->device));
    c->it_cache_rank = c->it_cache_request = 0;
    const int64_t N = c->N;
    const int gw = cross_multi_width(), ld = (rank + gw - 1) / gw * gw;
    const int64_t nblk = (N + LANCZOS_QTW_ROWS - 1) / LANCZOS_QTW_ROWS;
    CGLB_TRY(c->mem.reserve(c, &c->it_cache, &c->it_cache_cap, (size_t)N * ld * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->it_lq, &c->it_lq_cap, (size_t)N * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->it_lw, &c->it_lw_cap, (size_t)N * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->it_lc, &c->it_lc_cap, (size_t)(2 * ld + 2) * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->it_lpart, &c->it_lpart_cap, (size_t)nblk * ld * sizeof(double)));
    c->it_cache_ld = ld;
    c->it_cev_set[0] = false;
    CGLB_TRY(itergp_cache_mark(c, 0));
    HIP_CHECK(c, hipMemsetAsync(c->it_cache, 0, (size_t)N * ld * sizeof(double), c->stream));  // the padding columns stay zero
    double* coef = c->it_lc;          // [ld] first pass, [ld] second pass, then |w|^2
    double* norm2 = c->it_lc + 2 * ld;
    const unsigned gridn = (unsigned)((N + 255) / 256);
    // q_0 = e / |e|
    CGLB_TRY(launch_sub_scalar(c, c->it_lw, c->y, c->mean, N));
    CGLB_TRY(launch_dot(c, c->it_lw, c->it_lw, N, norm2));
    double e2 = 0.0;
    CGLB_TRY(read_scalars(c, norm2, &e2, 1));
    if (!(e2 > 0.0) || !std::isfinite(e2)) return cglb_fail(c, CGLB_ERR_STATE, "the variance cache starts its Lanczos run at y - mean, which is zero (or not finite)");
    hipLaunchKernelGGL(lanczos_next_kernel, dim3(gridn), dim3(256), 0, c->stream, (const double*)c->it_lw, std::sqrt(e2), N, c->it_lq, c->it_cache, (int64_t)ld, 0);
    CGLB_LAUNCH_CHECK(c);
    std::vector<double> alpha, beta;
    int J = 0;
    for (int j = 0; j < rank; ++j) {
        CGLB_TRY(launch_kff_matvec(c, c->it_lq, c->it_lw, nullptr));   // w = K q_j: the context's own mat-vec, noise included
        CGLB_TRY(lanczos_orthogonalise(c, j + 1, coef));               // two passes over all columns so far; coef[j] of the first is alpha_j
        CGLB_TRY(lanczos_orthogonalise(c, j + 1, coef + ld));
        CGLB_TRY(launch_dot(c, c->it_lw, c->it_lw, N, norm2));
        double aj = 0.0, b2 = 0.0;
        HIP_CHECK(c, hipMemcpyAsync(&aj, coef + j, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        CGLB_TRY(read_scalars(c, norm2, &b2, 1));
        const double bj = std::sqrt(b2);
        alpha.push_back(aj);
        beta.push_back(bj);
        J = j + 1;
        if (lanczos_stop(j, rank, bj, alpha[0])) break;
        hipLaunchKernelGGL(lanczos_next_kernel, dim3(gridn), dim3(256), 0, c->stream, (const double*)c->it_lw, bj, N, c->it_lq, c->it_cache, (int64_t)ld, j + 1);
        CGLB_LAUNCH_CHECK(c);
    }
    std::vector<double> diag, sub;
    if (lanczos_bidiag_factor(alpha.data(), beta.data(), J, diag, sub) != 0)
        return cglb_fail(c, CGLB_ERR_NOT_PD, "variance cache: the Lanczos tridiagonal is not positive definite");
    HIP_CHECK(c, hipMemcpyAsync(c->it_lc, diag.data(), (size_t)J * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(c->it_lc + ld, sub.data(), (size_t)J * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(lanczos_factor_apply_kernel, dim3(gridn), dim3(256), 0, c->stream, c->it_cache, (int64_t)ld, N, J, (const double*)c->it_lc,
                       (const double*)(c->it_lc + ld));
    CGLB_LAUNCH_CHECK(c);
    CGLB_TRY(itergp_cache_mark(c, 1));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));  // diag / sub are read until here
    c->it_cev_set[0] = true;
    c->it_cache_rank = J;
    c->it_cache_request = rank;
    *rank_out = J;
    return CGLB_OK;
}

int cglb_itergp_predict_cached(cglb_ctx* c, const void* xnew, int64_t n_new, double max_error, int max_cg_iter, void* f_mean, void* f_var) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !f_mean || !f_var || n_new < 0 || max_cg_iter < 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_var_cache_ok(c));
    if (c->it_cache_rank < 1) return cglb_fail(c, CGLB_ERR_STATE, "cglb_itergp_var_cache must precede cglb_itergp_predict_cached at the current data and hyper-parameters");
    if (n_new == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(itergp_predict_alpha(c, max_error, max_cg_iter, &w));
    const int r_pad = cache_cols_padded(c);
    CGLB_TRY(c->mem.reserve(c, &c->it_blk, &c->it_blk_cap, (size_t)n_new * r_pad * sizeof(double)));
    StagedPoints pts(c);
    CGLB_TRY(pts.alloc(n_new, sizeof(double)));
    CGLB_TRY(itergp_predict_mean(c, xnew, n_new, pts, f_mean));
    c->it_cev_set[1] = false;
    CGLB_TRY(itergp_cache_mark(c, 2));
    CGLB_TRY(itergp_cached_var(c, pts, n_new, r_pad, f_var));
    CGLB_TRY(itergp_cache_mark(c, 3));
    c->it_cev_set[1] = true;
    return CGLB_OK;
}

int cglb_cross_matmat(cglb_ctx* c, const void* xnew, int64_t n_new, const void* V, int S, void* out) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !V || !out || n_new < 0 || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_cross_multi_ok(c));
    return cross_product(c, xnew, n_new, V, S, [&](const StagedPoints& pts, int64_t ldv) {
        return launch_cross_multi(c, pts.xs, pts.xa, n_new, (const double*)c->cm_vi, ldv, S, (double*)out, S);
    });
}

int cglb_time_cross_matmat(cglb_ctx* c, int64_t n_new, int S, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0 || S == 0 || n_new < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_cross_multi_ok(c));
    if (n_new > c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the timed product takes its new points from the training rows: n_new <= n_total");
    HIP_CHECK(c, hipSetDevice(c->device));
    const int s = S < 0 ? -S : S;
    multi_work w;
    CGLB_TRY(multi_reserve(c, s, &w));
    void* out = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &out, (size_t)n_new * s * sizeof(double)));
    // operands: the first n_new training rows as new points, s copies of y as columns (values do not change the instruction stream)
    CGLB_TRY(fill_y_columns(c, w.p, s));
    const int rc = time_repeated(c, reps, [&]() -> int {
        if (S < 0) {  // the comparison side: s single products
            for (int b = 0; b < s; ++b) CGLB_TRY(launch_cross_matvec(c, c->Xh, c->xah, n_new, w.p + (size_t)b * c->N * c->esz, (double*)out + (size_t)b * n_new));
            return CGLB_OK;
        }
        int64_t ldv = 0;
        CGLB_TRY(launch_cross_multi_operand(c, w.p, s, &ldv));
        return launch_cross_multi(c, c->Xh, c->xah, n_new, (const double*)c->cm_vi, ldv, s, (double*)out, s);
    }, ms_avg);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int cglb_feature_matmat(cglb_ctx* c, const void* x, int64_t n_rows, const void* omega, const void* phase, const void* W, int64_t F, int S, void* out) {
    if (c) c->obj_valid = false;
    if (!c || !omega || !phase || !W || !out || n_rows < 0 || F < 1 || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_itergp_ok(c));
    return feature_rows_product(c, x, n_rows, omega, phase, W, F, S, [&](const double* rows) { return feature_product(c, rows, n_rows, F, S, (double*)out); });
}

int cglb_time_feature_matmat(cglb_ctx* c, int64_t n_rows, int64_t F, int S, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0 || S < 1 || F < 1 || n_rows < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_itergp_ok(c));
    if (n_rows > c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the timed product takes its rows from the training rows: n_rows <= n_total");
    HIP_CHECK(c, hipSetDevice(c->device));
    void *om = nullptr, *ph = nullptr, *W = nullptr, *out = nullptr;
    DevTemps tmp;
    int rc = timed_feature_operands(c, tmp, n_rows, F, S, &om, &ph, &W, &out);
    if (rc == CGLB_OK)
        rc = time_repeated(c, reps, [&]() -> int {
            CGLB_TRY(launch_feature_operand(c, om, ph, W, F, S));
            return launch_feature_multi(c, (const double*)c->X, n_rows, F, S, (double*)out, S);
        }, ms_avg);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int cglb_itergp_sample(cglb_ctx* c, const void* xnew, int64_t n_new, const void* omega, const void* phase, const void* W, const void* eps, int64_t F, int S,
                       double max_error, int max_cg_iter, void* f_out, void* U_out, int* steps, double* half_rz) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !omega || !phase || !W || !eps || !f_out || n_new < 0 || F < 1 || S < 1 || max_cg_iter < 0)
        return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_itergp_ok(c));
    if (n_new == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t col = (size_t)c->N * sizeof(double);
    multi_work w;
    CGLB_TRY(sample_reserve(c, S, n_new, &w));
    CGLB_TRY(c->mem.reserve(c, &c->ft_KU, &c->ft_KU_cap, (size_t)n_new * S * sizeof(double)));
    StagedPoints pts(c);  // the stream is idle on return: the caller's host arrays are its own again
    CGLB_TRY(pts.alloc(n_new, sizeof(double)));
    int st = 0;
    double half = 0.0;
    CGLB_TRY(sample_solve(c, w, omega, phase, W, eps, F, S, max_error, max_cg_iter, &st, &half));
    CGLB_TRY(sample_eval(c, xnew, n_new, pts, c->it_V, F, S, f_out));
    if (U_out) HIP_CHECK(c, hipMemcpyAsync(U_out, c->it_V, (size_t)S * col, hipMemcpyDeviceToDevice, c->stream));
    put_solve_stats(st, half, steps, half_rz);
    return CGLB_OK;
}

// ---- input gradients of predictive and sample paths (kernels_input_grad.hip) ------------------------------------------------------------------
int cglb_cross_grad_matmat(cglb_ctx* c, const void* xnew, int64_t n_new, const void* V, int S, void* out, void* gout) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !V || !gout || n_new < 0 || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_cross_grad_ok(c));
    return cross_product(c, xnew, n_new, V, S, [&](StagedPoints& pts, int64_t ldv) {
        const void* rows = nullptr;
        CGLB_TRY(input_grad_rows(c, pts, &rows));
        return launch_cross_grad(c, rows, n_new, (const double*)c->cm_vi, ldv, S, (double*)out, S, (double*)gout);
    });
}

int cglb_time_cross_grad_matmat(cglb_ctx* c, int64_t n_new, int S, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0 || S < 1 || n_new < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_cross_grad_ok(c));
    if (n_new > c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the timed product takes its new points from the training rows: n_new <= n_total");
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(multi_reserve(c, S, &w));
    void *out = nullptr, *gout = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &out, (size_t)n_new * S * sizeof(double)));
    CGLB_TRY(tmp.alloc(c, &gout, (size_t)n_new * S * c->D * sizeof(double)));
    // operands as cglb_time_cross_matmat forms them: the first n_new training rows as new points, S copies of y as columns
    CGLB_TRY(fill_y_columns(c, w.p, S));
    const int rc = time_repeated(c, reps, [&]() -> int {
        int64_t ldv = 0;
        CGLB_TRY(launch_cross_multi_operand(c, w.p, S, &ldv));
        return launch_cross_grad(c, c->Xh, n_new, (const double*)c->cm_vi, ldv, S, (double*)out, S, (double*)gout);
    }, ms_avg);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int cglb_feature_grad_matmat(cglb_ctx* c, const void* x, int64_t n_rows, const void* omega, const void* phase, const void* W, int64_t F, int S, void* out,
                             void* gout) {
    if (c) c->obj_valid = false;
    if (!c || !omega || !phase || !W || !gout || n_rows < 0 || F < 1 || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_feature_grad_ok(c));
    return feature_rows_product(c, x, n_rows, omega, phase, W, F, S,
                                [&](const double* rows) { return launch_feature_grad(c, rows, n_rows, F, S, (double*)out, S, (double*)gout); });
}

int cglb_time_feature_grad_matmat(cglb_ctx* c, int64_t n_rows, int64_t F, int S, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0 || S < 1 || F < 1 || n_rows < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_feature_grad_ok(c));
    if (n_rows > c->N) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the timed product takes its rows from the training rows: n_rows <= n_total");
    HIP_CHECK(c, hipSetDevice(c->device));
    void *om = nullptr, *ph = nullptr, *W = nullptr, *out = nullptr, *gout = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &gout, (size_t)n_rows * S * c->D * sizeof(double)));  // before the operands: nothing is enqueued yet if this fails
    int rc = timed_feature_operands(c, tmp, n_rows, F, S, &om, &ph, &W, &out);    // as cglb_time_feature_matmat forms them
    if (rc == CGLB_OK)
        rc = time_repeated(c, reps, [&]() -> int {
            CGLB_TRY(launch_feature_operand(c, om, ph, W, F, S));
            return launch_feature_grad(c, (const double*)c->X, n_rows, F, S, (double*)out, S, (double*)gout);
        }, ms_avg);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int cglb_itergp_predict_grad(cglb_ctx* c, const void* xnew, int64_t n_new, double max_error, int max_cg_iter, void* f_mean, void* g_mean, void* f_var,
                             void* g_var) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !f_mean || !g_mean || (!f_var) != (!g_var) || n_new < 0 || max_cg_iter < 0)
        return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_cross_grad_ok(c));
    if (f_var && c->it_cache_rank < 1)
        return cglb_fail(c, CGLB_ERR_STATE, "cglb_itergp_var_cache must precede cglb_itergp_predict_cached at the current data and hyper-parameters");
    if (n_new == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(itergp_predict_alpha(c, max_error, max_cg_iter, &w));
    const int r_pad = f_var ? cache_cols_padded(c) : 0;
    // the gradient block over the cache columns, a row block at a time: at most 2^23 doubles whatever n_new is
    const int64_t rows_blk = f_var ? std::max<int64_t>(1, std::min<int64_t>(n_new, ((int64_t)1 << 23) / ((int64_t)r_pad * c->D))) : 0;
    if (f_var) {
        CGLB_TRY(c->mem.reserve(c, &c->it_blk, &c->it_blk_cap, (size_t)n_new * r_pad * sizeof(double)));
        CGLB_TRY(c->mem.reserve(c, &c->ig_gk, &c->ig_gk_cap, (size_t)rows_blk * r_pad * c->D * sizeof(double)));
    }
    StagedPoints pts(c);
    CGLB_TRY(pts.alloc(n_new, sizeof(double)));
    CGLB_TRY(itergp_predict_mean(c, xnew, n_new, pts, f_mean));  // the mean of both predictives, bitwise
    // g_mean = grad (K_*f alpha): the stored alpha as the single column of the gradient product
    const void* rows = nullptr;
    CGLB_TRY(input_grad_rows(c, pts, &rows));
    int64_t ldv = 0;
    CGLB_TRY(launch_cross_multi_operand(c, c->it_alpha, 1, &ldv));
    CGLB_TRY(launch_cross_grad(c, rows, n_new, (const double*)c->cm_vi, ldv, 1, nullptr, 1, (double*)g_mean));
    if (!f_var) return CGLB_OK;
    // f_var as cglb_itergp_predict_cached forms it (B = K_*f R through the value kernel, bitwise), then g_var = -2 sum_s B G
    CGLB_TRY(itergp_cached_var(c, pts, n_new, r_pad, f_var));
    for (int64_t i0 = 0; i0 < n_new; i0 += rows_blk) {
        const int64_t nr = std::min(rows_blk, n_new - i0);
        CGLB_TRY(launch_cross_grad(c, (const double*)rows + i0 * input_grad_row_stride(c), nr, c->it_cache, c->it_cache_ld, r_pad, nullptr, r_pad, c->ig_gk));
        CGLB_TRY(launch_input_grad_var(c, c->it_blk + i0 * r_pad, r_pad, c->ig_gk, nr, r_pad, (double*)g_var + i0 * c->D));
    }
    return CGLB_OK;
}

int cglb_itergp_paths_solve(cglb_ctx* c, const void* omega, const void* phase, const void* W, const void* eps, int64_t F, int S, double max_error,
                            int max_cg_iter, void* U_out, int* steps, double* half_rz) {
    if (c) c->obj_valid = false;
    if (!c || !omega || !phase || !W || !eps || !U_out || F < 1 || S < 1 || max_cg_iter < 0)
        return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_feature_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(sample_reserve(c, S, 0, &w));
    StagedPoints none(c);  // no new points here: the caller's host arrays are read until the stream is idle, which it is on return
    int st = 0;
    double half = 0.0;
    CGLB_TRY(sample_solve(c, w, omega, phase, W, eps, F, S, max_error, max_cg_iter, &st, &half));
    HIP_CHECK(c, hipMemcpyAsync(U_out, c->it_V, (size_t)S * c->N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    put_solve_stats(st, half, steps, half_rz);
    return CGLB_OK;
}

int cglb_itergp_paths_eval(cglb_ctx* c, const void* xnew, int64_t n_new, const void* omega, const void* phase, const void* W, const void* U, int64_t F, int S,
                           void* f_out, void* g_out) {
    if (c) c->obj_valid = false;
    if (!c || !xnew || !omega || !phase || !W || !U || !f_out || n_new < 0 || F < 1 || S < 1)
        return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_feature_grad_ok(c));
    if (n_new == 0) return CGLB_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    CGLB_TRY(c->mem.reserve(c, &c->ft_G, &c->ft_G_cap, (size_t)n_new * S * sizeof(double)));
    CGLB_TRY(c->mem.reserve(c, &c->ft_KU, &c->ft_KU_cap, (size_t)n_new * S * sizeof(double)));
    if (g_out) {
        CGLB_TRY(c->mem.reserve(c, &c->ig_gk, &c->ig_gk_cap, (size_t)n_new * S * c->D * sizeof(double)));
        CGLB_TRY(c->mem.reserve(c, &c->ig_gf, &c->ig_gf_cap, (size_t)n_new * S * c->D * sizeof(double)));
    }
    StagedPoints pts(c);  // the stream is idle on return: the caller's host arrays are its own again
    CGLB_TRY(pts.alloc(n_new, sizeof(double)));
    CGLB_TRY(launch_feature_operand(c, omega, phase, W, F, S));
    if (!g_out) return sample_eval(c, xnew, n_new, pts, (const double*)U, F, S, f_out);  // the value kernels of cglb_itergp_sample, bitwise
    // values and gradients from the two fused passes
    CGLB_TRY(pts.stage(xnew, true));
    CGLB_TRY(launch_feature_grad(c, (const double*)pts.xr, n_new, F, S, c->ft_G, S, c->ig_gf));
    int64_t ldv = 0;
    CGLB_TRY(launch_cross_multi_operand(c, U, S, &ldv));
    const void* rows = nullptr;
    CGLB_TRY(input_grad_rows(c, pts, &rows));
    CGLB_TRY(launch_cross_grad(c, rows, n_new, (const double*)c->cm_vi, ldv, S, c->ft_KU, S, c->ig_gk));
    return launch_input_grad_paths(c, c->ft_G, c->ft_KU, c->ig_gf, c->ig_gk, n_new, S, (double*)f_out, (double*)g_out);
}

int cglb_grad_kff_multi(cglb_ctx* c, const void* U, const void* V, int S, double* out) {
    if (c) c->obj_valid = false;
    if (!c || !U || !V || !out || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_multi_ok(c));
    if (c->dtype != CGLB_F64) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the multi-pair gradient pass needs an fp64 context (-t fp64)");
    if (!c->have_hypers) return cglb_fail(c, CGLB_ERR_STATE, "set_hypers must precede cglb_grad_kff_multi");
    HIP_CHECK(c, hipSetDevice(c->device));
    CGLB_TRY(c->mem.reserve(c, &c->it_scal, &c->it_scal_cap, (size_t)(c->D + 1) * sizeof(double)));
    CGLB_TRY(launch_grad_kff_multi(c, U, V, S, c->it_scal));
    return read_scalars(c, c->it_scal, out, c->D + 1);
}

int cglb_grad_x_kff_multi(cglb_ctx* c, const void* U, const void* V, int S, void* gx_out) {
    if (c) c->obj_valid = false;
    if (!c || !U || !V || !gx_out || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    CGLB_TRY(launch_grad_x_kff_multi(c, U, V, S, (double*)gx_out));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return CGLB_OK;
}

int cglb_time_grad_x_kff_multi(cglb_ctx* c, int S, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0 || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(multi_reserve(c, S, &w));
    void* gx = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &gx, (size_t)c->N * c->D * sizeof(double)));
    CGLB_TRY(fill_y_columns(c, w.p, S));  // operands: S copies of y on both sides, as cglb_time_grad_kff_multi
    const int rc = time_repeated(c, reps, [&]() -> int { return launch_grad_x_kff_multi(c, w.p, w.p, S, (double*)gx); }, ms_avg);
    (void)hipStreamSynchronize(c->stream);  // before `tmp` frees
    return rc;
}

int cglb_grad_x_kff_pair(cglb_ctx* c, const void* u, const void* v, void* gx_out) {
    if (c) c->obj_valid = false;
    if (!c || !u || !v || !gx_out) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    CGLB_TRY(launch_grad_x_kff_pair(c, u, v, (double*)gx_out, 0));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return CGLB_OK;
}

int cglb_time_grad_x_kff_pair(cglb_ctx* c, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(multi_reserve(c, 1, &w));
    void* gx = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &gx, (size_t)c->N * c->D * sizeof(double)));
    CGLB_TRY(fill_y_columns(c, w.p, 1));  // operands: y on both sides, as cglb_time_grad_x_kff_multi(S = 1)
    const int rc = time_repeated(c, reps, [&]() -> int { return launch_grad_x_kff_pair(c, w.p, w.p, (double*)gx, 0); }, ms_avg);
    (void)hipStreamSynchronize(c->stream);  // before `tmp` frees
    return rc;
}

// the standalone transposed panel pass: the operand sets of the last set_hypers (the inducing points and lengthscales it was given), no common terms
int cglb_grad_x_kuf(cglb_ctx* c, const void* G, int64_t ldg, const void* cvec, const void* wvec, void* gx_out) {
    if (c) c->obj_valid = false;
    if (!c || !G || !gx_out) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    CGLB_TRY(launch_grad_x_kuf(c, G, ldg, cvec, wvec, (double*)gx_out));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return CGLB_OK;
}

int cglb_time_grad_x_kuf(cglb_ctx* c, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_train_input_grad_ok(c));
    HIP_CHECK(c, hipSetDevice(c->device));
    const int64_t ld = (c->N + 31) & ~(int64_t)31;
    void *G = nullptr, *cv = nullptr, *gx = nullptr;
    DevTemps tmp;
    CGLB_TRY(tmp.alloc(c, &G, (size_t)c->M * ld * sizeof(double)));  // operands: a panel of zeros with the rank-one term 0 y^T (values do not change the instruction stream)
    CGLB_TRY(tmp.alloc(c, &cv, (size_t)c->M * sizeof(double)));
    CGLB_TRY(tmp.alloc(c, &gx, (size_t)c->N * c->D * sizeof(double)));
    HIP_CHECK(c, hipMemsetAsync(G, 0, (size_t)c->M * ld * sizeof(double), c->stream));
    HIP_CHECK(c, hipMemsetAsync(cv, 0, (size_t)c->M * sizeof(double), c->stream));
    const int rc = time_repeated(c, reps, [&]() -> int { return launch_grad_x_kuf(c, G, ld, cv, c->y, (double*)gx); }, ms_avg);
    (void)hipStreamSynchronize(c->stream);  // before `tmp` frees
    return rc;
}

int cglb_time_grad_kff_multi(cglb_ctx* c, int S, int reps, double* ms_avg) {
    if (c) c->obj_valid = false;
    if (!c || !ms_avg || reps <= 0 || S < 1) return c ? cglb_fail(c, CGLB_ERR_BAD_ARG, "bad argument") : CGLB_ERR_BAD_ARG;
    CGLB_TRY(require_multi_ok(c));
    if (c->dtype != CGLB_F64) return cglb_fail(c, CGLB_ERR_BAD_ARG, "the multi-pair gradient pass needs an fp64 context (-t fp64)");
    if (!c->have_hypers) return cglb_fail(c, CGLB_ERR_STATE, "set_hypers must precede timing");
    HIP_CHECK(c, hipSetDevice(c->device));
    multi_work w;
    CGLB_TRY(multi_reserve(c, S, &w));
    CGLB_TRY(c->mem.reserve(c, &c->it_scal, &c->it_scal_cap, (size_t)(c->D + 1) * sizeof(double)));
    CGLB_TRY(fill_y_columns(c, w.p, S));  // operands: S copies of y on both sides
    return time_repeated(c, reps, [&]() -> int { return launch_grad_kff_multi(c, w.p, w.p, S, c->it_scal); }, ms_avg);
}

}  // extern "C"
