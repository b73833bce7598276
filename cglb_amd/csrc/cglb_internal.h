// Internal declarations shared by the translation units of libcglb_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/cglb_hip.h"
#include "pair_worklist.h"

#define CGLB_MAX_D 1024        // widest input the context accepts (host-side arrays)
#define CGLB_MAX_D_NARROW 32   // widest input of the register-resident pair kernels; beyond it the "wide" path runs (kernels_wide.hip)
#define CGLB_MAX_D_MID 96     // ... except the symmetric K_ff mat-vec (fp64): up to here it still runs register-resident, the Gram chain in 16-wide slices
#define CGLB_WAVE 64

// Device memory of a context.  A pool owns the device buffers whose pointers sit in fields ("slots") of cglb_ctx / cglb_comm_state: both are
// heap objects that are never copied, so the pool keeps the addresses of the fields it has filled and release() frees exactly those.
// A new buffer needs a field and one alloc / reserve call; nothing else names it.  Defined in cglb_api.hip.
struct cglb_ctx;
struct cglb_devpool {
    struct entry { void** slot; size_t* cap; };
    std::vector<entry> entries;
    int alloc(cglb_ctx* c, void** slot, size_t bytes);                   // fixed size, eager or on first use: nothing if *slot is set
    int reserve(cglb_ctx* c, void** slot, size_t* cap, size_t need);     // grow-only: nothing if *slot holds `need` bytes already
    hipError_t drop(void** slot, size_t* cap = nullptr);                 // frees one buffer now: *slot = nullptr, *cap = 0
    void release();                                                      // ... and every buffer the pool has handed out
    template <typename P> int alloc(cglb_ctx* c, P** slot, size_t bytes) { return alloc(c, (void**)slot, bytes); }
    template <typename P> int reserve(cglb_ctx* c, P** slot, size_t* cap, size_t need) { return reserve(c, (void**)slot, cap, need); }
};

// Collectives of the N-rank path inside the library (cglb_comm_init_*, cglb_dist_*; include/cglb_hip.h): RCCL on the context stream, or
// host-provided callbacks (the same loop over another fabric, e.g. gloo in the tests).
struct cglb_comm_state {
    int kind = 0;  // 1 RCCL, 2 host callbacks
    int world = 1, rank = 0;
    int64_t per = 0;       // rows per rank of the contiguous panel partition, ceil(N / world)
    void* nccl = nullptr;  // ncclComm_t
    cglb_allreduce_fn ar = nullptr;
    cglb_allgather_fn ag = nullptr;
    void* user = nullptr;
    // replicated full-length work vectors (element type T) and gather buffers
    void *p = nullptr, *r = nullptr, *Ap = nullptr, *Kv = nullptr, *b = nullptr;  // [N]
    void* zseg = nullptr;   // [world * (per + 1)]: all-gather target of z with each rank's partial of r^T z
    void* ubuf = nullptr;   // [world * per]: all-gather target of u = w + v/2 (gradient phase)
    void *u = nullptr, *aw = nullptr;  // [M]
    double* sc = nullptr;   // [8]
    double* grad = nullptr; // [GRAD_LEN]
    void* gat = nullptr;    // prediction gather buffer
    size_t gat_cap = 0;
    long long n_allreduce = 0, n_allgather = 0;  // collectives issued since cglb_comm_init (cglb_get_stat)
    cglb_devpool mem;      // owns every device buffer above; released by comm_free
};

// Per-iteration scalars of a solve, kept for the Lanczos quadrature of the iterative exact-GP class (cglb_api.hip: pcg_solve fills the log its
// pcg_ops names; csrc/slq_host.h reads it): rz [steps + 1][s], pap [steps][s], column b of iteration j at [j * s + b].
struct pcg_log {
    std::vector<double> rz, pap;
    double* host_pap = nullptr;  // [s] pinned host mirror of the p.Ap scalars of one iteration
    int host_cap = 0;
};

struct cglb_ctx {
    cglb_comm_state* comm = nullptr;
    cglb_devpool mem;      // owns every device buffer below but the n2m_* ones; released by cglb_ctx_destroy
    cglb_devpool n2m_mem;  // owns the n2m_* buffers; released by n2m_free (a changed "n2m_tile" drops the tiles) and cglb_ctx_destroy
    cglb_devpool gpr_mem;  // owns the gpr_* buffers (Xn, the N x N factor and inverse); released by gpr_free (a changed "gpr_block") and cglb_ctx_destroy
    // geometry
    int64_t N = 0, r0 = 0, r1 = 0, nloc = 0, lda = 0;  // lda: leading dimension of At/Guf (nloc rounded up to 8)
    int D = 0, Dp = 0, M = 0, dtype = CGLB_F64, kind = CGLB_RBF, device = 0;
    int Dh = 0;        // 32 < D <= 96, fp64: padded width (48, 64, 80, 96) of the hot operand set Xh kept for the register-resident mat-vec
    int wide_grad_sym = 1;  // option "wide_grad_sym": 0 evaluates every tile of the tiled K_ff gradient pass (A/B)
    int wide_reg = 1;  // option "wide_reg": 0 sends that mat-vec through the Gram tiles of kernels_wide.hip as well (A/B, fallback)
    int input_grad_mid = 0;  // option "input_grad_mid": 1 opens every input-gradient product of a mid-width context (kernels_input_grad_mid.hip, kernels_predict_grad_mid.hip); 0: refused
    int grad_multi_mid = 1;  // option "grad_multi_mid": 0 sends the multi-pair gradient pass of a mid-width context through single passes (A/B, fallback)
    size_t esz = 8;
    hipStream_t stream = nullptr;
    rocblas_handle blas = nullptr;
    // state flags
    bool have_data = false, have_hypers = false, have_local = false, have_terms = false;
    bool obj_valid = false;  // w_r / w_z hold r = e - K v and w = P r of the last cglb_objective_and_grad
    // raw data (element type T)
    void *X = nullptr, *y = nullptr, *Z = nullptr;
    double xmean[CGLB_MAX_D] = {0};  // column means of X (centre for the Gram form)
    double xrange[CGLB_MAX_D] = {0}; // max |x - mean| per column (bounds the exponent range of the hot loops)
    double xradius2 = 0.0;           // max_i |x_i - mean|^2 (ball bound of the row norms)
    // hypers (host)
    double ls[CGLB_MAX_D] = {0};
    double var = 1, noise = 1, mean = 0, jitter = 1e-6;
    // scaled operands of the streaming kernels (T): xs = (x-c)/l*kscale padded to Dp, xa = per-row norm term
    void *Xs = nullptr, *xa = nullptr, *Zs = nullptr, *za = nullptr;
    void *Zh = nullptr, *zah = nullptr;  // hot-scaled inducing points (implicit preconditioner)
    void* Zhm = nullptr;                 // [M][Dh] inducing points in hot units at width Dh: the row-weighted gradient product of a mid-width context (first use)
    bool Zhm_valid = false;              // Zhm belongs to the current data and hyper-parameters (predict_grad_mid_inducing)
    void *Linv = nullptr, *LinvT = nullptr;  // L^-1 (column-major lower) and its transpose (implicit preconditioner)
    void* w_q = nullptr;                 // [M] scratch
    void* ppart = nullptr;               // partial slab of launch_pairs_rect
    size_t ppart_cap = 0;
    void* chol_blk = nullptr;            // dense copy of the current diagonal block + reciprocal diagonal (kernels_chol.hip)
    int chol_mode = 1;                   // 1: blocked LDS Cholesky (kernels_chol.hip), 0: rocSOLVER potrf
    int precond_mode = 0;                // 0: stored panel A (reference form), 1: implicit K_uf products
    void *Xhsq = nullptr;  // Xh squared element-wise: second-moment operand of the Gram-form gradient pass (kernels_grad.hip)
    const void* pwh_src = nullptr;       // vector whose weighted copy pwh currently holds (set by update_p, consumed once by the next symmetric mat-vec)
    // wide inputs (D > 32, kernels_wide.hip): element-wise squares of the scaled operands, tile / panel / moment scratch, device copies of
    // the per-dimension centre and scale
    void *Xsq = nullptr, *Zsq = nullptr;
    void *wtile = nullptr, *wpart = nullptr, *wS1 = nullptr, *wR = nullptr, *wC = nullptr, *wones = nullptr, *wpanel = nullptr;
    size_t wtile_cap = 0, wpart_cap = 0, wS1_cap = 0, wpanel_cap = 0;
    void* wlong = nullptr;   // slabs of a long-k GEMM cut into chunks (kernels_wide.hip: gemm_long_k)
    size_t wlong_cap = 0;
    double *wcenter = nullptr, *wscale = nullptr, *wsmall = nullptr;
    void* uwh = nullptr;                 // u o wh: second weighted column operand of the Gram-form gradient pass (allocated on first use)
    void *wh = nullptr, *pwh = nullptr;  // RBF column weights 2^(xah_j/T) and the weighted operand p_j * wh_j of the symmetric mat-vec (length N)
    void *Xh = nullptr, *xah = nullptr;  // hot operand set of the pair kernels: exponents in 1/T octave, T = 2^CGLB_TAB_BITS (devmath.h exp2_tab)
    double* exp_tab = nullptr;           // device table 2^(k/T) or 2^((k+1/2)/T) (CGLB_EXP_FLOOR), k < T = 2^CGLB_TAB_BITS, exponent pre-compensated (devmath.h)
    // common terms (column-major M x M unless noted)
    void* At = nullptr;      // A as [M][nloc] row-major == (nloc x M) column-major, ld = nloc
    void* Lc = nullptr;      // chol(Kuu + jitter I), lower, column-major
    void* LBc = nullptr;     // chol(B), lower, column-major
    void* LBinv = nullptr;   // LB^-1 lower, column-major, strict upper zeroed
    void* LBinvT = nullptr;  // its transpose (upper as col-major == rows of LB^-1 contiguous)
    void* AAt = nullptr;     // A A^T (full symmetric)
    void* Mtmp = nullptr;    // M x M scratch
    void* Mtmp2 = nullptr;   // M x M scratch
    void* Mtmp3 = nullptr;   // M x M scratch of the gradient algebra (allocated on first use)
    void* Mtmp4 = nullptr;   // M x M residual scratch of its refinement steps (allocated on first use)
    bool have_Linv = false;  // Linv holds L^-1 of the current K_uu factor
    bool Linv_unchecked = false;  // the trtri status of Linv (info_dev[2]) has not been read back yet
    int grad_trsm = 2;       // gradient algebra against L: 0 products with the explicit L^-1 (fastest), 1 rocBLAS trsm / trsv (backward stable),
                             // 2 (default) the products + one step of iterative refinement against L (accuracy of 1 at ~2/3 of its time)
    double L_diag_ratio = 1.0;  // max diag(L) / min diag(L) of the current K_uu factor (cglb_get_stat "L_diag_ratio")
    void* Guf = nullptr;     // adjoint of Kuf, same layout as At (allocated on first gradient)
    void *fragA = nullptr, *fragB = nullptr;  // MFMA-ordered augmented operands (kernels_kff_mfma.hip)
    size_t fragA_cap = 0, fragB_cap = 0;
    bool frag_valid = false;  // fragA / fragB (operands of the experimental matrix-pipe variant) match the current hypers
    pair_list sym_list;              // work list (row block, column chunk) of the symmetric mat-vec (kernels_kff_sym.hip: ensure_sym_items)
    int64_t sym_chunk_opt = 0;
    double sym_pairs = 0.0;          // kernel pairs one launch of the symmetric pair kernel evaluates (current item list)
    // in-situ timing of the dominant kernel (cglb_set_option "k1_profile", cglb_get_stat): HIP event pairs around every launch of the
    // symmetric pair kernel on the context stream, resolved lazily
    bool k1_profile = false;
    std::vector<hipEvent_t> k1_events;
    size_t k1_events_used = 0;
    double k1_ms_total = 0.0;
    long long k1_launches = 0;
    // phase timing of cglb_objective_and_grad / cglb_dist_objective_and_grad / cglb_objective_and_grad_multi ("eval_profile"): 5 events per completed evaluation (start | common terms | PCG | final mat-vec +
    // preconditioner + scalars | gradient), resolved lazily by cglb_get_stat "eval_*_ms"
    bool eval_profile = false;
    std::vector<hipEvent_t> eval_events;
    size_t eval_events_used = 0;
    double eval_ms[4] = {0, 0, 0, 0};
    long long eval_count = 0;
    int grad_gram = 1;    // 1: Gram-form symmetric gradient pass (moments), 0: direct differences
    int aat_block = 512;  // block width of the lower-triangle-only split-K A A^T (0 or not dividing M: the full square)
    int sym_order = 1;  // item order of the symmetric kernels: 0 row-block major, 1 XCD-aware (pair_worklist.h)
    int par_world = 1, par_rank = 0;  // cyclic distribution of the symmetric K_ff work over ranks (cglb_set_parallel)
    void* slabs = nullptr;   // split-K partial A A^T slabs [nslab][M][M]
    size_t slab_cap = 0;
    rocblas_int* info_dev = nullptr;
    double trace_AAt = 0, sum_log_diag_LB = 0;
    // work vectors (T): all length nloc unless noted
    void *w_r = nullptr, *w_z = nullptr, *w_p = nullptr, *w_Ap = nullptr, *w_Kv = nullptr, *w_e = nullptr;
    void* w_pfull = nullptr;       // [N] gathered p for single-shard solve
    void *w_u = nullptr, *w_t = nullptr, *w_t2 = nullptr;  // [M]
    void* kpart = nullptr;         // K_ff mat-vec partial row sums [jsplit][nloc]
    size_t kpart_cap = 0;
    void* tpart = nullptr;         // A^T t partial sums [msplit][nloc]
    double* dotpart = nullptr;     // block partials for dots (double always) [DOTPART_CAP]
    double* scal = nullptr;        // device scalars (double) [64]
    double* host_scal = nullptr;   // pinned host mirror for the asynchronous read of the stop-test scalar
    hipEvent_t scal_event = nullptr;
    int final_matvec = 0;          // 1: K v recomputed after the solve (models.py:280); 0 (default): K v = e - r from the residual the PCG recurrence carries
    int pcg_lookahead = 1;         // 1: enqueue the next mat-vec before waiting for the stop-test scalar (cglb_api.hip: pcg_solve)
    double* gpart = nullptr;       // gradient partial buffers
    size_t gpart_cap = 0;
    double* gradbuf = nullptr;     // device packed gradient [GRAD_LEN]
    // tunables
    int precision = 1;  // CGLB_PREC_FAST (devmath.h): kernel values to <= 1e-13; 0 = CGLB_PREC_EXACT (~3e-16); 2 = CGLB_PREC_LOW (~1e-10, opt-in)
    int kff_variant = 2, kff_jsplit = 0, kff_rows = 4;  // 0 plain, 1 matrix-pipe Gram (fp64), 2 symmetric (default)
    int kuf_msplit = 0;             // > 0: forced chunk count over the inducing points of the transposed panel pass (row_slab.h: row_slab_panel_split)
    bool exp_clamp = false;         // scaled operands so large that 2^x needs the range clamp (set by set_hypers)
    double m32_bias = 0.0;          // Matern-3/2 and -5/2: positivity bias of the squared distance in hot units^2 (devmath.h CGLB_M32_BIAS_*; set by set_hypers)
    bool kff_skip_combine = false;  // timing only: launch the pair kernel without the slab combine
    // bound variants (options "logdet_bound", "quad_term"; include/cglb_hip.h).  Both 0: the CGLB bound of models.py:215-286.
    int logdet_bound = 0;  // 0 Jensen (cglb), 1 NM^2 (cglbnm2, sgpr), 2 N^2M (cglbn2m, sgprn2m; fp64, stored panel, one shard)
    int quad_term = 0;     // 0 CG (v, PCG), 1 exact Woodbury quadratic term at v = 0 (sgpr, sgprn2m): no N^2 work
    void* w_zero = nullptr;  // [N] zeros: the v of the exact quadratic term (allocated on first use)
    // multi-output targets (cglb_set_targets) and the shared-kernel product K_ff V (kernels_kff_multi.hip); all allocated on first use
    int p = 1;               // number of target columns; column 0 is always mirrored in y, so every single-column entry point sees it
    void* Ym = nullptr;      // [p][N] targets, column b contiguous (p > 1 only)
    size_t Ym_cap = 0;
    void* mw = nullptr;      // [6][s][N] work vectors of the batched PCG / evaluation: r, z, p, Ap, Kv, b
    size_t mw_cap = 0;
    double* mscal = nullptr; // [3][s] device scalars per column: rz, new rz, p.Ap (what scal + S_RZ / S_NRZ / S_PAP are to one column)
    size_t mscal_cap = 0;
    double* mhost = nullptr; // [s] pinned host mirror of one row of mscal (what host_scal is to one column: pcg_ops::host)
    int mhost_cap = 0;
    double* mgrad = nullptr; // [GRAD_LEN] device sum of the per-column gradients
    pair_list mm_list;          // work list (group of four row blocks, column span) of the multi-column pair kernel
    void* mm_part = nullptr;    // its partial-sum slabs
    size_t mm_part_cap = 0;
    void* mm_vi = nullptr;      // [N][8] interleaved (and pre-weighted) column-side operand
    size_t mm_vi_cap = 0;
    // N^2M pass (kernels_n2m.hip), fp64, allocated on first use
    double *n2m_Xn = nullptr, *n2m_Wt = nullptr, *n2m_Ct = nullptr, *n2m_K = nullptr, *n2m_G = nullptr;  // X/l; W = K_ff A^T and C^T (layout of At); tiles
    double *n2m_H = nullptr, *n2m_E = nullptr, *n2m_T = nullptr;  // H = A W, E = B^-1 (H + s AA^T) B^-1, M x M scratch
    double *n2m_ls = nullptr, *n2m_part = nullptr, *n2m_gacc = nullptr, *n2m_scal = nullptr;  // lengthscales, block partials, sum_ij G_ij dK_ij/dl_d, scalars
    int64_t n2m_bt = 0;    // tile edge of the K / G panels
    int64_t n2m_tile = 0;  // option "n2m_tile": requested tile edge (0: min(4096, N rounded up to 64))
    double n2m_tau = 0, n2m_BH = 0, n2m_trBinv = 0;  // tau = tr K~ - tr(C K~ C^T), <B^-1, H>, tr B^-1 (of the last setup)
    // exact GPR (kernels_gpr.hip; cglb_gpr_*), fp64, one shard, one target column; everything allocated on first use
    std::vector<double> gpr_ls;                         // lengthscales of cglb_gpr_set_hypers (host); its variance, noise and mean follow
    double gpr_var = 1, gpr_noise = 1, gpr_mean = 0;
    bool gpr_have_hypers = false, gpr_factored = false; // gpr_L / gpr_alpha hold chol(K) and K^-1 e at the current data and hypers
    int64_t gpr_block = 2048;                           // option "gpr_block": outer block edge of the fill, the factorisation and the gradient pass
    double *gpr_Xn = nullptr, *gpr_lsd = nullptr;       // X / l [N][D]; device lengthscales
    double *gpr_L = nullptr, *gpr_Kinv = nullptr;       // N x N column-major, lower triangle: chol(K); K^-1 (gradient evaluations only)
    double *gpr_blk = nullptr;                          // dense copy of the current diagonal block (edge gpr_block)
    double *gpr_e = nullptr, *gpr_alpha = nullptr, *gpr_ones = nullptr;  // [N]: y - c, K^-1 e, ones
    double *gpr_part = nullptr, *gpr_acc = nullptr, *gpr_scal = nullptr; // block partials [(block / 64)^2][D + 2], their sums [D + 2], scalars [8]
    int* gpr_info = nullptr;                            // pivot status of the current diagonal block; potri status
    double *gpr_Ks = nullptr, *gpr_xnew = nullptr;      // prediction: K_f* (N x batch, column-major) and the scaled new points
    size_t gpr_Ks_cap = 0, gpr_xnew_cap = 0;
    double *gpr_Xh = nullptr, *gpr_xh = nullptr, *gpr_Ct = nullptr;  // input gradients: X and the batch in hot units at gpr_ls, C = K^-1 K_f* as [N][ld]
    size_t gpr_xh_cap = 0, gpr_Ct_cap = 0;
    double* gpr_Wt = nullptr;                           // training-input gradient: a block column of alpha alpha^T - K^-1 as [N][ld]
    size_t gpr_Wt_cap = 0;
    bool gpr_hot_valid = false;                         // gpr_Xh holds X at the current data and lengthscales
    double* gpr_cs = nullptr;                           // mid widths: device [centre (D) | ks / gpr_ls (D)], scales of gpr_Xh / gpr_xh and of their gradient constants
    size_t gpr_bytes = 0;                               // device bytes the pool holds (cglb_get_stat "gpr_bytes")
    hipEvent_t gpr_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // start | fill | factor | solves | inverse | gradient of the last evaluation
    int gpr_ev_last = 0;                                // index of the last event that evaluation recorded (2: no solve reached, 3: value only, 5: with gradient)
    // multi-pair gradient pass (kernels_grad_multi.hip) and the iterative exact-GP class (cglb_itergp_*): fp64, one shard, one rank, one target
    // column; everything allocated on first use
    void* gm_uv = nullptr;                              // [N][16] interleaved column-side operands of the multi-pair gradient pass
    size_t gm_uv_cap = 0;
    pcg_log it_log;                                     // coefficient logs of the last solve of cglb_itergp_objective_and_grad
    int it_steps = 0, it_t = 0;                         // ... its step count and number of probes
    double *it_V = nullptr, *it_eps = nullptr, *it_scal = nullptr;  // [1 + t][N] solutions; [t][k + N] probes; [D + 1 + (1 + t) + 2] device scalars
    size_t it_V_cap = 0, it_eps_cap = 0, it_scal_cap = 0;
    double* it_alpha = nullptr;                         // [N] alpha = K^-1 e of the last evaluation (warm start of the predictive solve)
    bool it_valid = false;                              // it_alpha and the common terms belong to the current data, targets and hyper-parameters
    hipEvent_t it_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start | pivots and common terms | solve | gradient of the last evaluation
    int it_ev_last = 0;                                 // index of the last event that evaluation recorded (0: none, 2: value only, 3: with gradient)
    // Lanczos variance cache of the class (cglb_itergp_var_cache) and the multi-column cross product that applies it (kernels_cross_multi.hip)
    double* it_cache = nullptr;                         // [N][it_cache_ld]: Q during the build, then R = Q L^-T with K^-1 ~ R R^T; zero beyond column J
    size_t it_cache_cap = 0;
    int it_cache_rank = 0, it_cache_ld = 0;             // J columns in use (0: no valid cache); row stride = the requested rank rounded up to 8
    int it_cache_request = 0;                           // the rank the valid cache was asked for
    double *it_lq = nullptr, *it_lw = nullptr, *it_lc = nullptr, *it_lpart = nullptr;  // [N] q_j, [N] w, [2 ld + 2] coefficients, block partials of Q^T w
    size_t it_lq_cap = 0, it_lw_cap = 0, it_lc_cap = 0, it_lpart_cap = 0;
    double* it_blk = nullptr;                           // [rows][r_pad] summed block K_*f R of the cached predictive
    size_t it_blk_cap = 0;
    hipEvent_t it_cev[4] = {nullptr, nullptr, nullptr, nullptr};  // cache build start | end, cached variance start | end
    bool it_cev_set[2] = {false, false};
    void* cm_part = nullptr;                            // partial-sum slabs [jsplit][rows][8] of the multi-column cross product
    size_t cm_part_cap = 0;
    void* cm_vi = nullptr;                              // [N][S rounded up to 8] interleaved column operand of cglb_cross_matmat
    size_t cm_vi_cap = 0;
    // random-feature product (kernels_feature_multi.hip) and the pathwise posterior samples built on it (cglb_itergp_sample)
    double* ft_rec = nullptr;                           // [groups][F][FEATURE_REC (row_slab.h)] operand records {b_j | omega_j | W[8 g .., j]} in turns
    double* ft_in = nullptr;                            // [F][D] omega and [F] phases as the caller gave them (device copy)
    double* ft_par = nullptr;                           // [D] 1 / (2 pi l_k), [D] centre c_k
    double* ft_part = nullptr;                          // partial-sum slabs [jsplit][rows][8]
    size_t ft_rec_cap = 0, ft_in_cap = 0, ft_par_cap = 0, ft_part_cap = 0;
    std::vector<double> ft_host;                        // host source of ft_par
    double* ft_G = nullptr;                             // [rows][S] feature product of a sampling call (training rows, then the new points)
    double* ft_KU = nullptr;                            // [n_new][S] K_*f U of a sampling call
    size_t ft_G_cap = 0, ft_KU_cap = 0;
    double* ig_part = nullptr;                          // partial-sum slabs [jsplit][rows][G][Dp + 1] of the input-gradient products
    double* ig_gk = nullptr;                            // [rows][S][D] gradient block of the cross product (predictive: a row block over the cache columns)
    double* ig_gf = nullptr;                            // [rows][S][D] gradient block of the feature product of cglb_itergp_paths_eval
    size_t ig_part_cap = 0, ig_gk_cap = 0, ig_gf_cap = 0;
    hipEvent_t ft_ev[2] = {nullptr, nullptr};           // start | end of the last feature product ("feature_ms")
    bool ft_ev_set = false;
    hipEvent_t pg_ev[2] = {nullptr, nullptr};           // start | end of the last row-weighted gradient product ("predict_grad_kernel_ms")
    bool pg_ev_set = false;
    std::string err;
};

#define DOTPART_CAP 65536
// A mis-speculated mat-vec costs 2.9 ms at the headline shape, the stall it avoids 38 us: speculation must be right ~99 % of the time.
// Measured on 33 warm-started training evaluations (tools/lookahead_waste.py, profiles/r03_lookahead_waste.log): factor 4 wasted 16
// mat-vecs (median evaluation 32.1 ms), 16 one, 64 none (29.05 ms).
#ifndef CGLB_LOOKAHEAD_FACTOR
#define CGLB_LOOKAHEAD_FACTOR 32.0
#endif

#define HIP_CHECK(ctx, expr)                                                                         \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                          \
            return CGLB_ERR_HIP;                                                                     \
        }                                                                                            \
    } while (0)

#define BLAS_CHECK(ctx, expr)                                                                        \
    do {                                                                                             \
        rocblas_status _s = (expr);                                                                  \
        if (_s != rocblas_status_success) {                                                          \
            (ctx)->err = std::string(#expr) + ": rocblas status " + std::to_string((int)_s);         \
            return CGLB_ERR_BLAS;                                                                    \
        }                                                                                            \
    } while (0)

#define CGLB_TRY(expr)                 \
    do {                               \
        int _rc = (expr);              \
        if (_rc != CGLB_OK) return _rc; \
    } while (0)

static inline int cglb_fail(cglb_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// per-call device temporaries: freed on every exit path of the function that owns the holder
struct DevTemps {
    std::vector<void*> ptrs;
    ~DevTemps() { for (void* p : ptrs) if (p) (void)hipFree(p); }
    int alloc(cglb_ctx* c, void** out, size_t bytes) {
        *out = nullptr;
        hipError_t e = hipMalloc(out, bytes ? bytes : 16);
        if (e != hipSuccess) return cglb_fail(c, CGLB_ERR_HIP, std::string("hipMalloc of a temporary: ") + hipGetErrorString(e));
        ptrs.push_back(*out);
        return CGLB_OK;
    }
};

// The new points of one call, staged on the device for the kernels it enqueues on c->stream: xr [n][D] the rows as given, xs [n][Dp] and xa [n]
// their scaled form (absent where a call reads the raw rows alone).  The destructor waits for the stream and only then frees: no buffer, of these
// or of `tmp`, is released while a kernel enqueued by the call may read it, on any exit path, and the caller's host arrays are its own again.
// (Methods: cglb_api.hip.)
struct StagedPoints {
    cglb_ctx* c;
    int64_t n = 0;
    size_t esz = 0;
    void *xr = nullptr, *xs = nullptr, *xa = nullptr;
    void* xh = nullptr;  // mid-width contexts, after stage_hot_mid: the points in hot units at width Dh (xs is the plain scaled set there)
    DevTemps tmp;  // the further temporaries of the call
    explicit StagedPoints(cglb_ctx* cc) : c(cc) {}
    StagedPoints(const StagedPoints&) = delete;
    ~StagedPoints() { (void)hipStreamSynchronize(c->stream); }  // `tmp` frees after this body
    int alloc(int64_t n_points, size_t elem, bool scaled = true);  // n points of element size elem; not scaled: xr alone
    int stage(const void* xnew, bool hot = true);                  // xr <- xnew (host or device), then (xs, xa) in hot or plain units where allocated
    int scale(bool hot);                                           // (xs, xa) from xr once more, in the units asked for
    int stage_hot_mid();                                           // xh [n][Dh] from the staged xr (wide_prep_hot_rows), allocated on first use
};

static inline int pad_dim(int d) {
    const int sizes[] = {1, 2, 3, 4, 6, 8, 10, 12, 16, 20, 24, 28, 32};  // 10, 20 and 28: the reference's own data sets have D = 9, 17, 18, 26, 27
    for (int s : sizes)
        if (d <= s) return s;
    return d;  // wide inputs are not padded: their Gram products go through rocBLAS (kernels_wide.hip)
}
static inline bool is_wide(const cglb_ctx* c);

static inline bool is_wide(const cglb_ctx* c) { return c->Dp > CGLB_MAX_D_NARROW; }
// padded width of the hot operand set of a mid-width fp64 context (0: none)
static inline int mid_dim(int d, int dtype) {
    if (dtype != CGLB_F64 || d <= CGLB_MAX_D_NARROW || d > CGLB_MAX_D_MID) return 0;
    return d <= 48 ? 48 : d <= 64 ? 64 : d <= 80 ? 80 : 96;  // (a 128-wide row operand alone would fill the 256 VGPRs VALU instructions can address)
}
static inline bool mid_reg(const cglb_ctx* c) { return c->Dh > 0 && c->wide_reg != 0; }
static inline bool input_grad_mid_on(const cglb_ctx* c) { return c->input_grad_mid != 0 && mid_reg(c); }  // every input-gradient product runs at this mid width

// kernels_wide.hip: D > 32.  The Gram part of the pair value is a contraction with k = D and goes through rocBLAS in tiles; same
// contracts as the launchers below they stand in for.
int wide_prep_scaled(cglb_ctx* c, const void* Xraw, int64_t n, void* Xs_out, void* xa_out, void* Xsq_out);
int wide_after_hypers(cglb_ctx* c);
int wide_prep_hot(cglb_ctx* c);   // Xh (N x Dh, zero padded), xah in hot units for the register-resident mat-vec of a mid-width context
int wide_prep_hot_rows(cglb_ctx* c, const void* Xraw, int64_t n, void* Xh_out, void* xah_out);  // the same for any n raw rows: Xh_out [n][Dh], xah_out [n]
int wide_kuf(cglb_ctx* c);
int wide_kuu(cglb_ctx* c);
int wide_kpanel(cglb_ctx* c, const void* Zs, int M, const void* XsNew, int64_t n_new, int64_t ld, void* out);  // out[m * ld + n] = var K(z_m, xnew_n), any two scaled sets
// out[i * ldo + s] = var * sum_j kappa(row_i, x_j) Vi[j * ldv + s], s < S (fp64): what launch_cross_multi is to narrow inputs, through the Gram tiles
int wide_cross_multi(cglb_ctx* c, const void* XsRow, const void* xaRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo);
int wide_matvec(cglb_ctx* c, const void* XsRow, const void* xaRow, int64_t row0_global, int64_t nrows, const void* p_full, void* out, bool diag_noise,
                double* pdot_slot, int tile_stride, int tile_offset);
int wide_grad_kff(cglb_ctx* c, const void* v_full, const void* u_rows, int64_t row0, int64_t nrows, int tile_stride, int tile_offset, double* out_dl);
int wide_grad_panel(cglb_ctx* c, const void* G, int64_t ldg, const void* cvec, const void* wvec, const void* XsCol, const void* xaCol, const void* XsqCol,
                    int64_t ncols, double zfactor, double* out);
// N^2M log-det bound (kernels_n2m.hip): the terms of the bound after setup, the kernel-hyper-parameter part of its gradient in phase 3
int n2m_setup(cglb_ctx* c);  // W = K_ff A^T, H = A W, tau, <B^-1, H>, tr B^-1
int n2m_grad_terms(cglb_ctx* c, const double* Binv);  // E (n2m_E, trace in n2m_scal[2]) and n2m_gacc[d] = sum_ij G_ij dK_ij/dl_d, G = C^T C
void n2m_free(cglb_ctx* c);
// exact GPR (kernels_gpr.hip): releases gpr_mem (the next evaluation allocates and factors again); the phase times of the last evaluation
void gpr_free(cglb_ctx* c);
int gpr_stat(cglb_ctx* c, const char* name, double* value);  // CGLB_OK if `name` is one of the gpr_* statistics, -1 if it is not

// ---- launchers implemented in the kernel translation units (all enqueue on ctx->stream) ----------
// kernels_prep.hip
int launch_prep_scaled(cglb_ctx* c, const void* Xraw, int64_t n, void* Xs_out, void* xa_out, bool hot = false);
double cglb_hot_scale(const cglb_ctx* c);  // xh = hot_scale * xs
double cglb_kscale(const cglb_ctx* c);     // xs = (x - centre) / l * kscale: the kind's operand scale
int launch_select_inducing(cglb_ctx* c, double variance, double jitter, long long* chosen_dev, void* Z_out, double* trace_dev);  // kernels_select.hip
int launch_kuf(cglb_ctx* c);  // At <- Kuf[:, rows] (unscaled by sigma)
int launch_kuu(cglb_ctx* c);  // Lc <- Kuu + jitter I (full symmetric)
// kernels_kff.hip
int launch_kff_matvec(cglb_ctx* c, const void* p_full, void* out_local, double* pdot_slot);
int launch_cholesky_lower(cglb_ctx* c, void* A, int* info_slot);
int launch_cholesky_lower_n(cglb_ctx* c, void* A, int n, int* info_slot);  // dense n x n, leading dimension n
int launch_frag_prep(cglb_ctx* c);
int launch_kff_sym(cglb_ctx* c, const void* p_full, void* out_local, double* pdot_slot);
int launch_hot_weights(cglb_ctx* c);  // wh = 2^(xah/T) after set_hypers (RBF)
int launch_kff_sym_mid(cglb_ctx* c, const void* p_full, void* out, double* pdot_slot, bool cyclic);  // 32 < D <= 96, fp64 (kernels_kff_sym.hip)
int grad_fold_operands(cglb_ctx* c, const void* v_full, const void* u, int64_t off, int64_t n_u, bool* fold);  // column-side copies u o w, v o w (folded column norm)
int launch_grad_kff_mid(cglb_ctx* c, const void* v_full, const void* u_full, int world, int rank, double* out_dl);  // kernels_grad_mid.hip
int launch_hot_squares(cglb_ctx* c);  // Xhsq = Xh .* Xh after set_hypers
int k1_profile_collect(cglb_ctx* c);  // resolves the pending event pairs into k1_ms_total / k1_launches
int launch_kff_sym_cyclic(cglb_ctx* c, const void* p_full, void* out_full_partial);  // this rank's share of the global upper triangle
int launch_grad_kff_cyclic(cglb_ctx* c, const void* v_full, const void* u_full, double* out_dl);
// kernels_kff_multi.hip: Out[b] = (K_ff + noise I) V[b], b < s; V [s][N], Out [s][nloc].  One evaluation of every kernel value for up to 8
// columns where kff_multi_native(c), s single mat-vecs elsewhere.
bool kff_multi_native(const cglb_ctx* c);
int launch_kff_matmat(cglb_ctx* c, const void* V, int s, void* Out);
// what the two pair kernels of the product share (kernels_kff_multi.hip): the span / LDS-chunk geometry with its work list and slabs, the
// interleaved column operand c->mm_vi (pre-weighted where `fold`), and the combine of the slabs into Out
struct multi_geometry {
    int64_t span = 0, chunk = 0, prow_ld = 0;
    int Q = 0, nwg = 0, nrb = 0, nspan = 0;
    double *Prow = nullptr, *Pcol = nullptr;
};
int multi_prepare(cglb_ctx* c, const double* V, int s, int sp, int rbrows, bool fold, multi_geometry* geo);
int multi_combine(cglb_ctx* c, const multi_geometry& geo, int rbrows, int sp, const double* V, int s, double* Out);
// kernels_kff_multi_mid.hip: one group of 2 .. multi_mid_group(Dh) columns of a context with mid_reg(c) (32 < D <= 96, fp64), both exponent ranges
int launch_kff_multi_mid(cglb_ctx* c, const double* V, int sg, double* Out);
int launch_kff_plain_range(cglb_ctx* c, const void* p_full, int64_t col0, int64_t col1, void* part, int64_t* nslots);
int launch_kff_mfma_pairs(cglb_ctx* c, const double* p_full, int64_t* jsplit_out);
int launch_pairs_rect(cglb_ctx* c, const void* XsRow, const void* xaRow, int64_t nrows, const void* XsCol, const void* xaCol, const void* pcol,
                      int64_t col0, int64_t col1, void* out);
int launch_tri_rowdot(cglb_ctx* c, const void* Wrows, const void* x, int lower, void* out);
int launch_scale(cglb_ctx* c, void* x, double a, int64_t n);
int launch_precond_z_from(cglb_ctx* c, const void* r_local, const void* Ks_local, void* z_local, double* rz_slot);
int launch_cross_matvec(cglb_ctx* c, const void* Xs_new, const void* xa_new, int64_t n_new, const void* v_full, void* out);
// kernels_grad_multi.hip: out[d] = sum_b u_b^T (dK_ff/dl_d) v_b, d < D, out[D] = sum_b u_b^T kappa v_b; U, V [S][N]; out dev double[D + 1], overwritten.
// One evaluation of every kernel value for up to 8 pairs where grad_multi_native(c), S single passes elsewhere.
bool grad_multi_native(const cglb_ctx* c);
int launch_grad_kff_multi(cglb_ctx* c, const void* U, const void* V, int S, double* out);
// kernels_grad_multi_mid.hip: out (+)= the same sums of one group of 2 .. grad_multi_mid_group(Dh) pairs of a context with mid_reg(c), both exponent ranges
int launch_grad_kff_multi_mid(cglb_ctx* c, const double* U, const double* V, int sg, double* out, int accumulate);
// kernels_train_input_grad.hip: gx[i * D + k] = sum_j w_ij d kappa(x_i, x_j) / d x_ik, w_ij = sum_b (u_bi v_bj + v_bi u_bj), with respect to the raw training
// inputs; U, V [S][N] as above; gx dev [N][D], overwritten.  Where !train_input_grad_native(c) (fp32, more than 32 dimensions, N ranks) it is refused.
// Bitwise repeatable.
bool train_input_grad_native(const cglb_ctx* c);
int launch_grad_x_kff_multi(cglb_ctx* c, const void* U, const void* V, int S, double* gx);
int train_input_grad_rows_per_block(const cglb_ctx* c);  // rows per workgroup at the context's width
int train_input_grad_width(const cglb_ctx* c);           // vector pairs per group at the context's width (8 or 4)
// ... its single-pair instance (G = 1): gx (+)= the same sum for ONE pair u, v (dev [N]), w_ij = u_i v_j + v_i u_j; accumulate: added to gx
int launch_grad_x_kff_pair(cglb_ctx* c, const void* u, const void* v, double* gx, int accumulate);
int train_input_grad_pair_rows_per_block(const cglb_ctx* c);
// kernels_bound_input_grad.hip, the transposed panel pass: gx[n * D + k] = sum_m (G[m * ldg + n] + cvec[m] wvec[n]) d k(z_m, x_n) / d x_nk with respect to
// the raw training inputs; G dev [M][ldg] (row m contiguous), cvec dev [M] and wvec dev [N] or both NULL; gx dev [N][D], overwritten.  The operand sets
// (Zs, Xs) and the evaluator of launch_grad_kuf.  fp64, one rank, Dp <= 32 (train_input_grad_native).  Bitwise repeatable.
int launch_grad_x_kuf(cglb_ctx* c, const void* G, int64_t ldg, const void* cvec, const void* wvec, double* gx);
int grad_x_kuf_rows_per_block(const cglb_ctx* c);
// The row-slab products (decomposition, chunk rules, layout constants and the shared value finish kernel: row_slab.h), one file each:
// kernels_cross_multi.hip: out[i * ldo + s] = var * sum_j kappa(row_i, x_j) Vi[j * ldv + s], s < S; Vi dev [N][ldv] row-major (ldv a multiple of 8, zero
// padded), rows hot-scaled; every kernel value evaluated once per group of 8 columns.  fp64, Dp <= 32.  Bitwise repeatable.
int launch_cross_multi(cglb_ctx* c, const void* XsRow, const void* xaRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo);
int launch_cross_multi_operand(cglb_ctx* c, const void* V, int S, int64_t* ldv_out);  // c->cm_vi <- V [S][N] interleaved
int launch_cross_multi_var(cglb_ctx* c, const double* blk, int64_t nrows, int sp, int64_t ld, double* f_var);  // f_var[i] = var - |blk[i][:sp]|^2
int cross_multi_rows_per_block(const cglb_ctx* c);  // new points per workgroup of the pair kernel at the context's width
int cross_multi_width();                            // columns per group (8): the leading dimensions are multiples of it
// kernels_feature_multi.hip: out[i * ldo + s] = sqrt(2 var / F) sum_j W[s][j] cos(sum_k omega[j][k] (x_ik - c_k) / l_k + b_j), s < S; X dev [nrows][D] raw
// rows; the operand records of (omega, phase, W) in c->ft_rec first (omega [F][D], phase [F]: host or device; W dev [S][F]).  fp64, any D.  Bitwise
// repeatable.
int launch_feature_operand(cglb_ctx* c, const void* omega, const void* phase, const void* W, int64_t F, int S);
int launch_feature_multi(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo);
int feature_rows_per_block(const cglb_ctx* c);      // rows per workgroup at the context's width
// kernels_input_grad.hip: value (out may be NULL) and input gradient gout[(i * S + s) * D + k] of the two products above, one evaluation of a pair per
// group of input_grad_width(c) columns; the operands of launch_cross_multi (hot-scaled rows, Vi [N][ldv]) / of launch_feature_multi (records first).
// fp64, Dp <= 32.  Bitwise repeatable.
int launch_cross_grad(cglb_ctx* c, const void* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo, double* gout);
int launch_feature_grad(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo, double* gout);
// kernels_input_grad_mid.hip: launch_cross_grad's and launch_feature_grad's contracts on a context with input_grad_mid_on(c) (fp64, 32 < D <= 96), where launch_cross_grad sends it:
// XhRow [nrows][Dh] from wide_prep_hot_rows.  Bitwise repeatable.
int launch_cross_grad_mid(cglb_ctx* c, const void* XhRow, int64_t nrows, const double* Vi, int64_t ldv, int S, double* out, int64_t ldo, double* gout);
int launch_feature_grad_mid(cglb_ctx* c, const double* X, int64_t nrows, int64_t F, int S, double* out, int64_t ldo, double* gout);  // launch_feature_grad's contract there
// the finish kernel of every mid-width input-gradient product: the slabs part[js][i][b < g][Dh + 1] in fixed order, then per slot b
//   out[b][i * ldo] = vscale * sum (out[b] NULL: no value), gout[b][i * ldg + k] = (gfac[b] scale[k]) * sum, k < D (gout[b] NULL: slot not stored);
// scale: the device copy of ks / l_k (NULL: 1, the feature product); add0: slot 0 adds to what gout[0] holds
#define INPUT_GRAD_MID_SLOTS 4
struct InputGradMidOut { double* out[INPUT_GRAD_MID_SLOTS]; double* gout[INPUT_GRAD_MID_SLOTS]; double gfac[INPUT_GRAD_MID_SLOTS]; int64_t ldo, ldg; int add0; };
int launch_input_grad_mid_finish(cglb_ctx* c, const double* part, int64_t jsplit, int64_t nrows, int g, double vscale, const double* scale, const InputGradMidOut& o);
int input_grad_mid_rows_per_block(const cglb_ctx* c);   // new points per workgroup (64)
int input_grad_mid_width(const cglb_ctx* c);            // columns per group at the context's hot width (4 or 2)
int launch_input_grad_var(cglb_ctx* c, const double* B, int64_t ldb, const double* G, int64_t nrows, int sp, double* g_var);  // g_var[i][k] = -2 sum_s B[i][s] G[i][s][k]
int launch_input_grad_paths(cglb_ctx* c, const double* Gf, const double* KU, const double* gf, const double* gk, int64_t n, int S, double* f, double* g);
// kernels_predict_grad.hip: row-weighted value and input gradient of a cross product between two explicit hot-unit point sets (lengthscales ls, host):
// out_u / gout_u with the shared weight u [npts], out_w / gout_w with new point i's own weights Wt[m * ldw + i]; gout_w times wscale, gout_u added to if add_u.
// Both sets have predict_grad_row_stride(c) doubles per point; a context with input_grad_mid_on(c) takes the gradient constants from scale_dev, the device
// copy of ks / l_k at ls, in place of ls
int launch_weighted_grad(cglb_ctx* c, const double* ls, double var, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u,
                         const double* Wt, int64_t ldw, double* out_u, double* gout_u, bool add_u, double* out_w, double* gout_w, double wscale,
                         const double* scale_dev = nullptr);
int launch_hot_points(cglb_ctx* c, const double* ls, const double* x, int64_t n, double* out);  // out [n][Dp] <- x [n][D] in hot units at ls
// kernels_predict_grad_mid.hip: the same product on a context with input_grad_mid_on(c) (fp64, 32 < D <= 96), where launch_weighted_grad sends each of its
// row blocks: both point sets [.][Dh]; scale: the device copy of ks / l_k both were staged with (c->wscale, or the second half of gpr_cs)
int launch_weighted_grad_mid(cglb_ctx* c, const double* scale, double var, const double* XhRow, int64_t nrows, const double* Ph, int64_t npts, const double* u,
                             const double* Wt, int64_t ldw, double* out_u, double* gout_u, bool add_u, double* out_w, double* gout_w, double wscale);
int launch_hot_points_mid(cglb_ctx* c, const double* cs, const double* x, int64_t n, double* out);  // out [n][Dh] <- x [n][D] in hot units, zero padded; cs dev [centre | ks / l]
int predict_grad_mid_inducing(cglb_ctx* c);               // c->Zhm [M][Dh] at the current hyper-parameters, built where it is not valid
int predict_grad_mid_rows_per_block(const cglb_ctx* c);   // new points per workgroup of the mid-width row-weighted kernel (64)
static inline int64_t predict_grad_row_stride(const cglb_ctx* c) { return input_grad_mid_on(c) ? c->Dh : c->Dp; }  // doubles per point of both sets of launch_weighted_grad
int launch_transpose(cglb_ctx* c, const double* src, int64_t lds, int64_t rows, int64_t cols, double* dst, int64_t ldd);  // dst[j * ldd + i] = src[i * lds + j]
int predict_grad_rows_per_block(const cglb_ctx* c);  // new points per workgroup of the row-weighted kernel at the context's width
int predict_grad_stat(cglb_ctx* c, const char* name, double* value);  // "predict_grad_kernel_ms"; -1: not this name
int input_grad_rows_per_block(const cglb_ctx* c);   // new points per workgroup at the context's width
int input_grad_width(const cglb_ctx* c);            // columns per group at the context's width (8, 4 or 2)
static inline int64_t input_grad_row_stride(const cglb_ctx* c) { return input_grad_mid_on(c) ? c->Dh : c->Dp; }  // doubles per new point of launch_cross_grad's XhRow
// kernels_vec.hip
// dot, update_v_r, update_p: s columns of length n ([s][n], one launch each; per-column device scalars [s]); s = 1 is the one-column form.
// A zero denominator gives a zero factor.
int launch_dot(cglb_ctx* c, const void* a, const void* b, int64_t n, double* out_slots, int s = 1);
int launch_update_v_r(cglb_ctx* c, void* v, void* r, const void* p, const void* Ap, const double* rz, const double* pAp, int update_r, int64_t n = -1,
                      int s = 1);
int launch_residual(cglb_ctx* c, void* r, const void* b, const void* Kv, int64_t n = -1);
int launch_axpy(cglb_ctx* c, void* y, double alpha, const void* x, int64_t n);
int launch_update_p(cglb_ctx* c, void* p, const void* z, const double* new_rz, const double* rz, int restart, int64_t n = -1, bool fuse = false,
                    int s = 1);  // fuse: s == 1 only
int launch_gemv_u(cglb_ctx* c, const void* r_local, void* u_out);               // u = A_loc r
int launch_tri_apply(cglb_ctx* c, const void* u, void* t_out);                  // t = LB^-T LB^-1 u
int launch_precond_z(cglb_ctx* c, const void* r_local, const void* t, void* z_local, double* rz_slot, void* rz_slot_T = nullptr);
int launch_update_p_seg(cglb_ctx* c, void* p, const void* zseg, int64_t n, int64_t per, int world, double* new_rz_out, const double* rz, int restart);
int launch_sub_scalar(cglb_ctx* c, void* out, const void* y_local, double mean, int64_t n);  // e = y - mean
int launch_tri_clean(cglb_ctx* c, void* Mc, int keep_lower);   // zero the other strict triangle
int launch_transpose(cglb_ctx* c, const void* src, void* dst); // M x M
int launch_add_identity_trace(cglb_ctx* c, void* Mc, double* trace_slot);        // trace then += I
int launch_sum_log_diag(cglb_ctx* c, const void* Mc, double* slot);
int launch_diag_minmax(cglb_ctx* c, const void* Mc, double* slot);  // slot[0..1] = min, max of the diagonal
int launch_symmetrize_lower(cglb_ctx* c, void* Mc);            // copy lower triangle to upper
int launch_obj_scalars(cglb_ctx* c, const void* v_local, const void* r, const void* Kv, const void* w, double* sc8);
// kernels_grad.hip
int launch_grad_kff(cglb_ctx* c, const void* v_full, const void* u_local, double* out_dl /* dev double[D], overwritten */);
int launch_grad_kuf(cglb_ctx* c, const void* cvec, const void* w_local, double* out /* packed gradient, accumulated */);
int launch_grad_kuu(cglb_ctx* c, const void* Guu, const void* cvec, const void* mhalf_c, double* out);
