/*
 * cglb_hip.h — C ABI of the MI355X-native CGLB quadratic-term solver (libcglb_hip.so).
 *
 * The reference (awav/CGLB, pure Python) has no FFI; these entry points are what a binding for its
 * hot path would call.  Each one cites the reference seam it stands in for (paths relative to the
 * reference repo root).  See INTEGRATION.md for the ctypes stub that plugs them into cglb.backend.
 *
 * Conventions
 *   - All array arguments are plain pointers; matrices are row-major; "dev" pointers are device
 *     (HBM) addresses (e.g. torch.Tensor.data_ptr()), "host" pointers are ordinary host memory,
 *     "any" may be either (copied with hipMemcpyDefault).  The caller owns every array it passes;
 *     the library keeps no pointer past the call (set_data/set_hypers copy).
 *   - Element type of vectors/matrices follows the ctx dtype (CGLB_F64 -> double, CGLB_F32 -> float);
 *     hyper-parameters and returned scalars are always double.
 *   - Every function returns 0 (CGLB_OK) or an error code; cglb_last_error() gives the text.
 *   - One ctx = one GPU = one row shard [row_begin,row_end) of the N training rows.  With a single
 *     shard (row_begin=0,row_end=N) the fused calls (cglb_pcg_solve, cglb_objective_and_grad) do the
 *     whole job.  With several shards (one process per GPU) either the library runs the loops itself and
 *     issues the collectives on its stream (cglb_comm_init_* + cglb_dist_*: RCCL, or callbacks), or the
 *     host drives the cglb_shard_* / cglb_vec_* phases and performs the collectives between them
 *     (cglb_amd/distributed.py: the same scheme step by step, testable over gloo with CPU local ops).
 *   - Calls on one ctx are serialised by the caller (the reference is single-threaded Python with a
 *     blocking sync per CG iteration, conjugate_gradient.py:80-81).  Work is enqueued on the HIP stream
 *     given at creation; functions that return host scalars synchronise that stream, the others do not.
 */
#ifndef CGLB_HIP_H
#define CGLB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cglb_ctx cglb_ctx;

enum { CGLB_OK = 0, CGLB_ERR_BAD_ARG = 1, CGLB_ERR_NOT_PD = 2, CGLB_ERR_HIP = 3, CGLB_ERR_BLAS = 4, CGLB_ERR_STATE = 5, CGLB_ERR_COMM = 6 };
enum { CGLB_RBF = 0, CGLB_MATERN32 = 1,        /* config.py:72-81 SquaredExponentialConfig / Matern32Config */
       CGLB_MATERN52 = 2 };                     /* beyond the reference's registry: k = f (1 + s + s^2/3) e^-s, s = sqrt5 r; gradient factor
                                                  * h = 5/3 f (1 + s) e^-s (dk/dl_d = h delta_d^2 / l_d).  Every entry point takes it except the
                                                  * experimental kff_variant 1, which returns CGLB_ERR_BAD_ARG.  cglb_ctx_create refuses any other value. */
enum { CGLB_F64 = 0, CGLB_F32 = 1 };           /* pytorch/interface.py:94-104 set_default_float */

/* Number of entries of the packed gradient: [dl_1..dl_D, d variance, d noise, d mean, dZ (M*D row-major)] */
#define CGLB_GRAD_LEN(D, M) ((D) + 3 + (M) * (D))

int cglb_version(void);

/* Model + data container.  Stands in for CGLB(data, likelihood, kernel) built by
 * pytorch/interface.py:315-323 (create_model for CGLBConfig) and models.py:54-68 (v_vec buffer).
 * stream: a hipStream_t (0 = default stream).  device: HIP device ordinal. */
int cglb_ctx_create(cglb_ctx** out, int64_t n_total, int64_t row_begin, int64_t row_end, int d, int m,
                    int dtype, int kernel_kind, int device, void* stream);
int cglb_ctx_destroy(cglb_ctx* ctx);
const char* cglb_last_error(const cglb_ctx* ctx); /* never NULL; ctx may be NULL (creation errors) */

/* Training inputs (model.train_inputs / train_targets, pytorch/interface.py:318-322).
 * X: any [n_total, d] (all rows: the column side of K_ff is replicated), y: any [n_total]. */
int cglb_set_data(cglb_ctx* ctx, const void* X, const void* y);

/* Constrained hyper-parameters: kernel lengthscales/outputscale, likelihood noise, ConstantMean,
 * inducing points, Cholesky jitter (pytorch/interface.py:150-178 model_parameters;
 * backend.py:77-79 jitter).  lengthscales: host double[d]; Z: any [m, d] of ctx dtype. */
int cglb_set_hypers(cglb_ctx* ctx, const double* lengthscales, double variance, double noise, double mean,
                    const void* Z, double jitter);

/* ---- common terms: LowerBoundCG.logdet_and_quad_common_terms, models.py:176-213 ---------------- */
/* single shard: L = chol(K_uu + jitter I), A = L^-1 K_uf / sigma, B = A A^T + I, LB = chol(B), tr(AA^T). */
int cglb_setup(cglb_ctx* ctx);
/* sharded: _local computes L, the column shard A[:, rows] and the partial A_loc A_loc^T into the buffer
 * returned by cglb_aat_buffer (dev [m*m]); the host all-reduces that buffer; _finish does the rest. */
int cglb_shard_setup_local(cglb_ctx* ctx);
void* cglb_aat_buffer(cglb_ctx* ctx);
int cglb_shard_setup_finish(cglb_ctx* ctx);
/* logdet_estimator (models.py:215-244) value for the current common terms. */
int cglb_logdet(cglb_ctx* ctx, double* logdet);

/* ---- operator seam: `A @ p` with A = kernel(x).add_diag(sigma^2), models.py:251-252,
 *      conjugate_gradient.py:57,66,72 -------------------------------------------------------------- */
/* out[row_begin:row_end] = K_ff[rows, :] p + noise * p[rows].  p_full: dev [n_total]; out: dev [n_local]. */
int cglb_matvec(cglb_ctx* ctx, const void* p_full, void* out_local);
/* same, and pdot[0] = sum over local rows of p_i * out_i  ((p * Ap).sum(), conjugate_gradient.py:67). pdot: dev double[1]. */
int cglb_matvec_dot(cglb_ctx* ctx, const void* p_full, void* out_local, void* pdot);
/* right-hand side of the solve: out_local = y[rows] - mean  (err, models.py:253-254). */
int cglb_shard_rhs(cglb_ctx* ctx, void* out_local);
/* Rectangular kernel mat-vec  out[i] = sum_j k(xnew_i, x_j) v_j  (ksf @ v, models.py:320,334).
 * xnew: any [n_new, d]; v_full: dev [n_total]; out: dev [n_new]. Sums over ALL n_total columns. */
int cglb_cross_matvec(cglb_ctx* ctx, const void* xnew, int64_t n_new, const void* v_full, void* out);

/* ---- preconditioner seam: NystromPreconditioner.__call__, conjugate_gradient.py:95-113 ------------ */
/* single shard: z = (Q_ff + noise I)^-1 r, rz = r^T z.  r,z: dev [n]; rz: host. */
int cglb_precond_apply(cglb_ctx* ctx, const void* r, void* z, double* rz);
/* sharded: u_partial[m] = A_loc r_loc (host all-reduces u), then z_loc and the partial sum of rz. */
int cglb_shard_precond_u(cglb_ctx* ctx, const void* r_local, void* u_partial /* dev [m] */);
int cglb_shard_precond_z(cglb_ctx* ctx, const void* r_local, const void* u /* dev [m], reduced */,
                         void* z_local, void* rz_partial /* dev [1], or NULL when the caller forms r^T z itself */);

/* segmented form for the cyclic multi-GPU path: z_slot is this rank's slice of the all-gather buffer, dev [per + 1]: z for the local
 * rows in [0, n_local) and, in element `per`, this rank's partial of r^T z over its own rows (in the vector element type). */
int cglb_shard_precond_z_seg(cglb_ctx* ctx, const void* r_local, const void* u /* dev [m], reduced */, void* z_slot, int64_t per);

/* ---- vector primitives of the PCG loop (conjugate_gradient.py:67-75), for the sharded host loop ---- */
/* dot: out[0] = sum_i a_i b_i over local rows (dev scalar, deterministic order). */
int cglb_shard_dot(cglb_ctx* ctx, const void* a_local, const void* b_local, void* out /* dev [1] */);
/* v += gamma p ; r -= gamma Ap  with gamma = rz / pAp read from device scalars (:67-68,:72). */
int cglb_shard_update_v_r(cglb_ctx* ctx, void* v_local, void* r_local, const void* p_local, const void* Ap_local,
                          const void* rz /* dev [1] */, const void* pAp /* dev [1] */, int update_r);
/* r = b - Kv (restart / initial residual, :58,:72). */
int cglb_shard_residual(cglb_ctx* ctx, void* r_local, const void* b_local, const void* Kv_local);
/* p = z + p * (new_rz / rz)  or  p = z on restart (:75). */
int cglb_shard_update_p(cglb_ctx* ctx, void* p_local, const void* z_local, const void* new_rz /* dev [1] */,
                        const void* rz /* dev [1] */, int restart);

/* ---- solver seam: ConjugateGradient.__call__, conjugate_gradient.py:41-86 (single shard) ---------- */
/* Solves (K_ff + noise I) v = b warm-started at v_inout (overwritten with the solution; the Python shim
 * clones first so the caller's tensor is not mutated, :55).  Stops when 1/2 r^T P r <= max_error or
 * steps == max_cg_iter, predicate tested before every iteration (:65); exact-residual restart when
 * i % restart_cg_iter == restart_cg_iter-1 (:70-75).  steps / half_rz mirror ConjugateGradientStats (:25-28). */
int cglb_pcg_solve(cglb_ctx* ctx, const void* b /* dev [n] */, void* v_inout /* dev [n] */, double max_error,
                   int max_cg_iter, int restart_cg_iter, int* steps, double* half_rz);

/* ---- objective seam: LowerBoundCG.forward + quad_estimator, models.py:151-174, :246-286, and its
 *      gradient as torch.autograd.grad yields it with v detached (pytorch/optimizer.py:95-98) -------- */
/* Runs cglb_setup, (optionally) the PCG from v_inout with b = y - mean, the bound assembly and the
 * gradient.  out4 = {bound, lower, upper, logdet} (host); grad: host double[CGLB_GRAD_LEN(d,m)] or NULL
 * (value only).  v_inout: dev [n] — the persistent warm-start vector (models.py:59-72, :274). */
int cglb_objective_and_grad(cglb_ctx* ctx, void* v_inout, int run_cg, double max_error, int max_cg_iter,
                            int restart_cg_iter, double* out4, double* grad, int* steps, double* half_rz);

/* TF twin only (tensorflow/models.py:36-51,161-164: `joint_optimization` makes v a trainable parameter): gradient of the bound
 * wrt v at the v of the evaluation just made, d bound / d v = K_sigma (P r) - r with r = e - K_sigma v.  Must directly follow
 * cglb_objective_and_grad (single shard); one more K_ff mat-vec.  gv_out: dev [n]. */
int cglb_objective_grad_v(cglb_ctx* ctx, void* gv_out);

/* sharded pieces of the same evaluation (host all-reduces between phases):
 *   phase1: Kv = (K+sI) v (v_full gathered), r = e - Kv, u_partial = A_loc r              -> all-reduce u[m]
 *   phase2: w = P r (local), partial scalars sc[8] and aw_partial = A_loc w               -> all-reduce sc[8], aw[m]
 *   phase3: partial packed gradient (dev double[GRAD_LEN]); rank-replicated terms are added by the
 *           shard with row_begin == 0 only                                               -> all-reduce grad
 *   finish: bound/lower/upper from reduced sc (host). */
int cglb_shard_obj_phase1(cglb_ctx* ctx, const void* v_full, void* u_partial);
int cglb_shard_obj_phase2(cglb_ctx* ctx, const void* v_full, const void* u /* dev [m], reduced */, void* sc_partial /* dev double[8] */,
                          void* aw_partial /* dev [m] */);
int cglb_shard_obj_phase3(cglb_ctx* ctx, const void* v_full, const void* sc /* dev double[8], reduced */,
                          const void* aw /* dev [m], reduced */, void* grad_partial /* dev double[GRAD_LEN] */);
int cglb_shard_obj_finish(cglb_ctx* ctx, const void* sc /* dev double[8], reduced */, double* out4);

/* ---- cyclic-symmetric multi-GPU path ----------------------------------------------------------------------------
 * K_ff is symmetric, and the symmetric pair kernel (each kappa_ij used for out_i and out_j) halves the work of a mat-vec.
 * To keep that factor under sharding the GLOBAL upper triangle is dealt to the ranks by cyclic 256-row blocks:
 * cglb_matvec_cyclic produces this rank's full-length PARTIAL of (K_ff + noise I) p (the noise term is added by rank 0 only);
 * the host all-reduces it and every
 * rank holds the full vectors p, Ap, v, r (their updates are O(N) and done redundantly with the cglb_vec_* primitives).
 * Only the Nystrom panel stays column-sharded (rows [row_begin,row_end)): u = A r is all-reduced (M), z is all-gathered. */
int cglb_set_parallel(cglb_ctx* ctx, int world, int rank);
int cglb_matvec_cyclic(cglb_ctx* ctx, const void* p_full, void* out_full_partial /* dev [n_total] */);
int cglb_rhs_full(cglb_ctx* ctx, void* out_full /* dev [n_total] */); /* y - mean for all rows */
/* vector primitives with an explicit length (same kernels as the cglb_shard_* ones) */
int cglb_vec_dot(cglb_ctx* ctx, int64_t n, const void* a, const void* b, void* out /* dev double[1] */);
int cglb_vec_update_v_r(cglb_ctx* ctx, int64_t n, void* v, void* r, const void* p, const void* Ap, const void* rz, const void* pAp, int update_r);
int cglb_vec_residual(cglb_ctx* ctx, int64_t n, void* r, const void* b, const void* Kv);
int cglb_vec_update_p(cglb_ctx* ctx, int64_t n, void* p, const void* z, const void* new_rz, const void* rz, int restart);
/* p = z + p * (new_rz / rz) (or p = z) with z all-gathered in `world` slices of per + 1 elements (cglb_shard_precond_z_seg) and
 * new_rz = the sum, in rank order, of the slices' extra elements: the stop-test scalar is then identical on every rank by
 * construction.  new_rz: dev double[1], written; rz: dev double[1], the previous value (conjugate_gradient.py:75-76).
 * As in cglb_vec_update_p, rz == 0 gives a zero factor (p = z, finite); a NaN in either scalar still propagates into p.
 * With restart = 1 the value of rz is not used, so new_rz and rz may be the same slot (the first call of a solve).
 * The kernel also prepares the operand of the NEXT cglb_matvec_cyclic(p): p must not be modified in between (the PCG loop does not). */
int cglb_vec_update_p_seg(cglb_ctx* ctx, int64_t n, int64_t per, int world, void* p, const void* zseg, void* new_rz, const void* rz, int restart);
int cglb_vec_axpy(cglb_ctx* ctx, int64_t n, double alpha, const void* x, void* y); /* y += alpha x */
/* objective phase 1 with (K_ff + noise I) v already computed for the local rows; phase 2 unchanged; the local slice of
 * w = P r for the all-gather of u = w + v/2; phase 3 with the cyclic share of the N^2 gradient form (u_full gathered).
 * Placement of that share: the global upper triangle of the symmetric form is dealt by row blocks, block b to rank b mod world, like the
 * mat-vec's, but the block size is that of the gradient kernel's instance (256 threads x 1, 2 or 4 rows, chosen from the padded input width,
 * the dtype and the option grad_gram; tiles on the wide path) and not the mat-vec's 256 rows.  Only the sum over the ranks of the lengthscale
 * entries is defined by this interface; every other entry of grad_partial is placed as in cglb_shard_obj_phase3. */
int cglb_shard_obj_phase1_kv(cglb_ctx* ctx, const void* Kv_local, void* u_partial);
int cglb_shard_obj_w(cglb_ctx* ctx, void* w_local_out);
int cglb_shard_obj_phase3_cyclic(cglb_ctx* ctx, const void* v_full, const void* u_full, const void* sc, const void* aw, void* grad_partial);

/* ---- prediction seam: PredictCG.forward, models.py:307-354 (needs common terms + a solved v) ------ */
/* f_mean, f_var: dev [n_new].  v_full: dev [n] solution at tolerance 1e-3 (models.py:291). single shard. */
int cglb_predict(cglb_ctx* ctx, const void* v_full, const void* xnew, int64_t n_new, void* f_mean, void* f_var);
/* sharded pieces of the same computation (host or library all-reduces between them):
 *   _u:    res = (y - mean) - Kv over the local rows (models.py:335), u_partial = A_loc res (:340)             -> all-reduce u[m]
 *   _rows: c = LB^-1 u / sigma (:343) and, for the new points handed to THIS rank (any subset of the rows of xnew - the driver deals
 *          contiguous slices to the ranks and all-gathers the results), cg_mean = k(xnew, X) v over ALL n_total columns (:334),
 *          tmp1, tmp2 (:344-345), f_mean, f_var (:347-351). */
int cglb_shard_predict_u(cglb_ctx* ctx, const void* Kv_local /* dev [n_local]: (K_ff + noise I) v on the local rows */, void* u_partial /* dev [m] */);
int cglb_shard_predict_rows(cglb_ctx* ctx, const void* v_full, const void* u /* dev [m], reduced */, const void* xnew, int64_t n_new, void* f_mean,
                            void* f_var);

/* ---- N ranks inside the library ------------------------------------------------------------------------------------
 * The cyclic-symmetric scheme above with its collectives issued by the library itself on the context stream, so that a PCG
 * iteration at world N is enqueued like the single-GPU one: no host work between the kernels of an iteration except the one
 * read-back of the stop statistic (conjugate_gradient.py:65,80-81), which the look-ahead hides.  One process per GPU; every
 * rank makes the same calls with the same arguments.  The context must own the rows of the contiguous partition
 * [rank * per, min((rank + 1) * per, n_total)), per = ceil(n_total / world), and use the stored-panel preconditioner.
 *   cglb_comm_get_unique_id: rank 0 obtains the RCCL id (CGLB_COMM_ID_BYTES bytes) and hands it to the other ranks through the
 *     launcher's store (torch.distributed's TCPStore in cglb_amd/dist_context.py); cglb_comm_init_rccl is collective.
 *   cglb_comm_init_callbacks: the same loops over collectives the HOST provides (buffers are device pointers of the context's
 *     device; in place; the callback must order itself after the work already enqueued on `stream` and leave the result visible
 *     to work enqueued on `stream` afterwards; return 0 on success).  Used to run the library's N-rank loops over gloo in the
 *     tests (several ranks sharing one GPU, which RCCL refuses) and available for any other fabric. */
#define CGLB_COMM_ID_BYTES 128
typedef int (*cglb_allreduce_fn)(void* user, void* buf, int64_t count, int dtype /* CGLB_F64 | CGLB_F32 */, void* stream);
/* in place: rank g's contribution sits at element g * count_per_rank of buf (world * count_per_rank elements) */
typedef int (*cglb_allgather_fn)(void* user, void* buf, int64_t count_per_rank, int dtype, void* stream);
int cglb_comm_get_unique_id(void* id_out /* host, CGLB_COMM_ID_BYTES */);
int cglb_comm_init_rccl(cglb_ctx* ctx, const void* unique_id /* host, CGLB_COMM_ID_BYTES */, int world, int rank);
int cglb_comm_init_callbacks(cglb_ctx* ctx, int world, int rank, cglb_allreduce_fn allreduce, cglb_allgather_fn allgather, void* user);
int cglb_comm_destroy(cglb_ctx* ctx);
/* common terms with B = I + sum_g A_g A_g^T (one all-reduce of m x m) */
int cglb_dist_setup(cglb_ctx* ctx);
/* out = (K_ff + noise I) x, full length on every rank (this rank's cyclic share + all-reduce). x_full, out_full: dev [n_total] */
int cglb_dist_matvec(cglb_ctx* ctx, const void* x_full, void* out_full);
/* z = (Q_ff + noise I)^-1 r on full replicated vectors; rz: host, may be NULL */
int cglb_dist_precond_apply(cglb_ctx* ctx, const void* r_full, void* z_full, double* rz);
/* cglb_pcg_solve / cglb_objective_and_grad / cglb_predict on N ranks: vectors are full length and replicated (b_full, v_full_inout,
 * f_mean, f_var identical on every rank afterwards); host outputs are identical on every rank.  The stop test is taken on
 * all-gathered per-rank partials of r^T P r, so every rank leaves the loop at the same step by construction. */
int cglb_dist_pcg_solve(cglb_ctx* ctx, const void* b_full, void* v_full_inout, double max_error, int max_cg_iter, int restart_cg_iter,
                        int* steps, double* half_rz);
int cglb_dist_objective_and_grad(cglb_ctx* ctx, void* v_full_inout, int run_cg, double max_error, int max_cg_iter, int restart_cg_iter,
                                 double* out4, double* grad, int* steps, double* half_rz);
int cglb_dist_predict(cglb_ctx* ctx, const void* v_full, const void* xnew, int64_t n_new, void* f_mean, void* f_var);

/* ---- multi-output targets: Y[N, P] with one shared kernel, mean and noise (tensorflow/models.py:45-47 v0 as [B, N], :90-104 the log-det
 *      term times output_dim, :183-187 the constant -N P/2 log 2 pi, :245 the variance tiled over the outputs) ------------------------------
 * Every multi-column array is [P, N]: column b is a contiguous length-N vector at offset b * N, so every single-vector entry point works
 * on one column by pointer offset.  One shard covering all rows, one rank, logdet_bound 0 and quad_term 0.  With s = 1 / p = 1 each of
 * these calls the single-column code (bit-identical results).
 * Batched PCG: the P columns are P independent recurrences (conjugate_gradient.py:41-86 per column) with their own
 * gamma_b = rz_b / pAp_b and beta_b = rz_b' / rz_b, advancing in lockstep over ONE product K_ff P[N, P] per iteration that evaluates every
 * kernel value once for up to 8 columns (fp64, kff_variant 2, and either d <= 32 with the unclamped exponent range or 32 < d <= 96 with
 * "wide_reg" 1, both ranges; otherwise s single mat-vecs - cglb_get_stat "matmat_native" tells which).  One
 * stop test before every iteration: 1/2 sum_b r_b^T P r_b <= max_error or steps == max_cg_iter (the sum is the gap upper - lower of the
 * summed bound); the restart rule applies to all columns at once; pAp_b == 0 gives gamma_b = 0 and rz_b == 0 gives beta_b = 0 (a column
 * that is exactly converged or all zero stays finite and leaves the others unchanged). */
/* replaces the targets: Y any [p, n_total].  After cglb_set_data p = 1.  CGLB_ERR_BAD_ARG on a context with more than one rank or with
 * logdet_bound / quad_term other than 0; cglb_set_parallel, cglb_comm_init_* and those two options refuse a context with p > 1. */
int cglb_set_targets(cglb_ctx* ctx, const void* Y, int p);
/* Out[b] = (K_ff + noise I) V[b].  V: dev [s, n_total]; Out: dev [s, n_local]. */
int cglb_matmat(cglb_ctx* ctx, const void* V, int s, void* Out);
/* B, V_inout: dev [s, n].  half_rz_total = 1/2 sum_b r_b^T P r_b; half_rz_cols: host [s] (the terms of that sum) or NULL. */
int cglb_pcg_solve_multi(cglb_ctx* ctx, const void* B, void* V_inout, int s, double max_error, int max_cg_iter, int restart_cg_iter, int* steps,
                         double* half_rz_total, double* half_rz_cols);
/* V_inout: dev [p, n] for the p columns of cglb_set_targets.  bound = sum_b (-upper_b) + p logdet - n p / 2 log 2 pi;
 * out4 = {bound, sum_b lower_b, sum_b upper_b, p logdet}; grad (packed layout unchanged, one shared mean) = the sum over b of the
 * single-output gradients at v_b, the log-det part taken p times. */
int cglb_objective_and_grad_multi(cglb_ctx* ctx, void* V_inout, int run_cg, double max_error, int max_cg_iter, int restart_cg_iter, double* out4,
                                  double* grad, int* steps, double* half_rz);
/* f_mean: dev [p, n_new]; f_var: dev [n_new] (the variance does not depend on the column). */
int cglb_predict_multi(cglb_ctx* ctx, const void* V, const void* xnew, int64_t n_new, void* f_mean, void* f_var);
/* average duration (ms) of `reps` back-to-back products with s columns (pair kernel + slab combine), in the style of cglb_time_kernel(which = 0) */
int cglb_time_matmat(cglb_ctx* ctx, int s, int reps, double* ms_avg);

/* ---- exact GP regression: model class "gpr" (GPRConfig: cglb_experiments/cli.py:166-181, :196-200, :293-311; tensorflow/interface.py:200-206,
 *      :386-395 - gpflow's GPR.log_marginal_likelihood; pytorch/interface.py:561-604 - ExactMarginalLogLikelihood times n) ---------------------
 * K = variance kappa(X, X) + noise I = L L^T (dense, N x N, factored on the GPU), e = y - mean, alpha = K^-1 e,
 * lml = -1/2 e^T alpha - sum log L_ii - N/2 log 2 pi.  fp64 contexts with one shard covering all rows, one rank and one target column;
 * anything else returns CGLB_ERR_BAD_ARG.  The context is created like any other: this class has no inducing points, so the caller passes
 * m = 1 as a placeholder, and none of these entry points calls cglb_setup or reads Z or the Nystrom panel.  Device memory: 8 N^2 bytes for
 * the factor, 8 N^2 more once a gradient is asked for, checked against the free device memory before they are allocated; released by
 * cglb_ctx_destroy and by a changed "gpr_block". */
/* lengthscales: host double[d].  No inducing points, no jitter.  The noise need not be positive: a matrix that is not positive definite is
 * reported by the evaluation (CGLB_ERR_NOT_PD with the row of the first non-positive pivot). */
int cglb_gpr_set_hypers(cglb_ctx* ctx, const double* lengthscales, double variance, double noise, double mean);
/* out3 = {lml, -1/2 e^T alpha, -sum log L_ii} (host).  grad: host double[d + 3] = d lml / d {lengthscales, variance, noise, mean}, or NULL
 * (value only: no inverse is formed).  With W = alpha alpha^T - K^-1: 1/2 sum_ij W_ij dK_ij/dl_d, 1/2 sum_ij W_ij kappa_ij, 1/2 tr W,
 * sum alpha.  Two evaluations of the same inputs return bitwise equal numbers. */
int cglb_gpr_objective_and_grad(cglb_ctx* ctx, double* out3, double* grad);
/* predict_f at new points (gpflow GPR.predict_f, full_cov = False): f_mean = mean + K_*f alpha, f_var = variance - |L^-1 K_f*|^2 column-wise.
 * xnew: any [n_new, d]; f_mean, f_var: dev [n_new].  Uses the factor of the last evaluation at the current data and hyper-parameters and
 * factors first if there is none. */
int cglb_gpr_predict(cglb_ctx* ctx, const void* xnew, int64_t n_new, void* f_mean, void* f_var);

/* ---- iterative exact GP regression: model class "itergp" - the "Iterative GP" baseline of the paper (cglb_experiments/cli.py:293-311 and
 *      pytorch/interface.py:233-260, :561-604 build it on gpytorch: modified batched CG, a pivoted-Cholesky preconditioner of rank _prec_size() = 100,
 *      stochastic Lanczos quadrature for the log-determinant).  gpytorch's random numbers and stop rule are not reproduced; the estimator is
 *      defined here and pinned to tests/itergp_ref.py.  O(N) memory.  fp64 contexts with one shard covering all rows, one rank, one target
 *      column, logdet_bound 0, quad_term 0 and the stored panel; anything else returns CGLB_ERR_BAD_ARG.
 * K = variance kappa(X, X) + noise I, e = y - mean, s = noise.  The context is created with m = k, the rank of the preconditioner (k <= n_total),
 * and cglb_set_hypers is called with any Z: every evaluation replaces Z by the k training points the greedy selection of cglb_select_inducing
 * picks under the CURRENT hyper-parameters (the pivoted Cholesky of K_ff, jitter included) and runs cglb_setup, so that P = Q_ff + s I with
 * A = L^-1 K_uf / sqrt(s) the stored panel and log|P| = N log s + 2 sum log diag LB.
 *   probes   z_i = sqrt(s) (A^T eps_i[:k] + eps_i[k:]), i < t, from the caller's eps [t, k + n_total] (any; standard normal entries give z_i ~ N(0, P);
 *            the library draws no random numbers)
 *   solve    one batched PCG (cglb_pcg_solve_multi's loop) on [e, z_1 .. z_t]: column 0 warm-started at v_inout (dev [n], overwritten with alpha),
 *            the probe columns from zero, no restart steps, stop on 1/2 sum_b r_b^T P^-1 r_b <= max_error or max_cg_iter steps; rz_j,b and
 *            pAp_j,b of every iteration are kept
 *   log|K|   ~ log|P| + (1/t) sum_i rz_0,i e_1^T log(T_i) e_1, T_i the Lanczos tridiagonal of probe i from gamma_j = rz_j / pAp_j and
 *            beta_j = rz_{j+1} / rz_j: T[j][j] = 1/gamma_j + beta_{j-1}/gamma_{j-1}, T[j][j+1] = sqrt(beta_j)/gamma_j, of min(steps, lanczos_iter)
 *            rows, cut at the first zero or non-finite gamma_j or rz_j (csrc/slq_host.h, host)
 *   out4     {lml, -1/2 e^T alpha, -1/2 log|K| (the estimate), log|P|},  lml = out4[1] + out4[2] - n/2 log 2 pi
 *   grad     host double[d + 3] = {lengthscales, variance, noise, mean} or NULL: sum_b u_b^T (dK/d theta) v_b with (u_0, v_0) = (alpha / 2, alpha)
 *            and (u_i, v_i) = (-a_i / (2 t), P^-1 z_i), a_i = K^-1 z_i - the usual unbiased estimate, NOT the derivative of the returned value
 *            (P is treated as constant); the mean entry is sum alpha.  The 1 + t bilinear forms run through cglb_grad_kff_multi's pass.
 * Two evaluations with the same inputs return bitwise equal numbers.  CGLB_ERR_NOT_PD if a tridiagonal has an eigenvalue that is not positive. */
int cglb_itergp_objective_and_grad(cglb_ctx* ctx, const void* eps, int t, void* v_inout, double max_error, int max_cg_iter, int lanczos_iter,
                                   double* out4, double* grad, int* steps, double* half_rz);
/* the coefficient logs of the last cglb_itergp_objective_and_grad: rz_log host [steps + 1][1 + t], pap_log host [steps][1 + t] (column 0: the data) */
int cglb_itergp_get_coefficients(cglb_ctx* ctx, double* rz_log, double* pap_log);
/* predict_f: f_mean = mean + K_*f alpha with alpha = K^-1 e solved to max_error (warm-started at the alpha of the last evaluation at the current
 * data and hyper-parameters; without one the preconditioner is built first), f_var = variance - k_*^T K^-1 k_* by batched solves on the columns
 * of K_f*, 8 new points at a time (each to 1/2 sum_b r_b^T P^-1 r_b <= max_error): n_new / 8 solves.  The Lanczos variance cache below
 * (cglb_itergp_var_cache, cglb_itergp_predict_cached) is the opt-in that replaces these solves.  xnew: any [n_new, d]; f_mean, f_var:
 * dev [n_new].  Any input width: beyond 32 dimensions the right-hand sides come from the wide operand set, and the batched solves run on the
 * shared-kernel product up to 96 dimensions and on single mat-vecs beyond. */
int cglb_itergp_predict(cglb_ctx* ctx, const void* xnew, int64_t n_new, double max_error, int max_cg_iter, void* f_mean, void* f_var);
/* Lanczos variance cache: what the reference's exact-GP metrics get from gpytorch.settings.fast_pred_var() (pytorch/interface.py:582) - a low-rank
 * approximation of K^-1 built once and applied to every new point.  gpytorch's start vector is not reproduced; the estimator is defined here and
 * pinned to tests/love_ref.py.  Scope of cglb_itergp_predict (fp64, one rank, one target column, any input width; else CGLB_ERR_BAD_ARG).
 *   Lanczos  on K = variance kappa(X, X) + noise I with full reorthogonalisation, started at q_0 = e / |e|, e = y - mean (CGLB_ERR_STATE if e = 0):
 *            w = K q_j (the context's own mat-vec), alpha_j = q_j^T w, two passes w <- w - Q (Q^T w) over all columns so far, beta_j = |w|;
 *            stop with J = j + 1 columns when j + 1 = rank or beta_j <= 1e-10 alpha_0 (the Krylov space has closed: with an RBF kernel K has
 *            about a hundred numerically distinct eigenvalues - this is a normal end, not an error), else q_{j+1} = w / beta_j
 *   factor   T = tridiag(alpha, beta) = L L^T on the host, L lower bidiagonal (csrc/lanczos_host.h); CGLB_ERR_NOT_PD at a pivot that is not positive
 *   cache    R = Q L^-T (R_j = (Q_j - l_{j-1} R_{j-1}) / d_j), so that K^-1 ~ R R^T; dev [n_total][rank rounded up to 8] row-major in a grow-only
 *            buffer of the context, zero beyond column J: the cache row of a training point is one contiguous scalar load
 *   variance f_var(x*) = variance - sum_s (sum_j variance kappa(x*, x_j) R[j, s])^2
 * A Galerkin projection of K^-1: f_var is never below the exact variance, does not increase with the rank and is exact at J = n_total.  It is an
 * APPROXIMATION - an upper bound that tightens with the rank (DESIGN.md section 4f has measured overestimates).  1 <= rank <= min(n_total, 1024);
 * rank_out = J.  Two builds on the same inputs give bitwise equal caches.  cglb_set_data, cglb_set_hypers, cglb_set_targets and
 * cglb_select_inducing invalidate the cache. */
int cglb_itergp_var_cache(cglb_ctx* ctx, int rank, int* rank_out);
/* cglb_itergp_predict with the variance from the cache: f_mean as there (the same solve for alpha, the same product), f_var from one
 * multi-column product K_*f R (cglb_cross_matmat's kernel; beyond 32 input dimensions the Gram tiles of csrc/kernels_wide.hip: Gram GEMM, kernel
 * profile in place and one GEMM of the tile against the matching cache rows) and the row norms of the result.  CGLB_ERR_STATE without a valid cache. */
int cglb_itergp_predict_cached(cglb_ctx* ctx, const void* xnew, int64_t n_new, double max_error, int max_cg_iter, void* f_mean, void* f_var);
/* The product of the cached predictive on its own (tests, timing): out[i, s] = variance sum_j kappa(xnew_i, x_j) V[s, j].  xnew: any [n_new, d];
 * V: dev [S, n_total], column s contiguous (the convention of cglb_grad_kff_multi); out: dev [n_new, S] row-major.  Every kernel value is
 * evaluated once per group of 8 columns (csrc/kernels_cross_multi.hip); always the range-clamped 2^x; bitwise reproducible.  Scope of
 * cglb_itergp_predict_cached, and d <= 32: this is the entry of the register-resident kernel (CGLB_ERR_BAD_ARG on wider inputs). */
int cglb_cross_matmat(cglb_ctx* ctx, const void* xnew, int64_t n_new, const void* V, int S, void* out);
/* average duration (ms) of `reps` back-to-back products with S > 0 columns (operand interleave, pair kernel and fixed-order sum of every group, on
 * the context stream) at the first n_new training rows as new points (n_new <= n_total), beside cglb_time_grad_kff_multi; S < 0 times the
 * comparison side instead: |S| single products of cglb_cross_matvec's kernel on the same operands */
int cglb_time_cross_matmat(cglb_ctx* ctx, int64_t n_new, int S, int reps, double* ms_avg);
/* Random-Fourier-feature product, the prior term of a pathwise sample (csrc/kernels_feature_multi.hip):
 *   out[i, s] = sqrt(2 variance / F) sum_{j < F} W[s, j] cos( sum_k omega[j, k] (x_ik - c_k) / l_k + b_j )
 * with l the current lengthscales and c the training column means the context centres by.  x: any [n_rows, d], or NULL for the training rows
 * (n_rows = n_total); omega: any (host or device) [F, d]; phase: any [F] (b, radians); W: dev [S, F], column s contiguous (the convention of
 * cglb_cross_matmat); out: dev [n_rows, S] row-major.  The n_rows x F feature matrix is never formed: every cosine is evaluated once per group of
 * 8 columns, by the branch-free cos_turns of csrc/devmath.h (absolute error <= 3e-16 at any phase magnitude; the "precision" option does not
 * apply).  Bitwise reproducible.  Scope of cglb_itergp_predict (fp64, one rank, one target column, any input width; else CGLB_ERR_BAD_ARG).
 * "feature_ms" (cglb_get_stat): device time of the last product. */
int cglb_feature_matmat(cglb_ctx* ctx, const void* x, int64_t n_rows, const void* omega, const void* phase, const void* W, int64_t F, int S, void* out);
/* average duration (ms) of `reps` back-to-back feature products (operand records, kernel and fixed-order sum of every group, on the context
 * stream) of F features and S columns at the first n_rows training rows (n_rows <= n_total), beside cglb_time_cross_matmat */
int cglb_time_feature_matmat(cglb_ctx* ctx, int64_t n_rows, int64_t F, int S, int reps, double* ms_avg);
/* predict_f_samples by pathwise conditioning (Matheron's rule with a random-feature prior; Wilson et al. 2020), S samples at once:
 *   f_s = mean + Phi(X*) w_s + K_*f U_s,   U_s = K^-1 (e - Phi(X) w_s - sqrt(noise) eps_s),   K = variance kappa(X, X) + noise I,  e = y - mean
 * with Phi w the product of cglb_feature_matmat.  The library draws no random numbers: omega [F, d], phase [F] (any), W (dev [S, F]) and eps
 * (any [S, n_total]) are the caller's; with standard normal W and eps, phases uniform on [0, 2 pi) and omega drawn from the spectral measure of the
 * unit-lengthscale kernel, each f_s is a draw of the posterior of the GP whose PRIOR is the F-feature approximation of the kernel, conditioned
 * through the exact K: exact for that prior up to the solve's tolerance, and the mean over draws is the exact predictive mean for ANY omega and
 * phase.  The feature approximation itself (covariance error O(1 / sqrt(F))) is a property of the estimator, not of this implementation.
 *   solve    one batched PCG (cglb_pcg_solve_multi's loop) on the S columns from zero with the class's preconditioner - the one of the last
 *            evaluation at the current data and hyper-parameters; without one it is built first, as in cglb_itergp_predict - no restart steps, stop
 *            on 1/2 sum_s r_s^T P^-1 r_s <= max_error or max_cg_iter steps (steps, half_rz: as returned by that loop)
 *   bound    P = Q_ff + noise I with the Nystrom term Q_ff (jitter included) below K_ff in the Loewner order, so P is below K and
 *            r_s^T K^-1 r_s <= r_s^T P^-1 r_s, the sum of which over s is <= 2 max_error at the stop; with
 *            d_s = K^-1 r_s the error of U_s, |k_*^T d_s| <= sqrt(k_*^T K^-1 k_*) sqrt(r_s^T K^-1 r_s) <= sqrt(variance) sqrt(2 max_error): every
 *            sample value is within sqrt(2 variance max_error) of its value at the exact solve
 *   product  K_*f U through cglb_cross_matmat's kernel up to 32 input dimensions, column by column through cglb_cross_matvec's beyond
 * f_out: dev [S, n_new], sample s contiguous; U_out: dev [S, n_total] or NULL (the solves, for tests).  Two calls with the same inputs return
 * bitwise equal samples.  The stored alpha and the variance cache are left as they are.  Scope of cglb_itergp_predict. */
int cglb_itergp_sample(cglb_ctx* ctx, const void* xnew, int64_t n_new, const void* omega, const void* phase, const void* W, const void* eps, int64_t F,
                       int S, double max_error, int max_cg_iter, void* f_out, void* U_out, int* steps, double* half_rz);
/* ---- input gradients of predictive and sample paths (csrc/kernels_input_grad.hip, csrc/kernels_input_grad_mid.hip) ----
 * All gradients below are with respect to the RAW coordinates of the new point (not centred, not scaled).  Scope of every entry: that of
 * cglb_itergp_predict (fp64, one rank, one target column, the default bound) and d <= 32; else CGLB_ERR_BAD_ARG with a message ("... no wide path
 * yet ...").  OPT-IN beyond: cglb_set_option(ctx, "input_grad_mid", 1) opens every entry below at 33 <= d <= 96 on a context whose option
 * "wide_reg" is on (the default): the same contracts, a new point shared by four lanes, 4 columns per group up to d = 64 and 2 beyond, 64 new points
 * per workgroup.  The option defaults to 0, where behaviour, messages and results are unchanged; on a narrow context it changes nothing.  The
 * statistic "input_grad_native" is 1 where the next call would run a register-resident instance (narrow or mid), 0 where it would be refused.
 * Not covered: fp32, N ranks, d > 96, "wide_reg" 0.  The gpr / cglb / sgpr predictors have their own entries further down (cglb_predict_grad, cglb_gpr_predict_grad),
 * under the same option.
 *
 * Value and input gradient of K_*f V in one pass over the pairs:
 *   out [i, s]    =  variance sum_j kappa(x*_i, x_j) V[s, j]
 *   gout[i, s, k] = -variance sum_j h(x*_i, x_j) (x*_ik - x_jk) / l_k^2 V[s, j]
 * h: the radial derivative factor of the lengthscale gradient (RBF kappa; Matern-3/2 3 e^(-sqrt3 r); Matern-5/2 (5/3)(1 + sqrt5 r) e^(-sqrt5 r)).
 * xnew, V: the convention of cglb_cross_matmat; out: dev [n_new, S] or NULL; gout: dev [n_new, S, d], k fastest.  A pair is formed from direct
 * differences (not the Gram chain), so a coincident pair adds exactly zero to the gradient and nothing is NaN at r = 0; always the range-clamped
 * 2^x.  One evaluation of a pair serves a group of 8 (d_p <= 8), 4 (d_p <= 16) or 2 columns.  No atomics: bitwise reproducible, and gout is
 * bitwise the same with out NULL. */
int cglb_cross_grad_matmat(cglb_ctx* ctx, const void* xnew, int64_t n_new, const void* V, int S, void* out, void* gout);
/* average duration (ms) of `reps` back-to-back value-and-gradient products with S columns, on the operands of cglb_time_cross_matmat */
int cglb_time_cross_grad_matmat(cglb_ctx* ctx, int64_t n_new, int S, int reps, double* ms_avg);
/* Value and input gradient of the random-feature product (arguments of cglb_feature_matmat; out may be NULL; gout: dev [n_rows, S, d]):
 *   out [i, s]    =  sqrt(2 variance / F) sum_j W[s, j] cos(phi_ij),   phi_ij = sum_k omega[j, k] (x_ik - c_k) / l_k + b_j
 *   gout[i, s, k] = -sqrt(2 variance / F) sum_j W[s, j] sin(phi_ij) omega[j, k] / l_k
 * One phase and one range reduction per (row, feature) serve cosine and sine (sincos_turns of csrc/devmath.h: absolute error <= 3e-16 each at any
 * phase magnitude).  Bitwise reproducible. */
int cglb_feature_grad_matmat(cglb_ctx* ctx, const void* x, int64_t n_rows, const void* omega, const void* phase, const void* W, int64_t F, int S, void* out,
                             void* gout);
/* average duration (ms) of `reps` back-to-back value-and-gradient feature products, on the operands of cglb_time_feature_matmat */
int cglb_time_feature_grad_matmat(cglb_ctx* ctx, int64_t n_rows, int64_t F, int S, int reps, double* ms_avg);
/* Predictive mean, variance and their input gradients.  f_mean (dev [n_new]) is bitwise that of cglb_itergp_predict / cglb_itergp_predict_cached
 * (same solve for alpha, same mean routine); g_mean (dev [n_new, d]) = grad (K_*f alpha), the gradient product with the stored alpha as its single
 * column: within sqrt(C variance) / l_k sqrt(2 max_error) of the gradient at the exact solve (C = 1, 3, 5/3 by kind: the prior variance of
 * df / dx_k is C variance / l_k^2, and the bound of cglb_itergp_sample applies with it in the place of the variance).
 * f_var, g_var (dev [n_new], [n_new, d]): both NULL or both set; they need a valid variance cache (CGLB_ERR_STATE otherwise).  f_var is bitwise
 * that of cglb_itergp_predict_cached; g_var[i, k] = -2 sum_s B[i, s] G[i, s, k] with B = K_*f R and G its input gradient, contracted in column
 * order, the new points taken in row blocks so that the G workspace is bounded.  g_var is the exact gradient of the CACHE's variance (the
 * Galerkin upper bound f - |R^T k_*|^2), not of the exact variance.  The stored alpha and the variance cache stay valid. */
int cglb_itergp_predict_grad(cglb_ctx* ctx, const void* xnew, int64_t n_new, double max_error, int max_cg_iter, void* f_mean, void* g_mean, void* f_var,
                             void* g_var);
/* ---- input gradients of the CGLB, SGPR and exact-GP predictive (csrc/kernels_predict_grad.hip, csrc/kernels_predict_grad_mid.hip) ----
 * Gradients with respect to the RAW coordinates of the new point, as above.  d <= 32; OPT-IN beyond, as above: cglb_set_option(ctx,
 * "input_grad_mid", 1) opens the four entries below at 33 <= d <= 96 on a context whose option "wide_reg" is on - the same contracts, the
 * row-weighted kernel with a new point shared by four lanes, 64 new points per workgroup; without the option such a context is refused ("... no wide
 * path yet ...").  "predict_grad_native" (cglb_get_stat) is 1 where the next cglb_predict_grad would run, 0 where it would be refused.
 * Not covered: fp32, N ranks, d > 96, "wide_reg" 0, more than one target column; CGLB_ERR_BAD_ARG with a message.
 *
 * Row-weighted value and input gradient of a cross product, one pass over the pairs for up to two weights:
 *   out_u[i] =  variance sum_m u[m]     kappa(x*_i, p_m)     gout_u[i, k] = -variance sum_m u[m]     h(x*_i, p_m) (x*_ik - p_mk) / l_k^2
 *   out_w[i] =  variance sum_m Wt[m, i] kappa(x*_i, p_m)     gout_w[i, k] = -variance sum_m Wt[m, i] h(x*_i, p_m) (x*_ik - p_mk) / l_k^2
 * set: 0 the training inputs (n_pts = n_total), 1 the inducing points Z of the current hyper-parameters (n_pts = m).  xnew: any [n_new, d];
 * u: dev [n_pts] or NULL; Wt: dev [n_pts, ldw] or NULL, the new-point index fastest, ldw >= n_new (the layout of the predictive panels; what the
 * columns [n_new, ldw) hold never reaches an output); at least one of the two.  out_*: dev [n_new]; gout_*: dev [n_new, d], k fastest; the outputs
 * of an absent weight must be NULL, any output of a present one may be.  Pairs from direct differences, always the range-clamped 2^x, as
 * cglb_cross_grad_matmat: a coincident pair adds exactly zero to the gradient.  No atomics: bitwise reproducible, and every output is bitwise the
 * same whichever of the others are requested.  Scope: a context with hyper-parameters set (cglb_set_hypers), fp64, one rank, d <= 32 (33 ... 96 under
 * "input_grad_mid"; the inducing points in the kernel's units at that width are staged on the first call after cglb_set_hypers that needs them).
 * "predict_grad_kernel_ms" (cglb_get_stat): device time of the pair kernel and slab sums of the last product. */
int cglb_cross_grad_weighted(cglb_ctx* ctx, int set, const void* xnew, int64_t n_new, const void* u, const void* Wt, int64_t ldw, void* out_u, void* gout_u,
                             void* out_w, void* gout_w);
/* cglb_predict with the input gradients of both outputs.  f_mean, f_var (dev [n_new]) come from the routines of cglb_predict and are bitwise its
 * outputs; g_mean, g_var: dev [n_new, d], k fastest; f_var and g_var are both NULL or both set.  With tmp1 = L^-1 K_u*, tmp2 = LB^-1 tmp1 and
 * c = LB^-1 A res / sigma of cglb_predict:
 *   g_mean[i, k] = grad (K_*f v)[i, k] + sum_m q_m dk(x*_i, z_m)/dx*_k,    q = L^-T LB^-T c
 *   g_var [i, k] = -2 sum_m C^T[m, i] dk(x*_i, z_m)/dx*_k,                 C^T = L^-T (tmp1 - LB^-T tmp2)   (f_var = variance - sum_m C^T[m, i] k(x*_i, z_m))
 * grad (K_*f v) is cglb_cross_grad_matmat's product with v as its single column (quad_term 1: skipped, v is not read); the sums over m are ONE launch
 * of the row-weighted kernel against Z.  Scope: that of cglb_predict (quad_term 0 and 1, every logdet_bound) in fp64, on one rank, with one
 * target column and d <= 32 (33 ... 96 under "input_grad_mid").  v, the common terms and every cached state are left as they are. */
int cglb_predict_grad(cglb_ctx* ctx, const void* v_full, const void* xnew, int64_t n_new, void* f_mean, void* g_mean, void* f_var, void* g_var);
/* cglb_gpr_predict with the input gradients of both outputs, in its batches.  f_mean, f_var are bitwise those of cglb_gpr_predict (the same gemv,
 * trsm and column-norm calls).  g_mean = sum_j alpha_j dk_ij, g_var = -2 sum_j C[j, i] dk_ij with C = K^-1 K_f* from one further trsm on the
 * panel, transposed to [n_total][ld]: one launch of the row-weighted kernel against X per batch.  X and each batch are staged in the kernel's units
 * at the class's own lengthscales.  The extra 8 n_total (batch + d_p) bytes are checked against the free device memory first.  d <= 32 (33 ... 96
 * under "input_grad_mid": d_p is the hot width 48, 64, 80 or 96 there). */
int cglb_gpr_predict_grad(cglb_ctx* ctx, const void* xnew, int64_t n_new, void* f_mean, void* g_mean, void* f_var, void* g_var);
/* average duration (ms) of `reps` back-to-back cglb_predict (with_grad 0) or cglb_predict_grad (with_grad 1) calls at the first n_new training rows
 * as new points (n_new <= n_total) and v = 0, HIP events on the context stream */
int cglb_time_predict_grad(cglb_ctx* ctx, int64_t n_new, int with_grad, int reps, double* ms_avg);
/* Sample paths that are solved once.  cglb_itergp_paths_solve is the first half of cglb_itergp_sample (the same code): the right-hand sides
 * e - Phi(X) w_s - sqrt(noise) eps_s and one batched solve from zero with the class's preconditioner; U_out: dev [S, n_total], bitwise the U_out of
 * cglb_itergp_sample for the same draws.  cglb_itergp_paths_eval runs NO solve:
 *   f_s(x*) = mean + Phi(x*) w_s + K_*f U_s          f_out: dev [S, n_new]
 *   grad f_s(x*) = grad Phi(x*) w_s + grad K_*f U_s   g_out: dev [S, n_new, d], or NULL
 * With g_out NULL the values go through the kernels of cglb_itergp_sample and are bitwise its samples when U is that call's U_out; with g_out
 * set, values and gradients come from the two fused products above.  omega, phase, W: as in cglb_itergp_sample, at the CURRENT lengthscales and
 * data - U is only meaningful at the hyper-parameters and data it was solved at (the caller keeps track; the backend's PathsIterGPR does). */
int cglb_itergp_paths_solve(cglb_ctx* ctx, const void* omega, const void* phase, const void* W, const void* eps, int64_t F, int S, double max_error,
                            int max_cg_iter, void* U_out, int* steps, double* half_rz);
int cglb_itergp_paths_eval(cglb_ctx* ctx, const void* xnew, int64_t n_new, const void* omega, const void* phase, const void* W, const void* U, int64_t F,
                           int S, void* f_out, void* g_out);
/* The gradient pass of the class on its own (tests, timing): out host double[d + 1], out[k] = sum_b u_b^T (dK_ff / dl_k) v_b for k < d and
 * out[d] = sum_b u_b^T kappa v_b (kappa = K_ff / variance), b < S.  U, V: dev [S, n_total], pair b contiguous.  Every kernel value is evaluated
 * once per unordered pair for up to 8 pairs of vectors (fp64, d <= 32: csrc/kernels_grad_multi.hip; 33 ... 96 dimensions with "wide_reg" and
 * "grad_multi_mid" 1: csrc/kernels_grad_multi_mid.hip, where a single left-over pair takes the single pass; everything else runs S single passes -
 * cglb_get_stat "grad_multi_native" tells which); S > 8 runs in groups of 8 added in group order.  Bitwise reproducible.  The scope of
 * cglb_matmat, fp64 only. */
int cglb_grad_kff_multi(cglb_ctx* ctx, const void* U, const void* V, int S, double* out);
/* average duration (ms) of `reps` back-to-back passes with S pairs (operand prep, pair kernel and fixed-order sum of every group, on the context
 * stream, no read-back), in the style of cglb_time_kernel(which = 2), which times one single pass */
int cglb_time_grad_kff_multi(cglb_ctx* ctx, int S, int reps, double* ms_avg);

/* ---- gradients with respect to the TRAINING inputs (csrc/kernels_train_input_grad.hip; no counterpart in the reference) ------------------
 * What a learned feature map in front of the kernel needs: X = g(raw), trained by back-propagating d objective / d X into g.
 *   d kappa(x_i, x_j) / d x_ik = -h_ij delta_ijk / l_k, delta_ijk = (x_ik - x_jk) / l_k         (the convention of cglb_cross_grad_matmat)
 *   gx[i, k] = sum_j w_ij variance d kappa(x_i, x_j) / d x_ik
 * with respect to the RAW coordinates.  A coincident pair (i = j, a duplicated row) has delta = 0 exactly and adds exactly zero.
 * Scope of all four entries: fp64, one rank, one target column, d <= 32, every kernel kind; elsewhere CGLB_ERR_BAD_ARG with a message
 * (cglb_get_stat "train_input_grad_native" tells which).
 *
 * cglb_grad_x_kff_multi: the standalone product of the bilinear forms of cglb_grad_kff_multi, w_ij = sum_b (u_bi v_bj + v_bi u_bj), b < S.
 * U, V: as in cglb_grad_kff_multi; gx_out: dev [n_total, d], k fastest.  The full square is swept in groups of 8 pairs (4 above 16 dimensions),
 * the groups added in order: no atomics, bitwise reproducible.  With out = cglb_grad_kff_multi(U, V):
 * sum_i x_ik gx[i, k] = -l_k out[k] and sum_i gx[i, k] = 0, both to round-off. */
int cglb_grad_x_kff_multi(cglb_ctx* ctx, const void* U, const void* V, int S, void* gx_out);
/* average duration (ms) of `reps` back-to-back passes with S pairs (operand records, pair kernel and finish of every group and row block, on the
 * context stream), beside cglb_time_grad_kff_multi */
int cglb_time_grad_x_kff_multi(cglb_ctx* ctx, int S, int reps, double* ms_avg);
/* cglb_itergp_objective_and_grad with the estimator's gradient with respect to the training inputs besides: the same evaluation - out4, grad,
 * steps, half_rz and the state left behind are bitwise those of that entry, which is the gx_out = NULL case of one implementation - then ONE further
 * pass over the 1 + t vector pairs the kernel gradient already holds, inside the "itergp_grad_ms" bracket.  grad and gx_out (dev [n_total, d]) must
 * both be set.  As grad, gx is the gradient of the ESTIMATOR (P treated as constant), not the derivative of the value in out4. */
int cglb_itergp_objective_and_grad_x(cglb_ctx* ctx, const void* eps, int t, void* v_inout, double max_error, int max_cg_iter, int lanczos_iter,
                                     double* out4, double* grad, int* steps, double* half_rz, void* gx_out);
/* cglb_gpr_objective_and_grad with the exact gradient with respect to the training inputs besides: out3 and grad are bitwise those of that entry;
 * gx_out: dev [n_total, d], w_ij = alpha_i alpha_j - K^-1_ij (half of alpha alpha^T - K^-1, counted for K_ij and K_ji), through the row-weighted
 * gradient product of cglb_gpr_predict_grad with rows = points = X, one row block of the option "gpr_block" at a time: n_total x gpr_block further
 * doubles, checked against the free device memory first. */
int cglb_gpr_objective_and_grad_x(cglb_ctx* ctx, double* out3, double* grad, void* gx_out);
/* ---- the CGLB / SGPR bounds -------------------------------------------------------------------------------------------------------------
 * cglb_objective_and_grad with the EXACT derivative of out4[0] with respect to the training inputs besides, at fixed v (detached, as the
 * hyper-parameter gradient has it), Z and hyper-parameters:
 *   gx[n, k] = sum_m (Guf[m, n] + c_m w_n) d k(z_m, x_n) / d x_nk                    (log-det, trace and preconditioner terms through K_uf)
 *            + sum_j (u_n v_j + v_n u_j) d k(x_n, x_j) / d x_nk,  u = w + v / 2       (quad_term 0 only: the term +(w + v/2)^T dK_ff v)
 * Guf, c and w are the K_uf adjoint, c = K_uu^-1 K_uf w and w = P r the hyper-parameter gradient forms; K_uu and tr K_ff do not depend on X.
 * One implementation with cglb_objective_and_grad, which is its gx_out = NULL case: out4, grad, steps, half_rz, v and the state left behind are
 * bitwise the same.  grad must be set with gx_out (dev [n_total, d], overwritten).  Two further passes: the transposed panel pass
 * (cglb_grad_x_kuf) and, with the CG quadratic term, the single-pair K_ff pass (cglb_grad_x_kff_pair); no atomics, bitwise reproducible.
 * Scope: fp64, one rank and one shard, one target column, d <= 32, logdet_bound 0 and 1, quad_term 0 and 1, precond_mode 0; elsewhere
 * CGLB_ERR_BAD_ARG with a message that names the reason (cglb_get_stat "bound_input_grad_native" tells beforehand). */
int cglb_objective_and_grad_x(cglb_ctx* ctx, void* v_inout, int run_cg, double max_error, int max_cg_iter, int restart_cg_iter, double* out4,
                              double* grad, int* steps, double* half_rz, void* gx_out);
/* The transposed panel pass on its own: gx[n, k] = sum_m (G[m * ldg + n] + cvec[m] wvec[n]) d k(z_m, x_n) / d x_nk with respect to the raw training
 * inputs, at the inducing points and hyper-parameters of the last cglb_set_hypers (no common terms needed).  G: dev [m][ldg], row m contiguous,
 * ldg >= n_total; cvec: dev [m] and wvec: dev [n_total], or both NULL; gx_out: dev [n_total, d], overwritten.  The operand sets and the evaluator of
 * the dZ reduction of the same panel; the inducing points are split into chunks (option "kuf_msplit" > 0 forces their count) whose partial sums
 * are added in fixed order.  A training point equal to an inducing point adds exactly zero.  Scope as cglb_grad_x_kff_multi. */
int cglb_grad_x_kuf(cglb_ctx* ctx, const void* G, int64_t ldg, const void* cvec, const void* wvec, void* gx_out);
/* average duration (ms) of `reps` back-to-back transposed panel passes over a panel with ldg = n_total rounded up to 32 */
int cglb_time_grad_x_kuf(cglb_ctx* ctx, int reps, double* ms_avg);
/* cglb_grad_x_kff_multi for ONE pair u, v (dev [n_total]): the kernel's G = 1 instance with more rows per lane; the same sums in another order, so
 * equal to cglb_grad_x_kff_multi(u, v, 1) to round-off, not bitwise.  cglb_grad_x_kff_multi itself is not routed here. */
int cglb_grad_x_kff_pair(cglb_ctx* ctx, const void* u, const void* v, void* gx_out);
/* average duration (ms) of `reps` back-to-back single-pair passes, beside cglb_time_grad_x_kff_multi(S = 1) on the same operands */
int cglb_time_grad_x_kff_pair(cglb_ctx* ctx, int reps, double* ms_avg);
/* Replace the training inputs (X: [n_total, d], host or device, the context's element type) and keep the targets.  Invalidates everything
 * cglb_set_data invalidates AND the hyper-parameters of both cglb_set_hypers and cglb_gpr_set_hypers: the scaled operand sets are made from X by
 * cglb_set_hypers, so an evaluation without a new push is CGLB_ERR_STATE instead of an evaluation on the old inputs.  Needs cglb_set_data first. */
int cglb_set_inputs(cglb_ctx* ctx, const void* X);

/* ---- inducing-point initialisation: InducingVariableConfig.init, config.py:55-65 ------------------------
 * The reference calls robustgp.ConditionalVariance(sample=False) (third-party): greedy maximisation of the conditional
 * variance under the INITIAL kernel (pivoted Cholesky of K_ff, lowest index on ties).  Needs set_data only; works on all n rows
 * whatever the row range of the context, so every rank of a sharded run obtains the same answer.  `lengthscales` host [d];
 * indices_out: host [min(m, n)] row indices in selection order; Z_out: dev [m, d] or NULL: rows 0 .. min(m, n) - 1 receive X[indices], with
 * m > n the rows from n on are left as they were; trace_out: host, sum of the remaining conditional variances,
 * tr(K_ff - Q_ff) (+ n * jitter), or NULL.  Invalidates set_hypers (the scaled
 * operand buffers are used as scratch).  Blocking. */
int cglb_select_inducing(cglb_ctx* ctx, const double* lengthscales, double variance, double jitter, int64_t* indices_out, void* Z_out,
                         double* trace_out);

/* ---- introspection / measurement ------------------------------------------------------------------ */
/* Copy common-term matrices out (tests): which = 0:A [m,n_local] 1:L [m,m] lower 2:LB [m,m] lower; 3: the stored alpha [n_total] of the
 * iterative exact-GP class (fp64; CGLB_ERR_STATE without one); dst: any. */
int cglb_get_matrix(cglb_ctx* ctx, int which, void* dst);
/* Average duration (ms, HIP events on the ctx stream) of `reps` back-to-back launches of one kernel family:
 * which = 0: K_ff mat-vec (pair kernel + slab combine), 1: preconditioner apply, 2: gradient bilinear pass,
 * 3: the pair kernel of the mat-vec alone (the dominant kernel), 4: the same for this rank's cyclic share (cglb_set_parallel),
 * 5: K_uu + jitter I and its Cholesky factorisation (invalidates the common terms: call cglb_setup again afterwards). */
int cglb_time_kernel(cglb_ctx* ctx, int which, int reps, double* ms_avg);
/* In-situ measurement of the dominant kernel: after cglb_set_option(ctx, "k1_profile", 1) every launch of the symmetric pair
 * kernel (in mat-vecs, solves and evaluations alike) is bracketed by HIP events on the context stream; "k1_ms_total" and
 * "k1_launches" return the accumulated device time and launch count since then (the call synchronises with the pending launches).
 * "k1_pairs_per_launch": kernel pairs one launch of that kernel evaluates with the current geometry (~N(N+256)/2 on one GPU: the
 * symmetric form visits each unordered pair once) - the unit count of the roofline; "kpart_bytes": size of the partial-sum slabs;
 * "matmat_native": 1 if a product of two or more columns (cglb_matmat, the batched solves) on this context in its current state - data, dtype,
 * hyper-parameters, "wide_reg", "kff_variant", ranks - runs through a shared-kernel instance, 0 if it falls back to single mat-vecs;
 * "grad_multi_native": 1 if a group of two or more vector pairs of the multi-pair gradient pass (cglb_grad_kff_multi, the gradient of
 * cglb_itergp_objective_and_grad) on this context in its current state - dtype, width, "wide_reg", "grad_multi_mid", ranks, shard - runs in ONE
 * pass over the kernel values (fp64 on one rank and one shard covering all rows, up to 32 dimensions and, register-resident, 33 ... 96), 0 if
 * it runs one single pass per pair and takes the kappa sums from one product;
 * "input_grad_native": 1 if the next input-gradient call on this context in its current state - dtype, width, "wide_reg", "input_grad_mid" - runs a
 * register-resident instance (fp64 up to 32 dimensions; 33 ... 96 under "input_grad_mid"), 0 if it is refused;
 * "predict_grad_native": 1 if the next cglb_predict_grad on this context in its current state - dtype, ranks, target columns, width, "wide_reg",
 * "input_grad_mid" - runs (fp64, one rank, one target column, up to 32 dimensions; 33 ... 96 under "input_grad_mid"), 0 if it is refused;
 * "train_input_grad_native": 1 if the next training-input gradient (cglb_grad_x_kff_multi, cglb_itergp_objective_and_grad_x,
 * cglb_gpr_objective_and_grad_x) on this context in its current state - dtype, width, ranks, shard, target columns - runs, 0 if it is refused;
 * "bound_input_grad_native": 1 if the next cglb_objective_and_grad_x with gx_out on this context in its current state - dtype, width, ranks,
 * shard, target columns, "logdet_bound", "precond_mode" - runs, 0 if it is refused;
 * "exp_clamp" | "m32_bias": the exponent-range regime the last cglb_set_hypers chose from the data's per-column range and the lengthscales
 * (CGLB_ERR_STATE before one) - 1 if the pair kernels run their range-clamped instances (kernel values below 2^-1000 come out as that floor,
 * not 0), 0 for the unclamped ones | the positivity bias of the Matern squared distance in hot units^2 (0 for RBF; above 2e-8 the clamped
 * instances run and the bias is not applied).  Read-only; for tests that must show which instance a configuration ran;
 * after cglb_set_option(ctx, "eval_profile", 1): "eval_setup_ms" | "eval_pcg_ms" | "eval_final_ms" | "eval_grad_ms" = device time (HIP events on
 * the context stream) accumulated over the phases of every cglb_objective_and_grad / cglb_dist_objective_and_grad /
 * cglb_objective_and_grad_multi since - common terms | PCG | final mat-vec, preconditioner and bound scalars | gradient - and "eval_count" =
 * the number of evaluations.  With p > 1 columns the third phase is K v alone and the fourth holds the column-by-column rest (preconditioner,
 * bound scalars and gradient of each column in turn);
 * "comm_allreduce_calls" | "comm_allgather_calls": collectives issued by the library since cglb_comm_init_*;
 * "L_diag_ratio": max/min of diag(chol(K_uu + jitter I)) of the last cglb_setup (a cheap proxy of cond(L));
 * "gpr_bytes": device bytes the exact GPR class holds; "gpr_fill_ms" | "gpr_factor_ms" | "gpr_solve_ms" | "gpr_inverse_ms" | "gpr_grad_ms": device
 * time (HIP events on the context stream) of the phases of the last cglb_gpr_objective_and_grad - tiles of K | factorisation | alpha and the
 * scalars | K^-1 | gradient pass; 0 for a phase that evaluation did not run;
 * "itergp_select_ms" | "itergp_solve_ms" | "itergp_grad_ms": device time of the phases of the last cglb_itergp_objective_and_grad - pivots and
 * common terms | right-hand sides and the batched solve | gradient; 0 for a phase that evaluation did not run;
 * "itergp_cache_ms" | "itergp_var_ms": device time of the last cglb_itergp_var_cache | of the variance part (product and row norms) of the last
 * cglb_itergp_predict_cached; "itergp_cache_request": the rank the valid variance cache was asked for, 0 without a valid cache;
 * "feature_ms": device time of the last feature product (kernel and slab sums of every group) of cglb_feature_matmat or cglb_itergp_sample. */
int cglb_get_stat(cglb_ctx* ctx, const char* name, double* value);
/* Tunables: name = "kff_variant" | "kff_jsplit" | "kuf_msplit" (chunks over the inducing points of cglb_grad_x_kuf, 0: the rule) | "kff_rows" | "sym_chunk" | "precond_mode" | "chol_mode" | "pcg_lookahead" | "sym_order" | "aat_block" | "grad_gram" | "k1_profile" |
 * "grad_trsm" (gradient algebra against L = chol(K_uu): 0 products with the explicit inverse, 1 backward-stable triangular solves, 2 = default:
 *  the products followed by one step of iterative refinement against L - the accuracy of the solves for about two thirds of their time) |
 * "precision" (the EVALUATOR of a kernel value - 2^x, square root, polynomial factor - given the squared distance it is handed: 1, default:
 *  <= 1e-13 relative - degree-3 table polynomial, one-step square root; 0: ~3e-16; 2: opt-in, degree-2 polynomial, ~1e-10 - inside the 1e-6
 *  the bound needs, one instruction per pair cheaper.  This is not the whole error of a kernel value: every N^2 product forms the squared
 *  distance in Gram form, |x_i|^2 + |x_j|^2 - 2 x_i.x_j on the centred, scaled inputs, whose rounding error is ABSOLUTE in the exponent -
 *  up to (5 d + 3) 2^-53 max(|x_i|^2, |x_j|^2) (csrc/devmath.h).  With R the exponent range of the data in octaves (RBF: 2 sum_k (range_k /
 *  l_k)^2 log2 e, range_k the largest deviation of column k from its mean) a kernel value moves by up to (ln2 / 4) (5 d + 3) 2^-53 R of
 *  itself (RBF; the Matern kinds: (ln2)^2 / 2 (5 d + 3) 2^-53 sum_k (sqrt(2 nu) range_k / l_k)^2 log2e^2 of the variance), at every level:
 *  3e-12 at d = 32 and R = 931, the widest range the unclamped kernels take (measured 2.2e-13), 9e-12 at d = 77 and R = 1200 (measured
 *  1.4e-12), below 1e-14 where R (5 d + 3) < 500.  Pairs near the centre of the data see their own, smaller norms.  The unclamped Matern
 *  instances of levels 1 and 2 add the positivity bias, at most 3e-13 of the variance on a coincident pair.  The direct-difference passes
 *  (cglb_select_inducing, K_uu and K_uf of inputs up to 32 dimensions, cglb_grad_kff_multi up to 32 dimensions) have no such term.
 *  tests/kernel_value_cases.py derives the bound of one value term by term; tests/test_gpu_kernel_values.py holds every fp64 product to it) ...;
 * "pcg_lookahead" (0: the host waits for the stop statistic before enqueuing anything; 1, default: the next mat-vec is enqueued first while
 *  1/2 r^T P r of the previous iteration exceeds 32 x max_error; k >= 2: that factor - a mis-speculated mat-vec is wasted work, never a wrong result) |
 * "final_matvec" (cglb_objective_and_grad after a solve: 1 recomputes K v with a mat-vec like models.py:280; 0, the default, takes K v = e - r
 *  from the residual r the PCG recurrence carries - exact at the start of a solve and after every restart step; measured difference at the
 *  headline shape: bound <= 3e-15 relative, gradient <= 1e-10 of its largest entry, one N^2 pass saved per evaluation; fp32 keeps the
 *  same default: after 56 / 67 steps with a restart (tests/test_gpu_fp32_parity.py) the bound from the recurrence residual was 1.4e-3 /
 *  1.8e-3 from the fp64 oracle at the same v, against 3.1e-3 / 1.4e-3 recomputed) |
 * "wide_grad_sym" (tiled K_ff gradient pass of wide inputs: 1, default - tiles on and right of the diagonal only; 0 - every tile) |
 * "wide_reg" (inputs of 33 ... 96 dimensions, fp64: 1, default - the symmetric K_ff mat-vec and the K_ff gradient pass stay register-resident,
 *  column operands handed out by v_fmac_f64 row_newbcast; 0 - both go through the Gram tiles like every other product of a wide input) |
 * "grad_multi_mid" (inputs of 33 ... 96 dimensions, fp64, "wide_reg" 1: 1, default - the multi-pair gradient pass evaluates every kernel value
 *  once per group of up to 8 vector pairs; 0 - one single pass per pair and one product for the kappa sums, what every other wide context runs;
 *  for A/B timing and tests; a single pair takes the single pass either way) |
 * "input_grad_mid" (inputs of 33 ... 96 dimensions, fp64, "wide_reg" 1: 0, default - every input-gradient entry refuses the context ("no wide path
 *  yet"); 1 - every input-gradient product runs at that width: the iterative class's two through csrc/kernels_input_grad_mid.hip, the row-weighted
 *  one of cglb_cross_grad_weighted, cglb_predict_grad and cglb_gpr_predict_grad through csrc/kernels_predict_grad_mid.hip; no effect on any other
 *  width or entry) |
 * "drop_weighted_operand" (any value: forget the pre-weighted copy cglb_vec_update_p_seg made of its p - for callers that modify p before the next mat-vec) |
 * "logdet_bound" (the log-det term of the bound; cglb_logdet, cglb_objective_and_grad and its gradient follow it.  e = y - mu, s = noise,
 *  f = variance, A = L^-1 K_uf / sqrt(s), B = I + A A^T = LB LB^T, C = LB^-1 A, t = N f / s - tr A A^T:
 *  0, default - Jensen (cglb, models.py:215-244): -sum log diag LB - N/2 log s - N/2 log(1 + t/N);
 *  1 - NM^2 (cglbnm2 and the SGPR bound, tensorflow/models.py:271-308, :353-413): -sum log diag LB - N/2 log s - t/2;
 *  2 - N^2M (cglbn2m, sgprn2m, tensorflow/models.py:311-350, :353-413): -sum log diag LB - N/2 log(tau/N), tau = tr(K_ff + s I) - tr(C (K_ff + s I) C^T),
 *  one N^2 M pass per setup and one more per gradient; fp64 contexts with the stored panel (precond_mode 0) only) |
 * "quad_term" (0, default - the CG quadratic term at the caller's v; 1 - the exact term 1/2 e^T (Q_ff + s I)^-1 e = |e|^2/(2s) - |LB^-1 A e|^2/(2s)
 *  of SGPR (tensorflow/models.py:393-402): cglb_objective_and_grad and cglb_predict treat v as 0 (v_inout is neither read nor written, no
 *  solve runs whatever run_cg says) and issue no N^2 work).  Both options at 0: every entry point behaves exactly as without them.  A
 *  non-zero value is refused on a context with more than one rank (cglb_set_parallel / cglb_comm_init_*), and both of those refuse a context
 *  that carries one;
 * "gpr_block" (outer block edge of the exact GPR class: its tiles of K, the block columns of its factorisation and the tiles of its gradient
 *  pass; a multiple of 64 in [64, 4096], default 2048; a changed value releases the buffers of that class);
 * returns CGLB_ERR_BAD_ARG if unknown. */
int cglb_set_option(cglb_ctx* ctx, const char* name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* CGLB_HIP_H */
