// What a model class with a translation unit of its own (api_itergp.hip) uses of the core in cglb_api.hip: the scalar slots, the preconditioner,
// the one PCG loop with the operators of its one-column and s-column callers, and the helpers of the timing entries.
#pragma once
#include "devmath.h"
#include "dispatch.h"

// scalar slots in ctx->scal
enum { S_RZ = 0, S_PAP = 1, S_NRZ = 2, S_TRACE = 3, S_SUMLOG = 4, S_TRBINV = 5, S_TMP = 6, S_SC = 8, S_TMP2 = 16, S_LDIAG = 56 };

inline int grid1d_full(int64_t n) { return (int)((n + 255) / 256); }  // one thread per element, no stride loop

int read_scalars(cglb_ctx* c, const double* dev, double* host, int n);   // blocking read of n device scalars
int precond_single(cglb_ctx* c, const void* r, void* z, double* rz_slot);  // z = P r, rz = r.z on one shard
int require_multi_ok(cglb_ctx* c);

// ---- PCG (conjugate_gradient.py:41-86) ----------------------------------------------------------------------
// What the one loop (pcg_solve) is told about its caller: where the recurrence keeps its vectors and scalars, how many columns it advances and
// how the two operators are applied.
//   fused (one GPU, one shard): the context's own work vectors; p.Ap comes out of the mat-vec's slab combine; z = P r in one piece
//   N ranks: replicated full-length vectors of the communicator state; cyclic share + all-reduce, then a dot over the summed product
//            (another summation order than the fused one, on purpose); z gathered in segments
//   s columns (multi-output targets): s independent recurrences, each with its own gamma_b and beta_b, in lockstep over one mat-mat
//            product per iteration (kernels_kff_multi.hip); vectors [s][n], column b contiguous
struct pcg_ops {
    void *r, *z, *p, *Ap, *Kv;  // [s][n]; z is the direction's scratch (unused on N ranks, which gather z in segments)
    int64_t n;
    int s;                      // columns
    double *rz, *nrz, *pap;     // [s] device scalars; rz and nrz swap roles every iteration
    double* host;               // [s] pinned host mirror of the stop-test scalars
    int (*matvec)(cglb_ctx* c, const pcg_ops& o, const void* x, void* out, double* pdot_slot);  // out_b = (K_ff + noise I) x_b; x.out into pdot_slot if it fuses the dot
    bool dot_fused;         // false: pdot_slot is ignored and a launch_dot follows the mat-vec
    int (*direction)(cglb_ctx* c, const pcg_ops& o, double* rz_new, const double* rz_old, int restart);  // z = P r, rz_new = r.z, p = z (+ p rz_new / rz_old)
    bool rz_must_be_finite; // N ranks leave the loop together or not at all: a non-finite r^T P r is CGLB_ERR_COMM, not a quiet end
    pcg_log* log = nullptr; // optional: receives rz_b before every iteration and after the last, and p_b.Ap_b of every iteration (host_pap: [s] pinned)
};
pcg_ops fused_ops(cglb_ctx* c);
int pcg_solve(cglb_ctx* c, const pcg_ops& o, const void* b, void* v, double max_error, int max_iter, int restart_iter, int* steps, double* half_rz,
              double* half_rz_cols = nullptr);

// Column b of every [P][N] array is a contiguous vector; pcg_solve advances the P recurrences through multi_ops.
struct multi_work {
    char *r, *z, *p, *Ap, *Kv, *b;      // [s][N]
    double *rz, *nrz, *pap;             // [s] device scalars
};
int multi_reserve(cglb_ctx* c, int s, multi_work* w);
pcg_ops multi_ops(cglb_ctx* c, const multi_work& w, int s);  // pcg_solve on s columns in the buffers of multi_reserve(c, s, &w)

// out[m * ld + n] = var * kappa(z_m, x_n) for any two sets in plain scaled units (the context's element type): Zs [M][Dp], Xs [n][Dp]
int launch_kpanel(cglb_ctx* c, const void* Zs, int M, const void* Xs, int64_t n, int64_t ld, void* out);
// dst [s][N] <- s copies of y: the operands of a timed launch (values do not change the instruction stream)
int fill_y_columns(cglb_ctx* c, void* dst, int s);
// the statistics of the iterative exact-GP class (api_itergp.hip); -1: not one of its names
int itergp_stat(cglb_ctx* c, const char* name, double* value);

// ms_avg = average time of `once` on the context stream over reps calls, after one warm-up call (which also sizes the work buffers)
template <typename F>
int time_repeated(cglb_ctx* c, int reps, F once, double* ms_avg) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_CHECK(c, hipEventCreate(&e0));
    {
        const hipError_t e = hipEventCreate(&e1);
        if (e != hipSuccess) { (void)hipEventDestroy(e0); return cglb_fail(c, CGLB_ERR_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    }
    int rc = once();
    if (rc == CGLB_OK) {
        (void)hipEventRecord(e0, c->stream);
        for (int i = 0; i < reps && rc == CGLB_OK; ++i) rc = once();
        (void)hipEventRecord(e1, c->stream);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_avg = (double)ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}
