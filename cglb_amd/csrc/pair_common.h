// Pieces shared by the N^2 pair kernels: the symmetric mat-vec (kernels_kff_sym.hip), the multi-column product (kernels_kff_multi.hip) and
// the Gram-form gradient passes (kernels_grad.hip, kernels_grad_mid.hip).  Launch geometry (host only): pair_worklist.h.  A kernel whose
// register allocation or schedule moves when it calls wave_colsum8 or pair_row_seed keeps that piece written out and says so at the place.
#pragma once
#include <cstddef>

#include "devmath.h"
#include "dispatch.h"
#include "pair_worklist.h"

static_assert(sizeof(pair_unit) == sizeof(int2) && offsetof(pair_unit, y) == offsetof(int2, y), "the kernels read the work lists as int2");

// Folded column norm (RBF, unclamped exponent range): kappa_ij = 2^(a_i + x_i.x_j) w_j, the add of a_j per pair dropped.  The mat-vec
// kernels fold for every T; the gradient kernels narrow this to fp64 at the use site.
template <int KIND, bool CLAMP>
constexpr bool pair_fold() { return KIND == CGLB_RBF && !CLAMP; }
// Any Matern kind (3/2 and 5/2 share the root and its bias), fast levels, unclamped range, fp64: squared distances kept positive by a bias in the row seeds instead of a clamp per pair
// (devmath.h CGLB_M32_BIAS_*)
template <typename T, int KIND, bool CLAMP, int PREC>
constexpr bool pair_biased() { return cglb_kind_matern<KIND>() && !CLAMP && PREC != CGLB_PREC_EXACT && sizeof(T) == 8; }
// seed of a row's Gram chain from its norm term a: RBF the exponent's a_i, any Matern kind the -|x_i|^2 / 2 of -2 (x_i.x_j - |x_i|^2 / 2) + a_j
template <typename T, int KIND, bool BIASED>
__device__ __forceinline__ T pair_row_seed(T a, T bias) {
    static_assert(cglb_kind_known<KIND>(), "unknown kernel kind");
    return (KIND == CGLB_RBF) ? a : (BIASED ? T(-0.5) * (a + bias) : T(-0.5) * a);
}

#define MULTI_CS_MAX 1024  // multi-column product (kernels_kff_multi.hip, kernels_kff_multi_mid.hip): column sums a wave stages in LDS (columns of a chunk x S_pad)
#define PAIR_TR_LD 65  // leading dimension of a wave's 8 x 64 transposition scratch (odd: the column reads spread over the banks)
// Sums ACROSS the 64 lanes of the 8 per-lane partials t8[0..7] (8 columns of a batch); every lane returns the sum of column lane & 7.
// Transposed through LDS: every lane writes its 8 partials (row jj of `tr`, stride PAIR_TR_LD: conflict-free), then lane (c = lane & 7,
// g = lane >> 3) adds the 8 lanes 8g..8g+7 of column c in fixed order and three xor-shuffles add the 8 groups: 7 + 3 adds and no selects
// per 32 pairs, against 83 VALU instructions per 64 pairs for the in-register form (kernels_kff_sym.hip).  One wave, in-order LDS: no
// barrier; the wave_barrier calls only pin the compiler's order.  `tr`: this wave's 8 * PAIR_TR_LD elements.
template <typename T>
__device__ __forceinline__ T wave_colsum8(const T* t8, T* tr, int lane) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) tr[jj * PAIR_TR_LD + lane] = t8[jj];
    __builtin_amdgcn_wave_barrier();
    const T* __restrict__ src = tr + (lane & 7) * PAIR_TR_LD + (lane & ~7);
    T v = src[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) v += src[i];
    __builtin_amdgcn_wave_barrier();
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Partial-sum slabs of `need` bytes in (*slabs, *cap).  They grow as N^2 / 256 elements per rank: when they do not fit the free device memory
// (the old slabs count as free) say so instead of failing inside hipMalloc.
static int pair_reserve_slabs(cglb_ctx* c, void** slabs, size_t* cap, size_t need, const char* what, const char* detail, const char* advice) {
    if (need > *cap) {
        HIP_CHECK(c, c->mem.drop(slabs, cap));
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(c, hipMemGetInfo(&free_b, &total_b));
        if (need > free_b)
            return cglb_fail(c, CGLB_ERR_HIP, std::string(what) + " needs " + std::to_string(need >> 20) + " MiB of partial-sum slabs" + detail + " but only " +
                                                  std::to_string(free_b >> 20) + " MiB of device memory are free: " + advice);
    }
    return c->mem.reserve(c, slabs, cap, need);
}

// Replaces the device list of `l` by `head` followed by `order` (one allocation) and records what it was built for.
static int pair_list_store(cglb_ctx* c, pair_list* l, const int64_t (&key)[6], const std::vector<pair_unit>& head, const std::vector<pair_unit>& order) {
    HIP_CHECK(c, c->mem.drop(&l->dev));  // the list is replaced, at its new size
    CGLB_TRY(c->mem.alloc(c, &l->dev, (head.size() + order.size()) * sizeof(pair_unit)));
    if (!head.empty()) HIP_CHECK(c, hipMemcpyAsync(l->dev, head.data(), head.size() * sizeof(pair_unit), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(c, hipMemcpyAsync((pair_unit*)l->dev + head.size(), order.data(), order.size() * sizeof(pair_unit), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    std::copy(key, key + 6, l->key);
    l->nwg = order[0].x < 0 ? 0 : (int)order.size();  // an empty problem launches nothing
    return CGLB_OK;
}
