// Launch geometry of the symmetric pair kernels (kernels_kff_sym.hip, kernels_kff_multi.hip): the column-chunk rule and the order of the
// work list.  Pure integer host code without HIP types, so that a plain C++ program can include and test it (tests/host).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#define PAIR_CHUNK_MAX 1024  // a workgroup stages the column sums of one chunk in LDS: at most this many per wave

struct pair_unit { int x, y; };  // (group of four row blocks, column unit), (-1, -1) = padding; the layout of int2 (pair_common.h checks)

// A work list on the device with what it was built for; one per kernel, so that alternating launches of the two rebuild nothing.
struct pair_list {
    void* dev = nullptr;
    int64_t key[6] = {-1, 0, 0, 0, 0, 0};  // n, column unit, rows per block, world, rank, order
    int nwg = 0;                           // workgroups of a launch (padding included)
    bool holds(const int64_t (&k)[6]) const { return dev && std::equal(k, k + 6, key); }
};

// Columns per work item: 1024, halved down to 128 while a rank has fewer than 16k items (measured per-rank kernel at N = 100k: world 8:
// 0.48 ms at 128, 0.63 ms at 1024; world 4: 0.82 at 256, 0.86 at 512; large N keeps 1024 at any world size: fewer, larger slabs); the
// option "sym_chunk" (> 0, at most 2^20: cglb_set_option) overrides; rounded up to the batch of 16 columns and clamped to the LDS staging.
static inline int64_t pair_column_chunk(int64_t n, int rbrows, int world, int64_t sym_chunk_opt) {
    int64_t chunk = PAIR_CHUNK_MAX;
    const double nrb_rank = (double)((n + rbrows - 1) / rbrows) / world;
    while (chunk > 128 && nrb_rank * ((double)n / (double)chunk) * 0.5 < 16384.0) chunk /= 2;
    if (sym_chunk_opt > 0) chunk = sym_chunk_opt;
    chunk = (chunk + 15) / 16 * 16;
    return chunk > PAIR_CHUNK_MAX ? PAIR_CHUNK_MAX : chunk;
}

// Workgroup b -> (group g, unit k) for every g < ngroups and first_unit(g) <= k < nunits; first_unit(g) is the unit that holds the first
// row of the group's first block.  Never empty: an empty problem gives one padding entry.
//   order 0: group major, longest rows first (group 0 sweeps the most columns).
//   order 1: XCD-aware.  Workgroups go round-robin to the 8 XCDs (workgroup b -> XCD b % 8), each with its own 4-MB L2, and the streamed
//            side of a workgroup is its column unit (chunk * (DP + 2) operands, 80 KB at 1024 columns).  The list sorted by unit is cut into
//            8 contiguous ranges of equal length, one per XCD: an XCD then only ever streams its own ~1/8 of the columns (L2-resident)
//            instead of every XCD sweeping all of X through the Infinity Cache.  Inside a range (a dozen units, ~1 MB of operands) the
//            entries go group by group, so that the row operands of a group are fetched once per XCD rather than once per workgroup.
//            Entry q of range x is workgroup 8 q + x; the ranges are padded to equal length.
template <typename F>
static std::vector<pair_unit> pair_work_order(int ngroups, int nunits, F first_unit, int order) {
    std::vector<pair_unit> list;
    if (order == 0) {
        for (int g = 0; g < ngroups; ++g)
            for (int k = first_unit(g); k < nunits; ++k) list.push_back({g, k});
    } else {
        std::vector<pair_unit> sorted;
        for (int k = 0; k < nunits; ++k)
            for (int g = 0; g < ngroups; ++g)
                if (first_unit(g) <= k) sorted.push_back({g, k});
        const size_t T = sorted.size(), XCDS = 8, per_xcd = (T + XCDS - 1) / XCDS;
        list.assign(per_xcd * XCDS, {-1, -1});
        for (size_t x = 0; x < XCDS; ++x) {
            const size_t lo = std::min(x * per_xcd, T), hi = std::min((x + 1) * per_xcd, T);
            std::stable_sort(sorted.begin() + lo, sorted.begin() + hi, [](const pair_unit& a, const pair_unit& b) { return a.x < b.x; });
            for (size_t q = lo; q < hi; ++q) list[(q - lo) * XCDS + x] = sorted[q];
        }
    }
    if (list.empty()) list.push_back({-1, -1});  // keeps the device allocation non-empty
    return list;
}

// Group width of the multi-column K_ff product (kernels_kff_multi.hip, kernels_kff_multi_mid.hip): a product of s columns is cut into groups
// of at most `group` columns, each padded to S_pad = 2, 4 or 8 right-hand sides, and a single left-over column goes through the mat-vec.
//   narrow widths (Dp <= 32): groups of 8.
//   mid widths (hot width Dh = 48, 64, 80, 96; one row per lane, the row operand alone fills 2 Dh VGPRs): the widest S_pad whose
//   instances compile without a spill (DESIGN.md section 4b has the registers of every instance); 0 = no instance, the product falls
//   back to single mat-vecs.  Every width holds 8: up to 80 inside the 256 VGPRs of two waves per SIMD (at 64 with S_pad 8, and at 80,
//   with 8 instead of 16 per-lane partials), at 96 as one wave per SIMD with 14 - 42 values in the accumulation registers.
#define MULTI_GROUP_NARROW 8
static constexpr int multi_mid_group(int dh) { return (dh == 48 || dh == 64 || dh == 80 || dh == 96) ? 8 : 0; }
// per-lane partial column sums of a batch at a mid width (16 as in the narrow kernel, 8 where 16 do not fit); 0 = not instantiated
static constexpr int multi_mid_partials(int dh, int sp) {
    if (sp < 2 || sp > multi_mid_group(dh) || (sp & (sp - 1)) != 0) return 0;
    return (dh <= 48 || (dh <= 64 && sp <= 4)) ? 16 : 8;
}
static constexpr int multi_group_pad(int sg) { return sg <= 2 ? 2 : (sg <= 4 ? 4 : 8); }  // S_pad of a group of sg columns
// columns of the next group when `left` columns remain and groups hold at most `group` (>= 2): 1 = the single left-over column
static constexpr int multi_next_group(int left, int group) { return left < group ? left : group; }

// Group rule of the mid-width multi-pair gradient pass (kernels_grad_multi_mid.hip): S pairs are cut into groups of at most `group` pairs in
// order (multi_next_group), each group of two or more padded to S_pad = 4 or 8 (the column operands of a group fill half a 16-lane row; the
// padding pairs cost S_pad - sg of the ~DP + 30 lane-instructions of a pair), and a single left-over pair goes through the single pass.  Every hot
// width holds 8 inside the 256 VGPRs of two waves per SIMD (DESIGN.md section 4d has the registers of every instance); 0 = no instance.
static constexpr int grad_multi_mid_group(int dh) { return (dh == 48 || dh == 64 || dh == 80 || dh == 96) ? 8 : 0; }
static constexpr int grad_multi_mid_pad(int sg) { return sg <= 4 ? 4 : 8; }
