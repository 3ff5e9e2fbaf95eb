// wide_products.h — schedule constants and launchers of the row-major feature products' kernels (wide_products.hip), called by hsw_api.cpp.
#ifndef HISPARSE_WIDE_PRODUCTS_H_
#define HISPARSE_WIDE_PRODUCTS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace hisparse {
namespace dev {

// Launch geometry (as row_softmax.h): workgroups of kWideThreads lanes, the grid never exceeds compute_units * kWideBlocksPerCu of them and
// strides over the schedule's virtual workgroups from there.  A feature row of d words is covered by a GROUP of lanes, one 16-byte chunk
// per lane: the smallest power of two that holds ceil(d / 4), at most 64 (d <= kWideMaxD).  A TEAM of one or more groups works on one row,
// its groups on different entries; the team of a row is set by the row's length class and by d.  kWideInFlight entries are gathered per
// group and trip of its loop.  hisparse_amd/wide.py restates the numbers (tests assert that a pattern is larger than two trips of the
// grid from them).
constexpr uint32_t kWideThreads = 256;
constexpr uint32_t kWideBlocksPerCu = 8;
constexpr uint32_t kWideInFlight = 4;
constexpr uint32_t kWideLong = 512;
constexpr uint32_t kWideMaxD = 256;

// Classes by row length n (rows of a transposed pattern: column lengths).  0 holds the long rows, n > kWideLong: the whole workgroup on
// one row.  Classes 1 ... 3 want 4, 16 and 64 groups per row (n <= 4, n <= 16, the rest; an EMPTY row is of class 1: its team writes
// the zeros); a team never exceeds a wavefront, so it is min(64, wanted groups * lanes per group) lanes.  Virtual workgroups are laid
// out in class order: the long rows are started first and the short ones fill in beside them.
constexpr uint32_t kWideClasses = 4;
inline uint32_t wide_class_of(uint32_t n) { return n > kWideLong ? 0u : n <= 4u ? 1u : n <= 16u ? 2u : 3u; }
// lanes per feature row of d words (1 <= d <= kWideMaxD)
inline uint32_t wide_group_lanes(uint32_t d) {
    uint32_t g = 1;
    while (g * 4u < d) g *= 2u;
    return g;
}
// lanes of the team that works on one row of class c with groups of `group` lanes
inline uint32_t wide_team_lanes(uint32_t c, uint32_t group) {
    if (c == 0) return kWideThreads;
    const uint32_t want = (1u << (2u * c)) * group;
    return want < 64u ? want : 64u;
}

// What a launch needs of a schedule, by value: first[c] = the first virtual workgroup of class c, first[kWideClasses] = all of them
// (these depend on d: wide_table); off[c] = where class c starts in the row list, off[kWideClasses] = the length of the list (every row).
struct WideTable {
    uint32_t first[kWideClasses + 1];
    uint32_t off[kWideClasses + 1];
};
// count[c] = the rows of class c
inline WideTable wide_table(const uint32_t (&count)[kWideClasses], uint32_t d) {
    WideTable t;
    t.first[0] = t.off[0] = 0;
    const uint32_t group = wide_group_lanes(d);
    for (uint32_t c = 0; c < kWideClasses; ++c) {
        const uint32_t per = kWideThreads / wide_team_lanes(c, group);
        t.first[c + 1] = t.first[c] + (count[c] + per - 1) / per;
        t.off[c + 1] = t.off[c] + count[c];
    }
    return t;
}

// One side of a pattern on the device: the CSR arrays themselves, or (transposed) column pointers, the row of every entry in column
// order and the CSR index of every such entry.
struct WideSide {
    const uint32_t* ptr = nullptr;         // rows + 1 words
    const uint32_t* idx = nullptr;         // per entry: the index of the gathered operand's row
    const uint32_t* perm = nullptr;        // per entry: where its value sits in the caller's array; nullptr = the entry's own index
    const uint32_t* list = nullptr;        // every row, class by class
    uint32_t count[kWideClasses] = {};     // rows per class
    uint64_t entries = 0;
    uint32_t compute_units = 0;
};

// out[e] = sum_j U[row(e)][j] * V[idx[e]][j]; nothing to do for a pattern without entries
hipError_t launch_wide_dot(const WideSide& s, const float* u, uint64_t ldu, const float* v, uint64_t ldv, uint32_t d, float* out, hipStream_t stream);
// Y[r][j] = sum_{e in row r} w[perm ? perm[e] : e] * X[idx[e]][j]; rows without entries are written as zeros
hipError_t launch_wide_gather(const WideSide& s, const float* w, const float* x, uint64_t ldx, uint32_t d, float* y, uint64_t ldy, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_WIDE_PRODUCTS_H_
