// neighbor_aggregate.hip — the neighbour aggregation of include/hisparse_aggregate.h over a CSR pattern, with ROW-MAJOR features
// ([index][feature], d <= 256).  Two kernel templates and ONE launch per call:
//   neighbor_forward_kernel    ysum[r][j] = sum (mean) of X[col(e)][j] over row r, ymax / ymin its extremes, amax / amin the CSR index of
//                              the winner                                                                     (hsagg_forward_device)
//   neighbor_backward_kernel   gx[c][j] = sum over column c's entries k, r = row(k), of w_r gsum[r][j] + [amax[r][j] == e_k] gmax[r][j]
//                              + [amin[r][j] == e_k] gmin[r][j], over the transposed pattern                  (hsagg_backward_device)
// Both run on the unchanged schedule of wide_products.h through wide_lanes.h (pick, trips_of, grid_of): a lane owns one 16-byte chunk of a
// feature row, the groups of a team take different entries, kWideInFlight per group and trip, and the trip's gathers are all issued before
// the first use.  ONE gather of X's chunk per entry serves every aggregator of the launch.  A lane keeps four double sums and, per
// extreme, four (value, index) pairs (Best4); a team's groups merge by lane shuffles (merge_lanes, merge_best_lanes), a long row's four
// wavefronts through LDS (merge_waves, merge_best_waves): 8 KiB per sum or extreme that the instantiation carries, none for the others.
// The pairs merge by the header's winner rule itself (outranks: NaN first, then the IEEE comparison, then the smaller index), a total
// order, so the winner does not depend on how the entries were dealt; a value word is carried as loaded and stored as loaded.
// The aggregators are template arguments (sum / max / min wanted or not, seven instantiations per kernel); mean against sum and the
// arg arrays taken or NULL are wave-uniform branches.  Every output word has one writer: no atomics, no scratch, no matrix engine, no
// inline assembly.  Arithmetic: the header's ARITHMETIC block -- doubles in registers, the mean's and the backward's ONE double division,
// one rounding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "neighbor_aggregate.h"
#include "wide_lanes.h"
#include "wide_products.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kNone = 0xFFFFFFFFu;      // HSAGG_NONE: larger than every entry's index

// this lane's 16 bytes of a feature row
struct Chunk {
    uint32_t at, words;      // the first word, and how many of the four are inside d (0 for a dead lane)
    bool live;
};

__device__ __forceinline__ Chunk chunk_of(uint32_t group, uint32_t d) {
    const uint32_t chunk = threadIdx.x & (group - 1u);
    Chunk c;
    c.live = chunk * 4u < d;
    c.at = c.live ? chunk * 4u : 0u;
    c.words = c.live ? min(d - c.at, 4u) : 0u;
    return c;
}

// the first `words` (1 ... 4) of a chunk: one 16-byte store, or narrower ones for the last chunk of a row with d % 4 != 0
template <typename T>
__device__ __forceinline__ void store_words(T* dst, T a, T b, T c, T d, uint32_t words) {
    typedef T T4 __attribute__((ext_vector_type(4)));
    if (words >= 4u) {
        T4 v = {a, b, c, d};
        *reinterpret_cast<T4*>(dst) = v;
    } else {
        dst[0] = a;
        if (words >= 2u) dst[1] = b;
        if (words >= 3u) dst[2] = c;
    }
}

__device__ __forceinline__ Best4 nothing_yet(float v) { return Best4{{v, v, v, v}, {kNone, kNone, kNone, kNone}}; }

template <bool kMax>
__device__ __forceinline__ void offer4(Best4& b, f32x4 x, uint32_t e) {
    offer<kMax>(b, 0, x.x, e);
    offer<kMax>(b, 1, x.y, e);
    offer<kMax>(b, 2, x.z, e);
    offer<kMax>(b, 3, x.w, e);
}

// an extreme of a row: the winners' words as they were loaded, +0.0f where no entry was offered (a row without entries), and their indices
__device__ __forceinline__ void store_best(const Best4& b, float* __restrict__ y, uint32_t* __restrict__ arg, uint64_t off, uint32_t words) {
    store_words<float>(y + off, b.e[0] == kNone ? 0.0f : b.v[0], b.e[1] == kNone ? 0.0f : b.v[1], b.e[2] == kNone ? 0.0f : b.v[2], b.e[3] == kNone ? 0.0f : b.v[3], words);
    if (arg) store_words<uint32_t>(arg + off, b.e[0], b.e[1], b.e[2], b.e[3], words);
}

template <bool kSum, bool kMax, bool kMin>
__global__ __launch_bounds__(kWideThreads) void neighbor_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, WideTable tab,
                                                                       const float* __restrict__ x, uint64_t ldx, uint32_t d, uint32_t group, uint32_t mean,
                                                                       float* __restrict__ ysum, float* __restrict__ ymax, uint32_t* __restrict__ amax, float* __restrict__ ymin,
                                                                       uint32_t* __restrict__ amin, uint64_t ldy) {
    const Chunk ck = chunk_of(group, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ x_chunk = x + ck.at;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        Best4 top = nothing_yet(-INFINITY), bottom = nothing_yet(INFINITY);
        // the row's entries lo + g, lo + g + groups, ...: an entry past the end gathers row 0 of X (in bounds, in the cache) and is not used
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t col[kWideInFlight];
            f32x4 xv[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) xv[i] = *reinterpret_cast<const f32x4*>(x_chunk + uint64_t(col[i]) * ldx);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    const uint32_t ei = uint32_t(e + uint64_t(i) * wk.groups);
                    if constexpr (kSum) {
                        acc[0] += static_cast<double>(xv[i].x);
                        acc[1] += static_cast<double>(xv[i].y);
                        acc[2] += static_cast<double>(xv[i].z);
                        acc[3] += static_cast<double>(xv[i].w);
                    }
                    // words past d of the row's last chunk are offered too and never stored: a NaN there reaches nothing
                    if constexpr (kMax) offer4<true>(top, xv[i], ei);
                    if constexpr (kMin) offer4<false>(bottom, xv[i], ei);
                }
            }
        }
        if constexpr (kSum) merge_lanes(acc, group, wk.team);
        if constexpr (kMax) merge_best_lanes<true>(top, group, wk.team);
        if constexpr (kMin) merge_best_lanes<false>(bottom, group, wk.team);
        bool stores = wk.mine && wk.g == 0 && ck.live;
        if (wk.c == 0) {      // a long row: the four wavefronts' partial results through LDS
            if constexpr (kSum) {
                __shared__ double red[kWaves][4][64];
                merge_waves(red, acc, lane, wave, group);
            }
            if constexpr (kMax) {
                __shared__ float top_v[kWaves][4][64];
                __shared__ uint32_t top_e[kWaves][4][64];
                merge_best_waves<true>(top_v, top_e, top, lane, wave, group);
            }
            if constexpr (kMin) {
                __shared__ float bottom_v[kWaves][4][64];
                __shared__ uint32_t bottom_e[kWaves][4][64];
                merge_best_waves<false>(bottom_v, bottom_e, bottom, lane, wave, group);
            }
            stores = wave == 0 && lane < group && ck.live;
        }
        if (stores) {
            const uint64_t off = uint64_t(wk.r) * ldy + ck.at;
            if constexpr (kSum) {
                const uint32_t n = wk.hi - wk.lo;
                if (mean && n) {      // a row without entries has summed nothing: +0.0
                    const double by = static_cast<double>(n);
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) acc[j] /= by;
                }
                store_words<float>(ysum + off, static_cast<float>(acc[0]), static_cast<float>(acc[1]), static_cast<float>(acc[2]), static_cast<float>(acc[3]), ck.words);
            }
            if constexpr (kMax) store_best(top, ymax, amax, off, ck.words);
            if constexpr (kMin) store_best(bottom, ymin, amin, off, ck.words);
        }
        if (wk.c == 0) __syncthreads();      // the LDS words are free for the workgroup's next long row
    }
}

// the terms of one entry's extreme: the gradient word where the row's arg word names this entry
__device__ __forceinline__ void add_where(double (&acc)[4], u32x4 arg, uint32_t e, f32x4 g) {
    if (arg.x == e) acc[0] += static_cast<double>(g.x);
    if (arg.y == e) acc[1] += static_cast<double>(g.y);
    if (arg.z == e) acc[2] += static_cast<double>(g.z);
    if (arg.w == e) acc[3] += static_cast<double>(g.w);
}

template <bool kSum, bool kMax, bool kMin>
__global__ __launch_bounds__(kWideThreads) void neighbor_backward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                                        const uint32_t* __restrict__ list, WideTable tab, const uint32_t* __restrict__ row_ptr,
                                                                        const float* __restrict__ gsum, const float* __restrict__ gmax, const uint32_t* __restrict__ amax,
                                                                        const float* __restrict__ gmin, const uint32_t* __restrict__ amin, uint64_t ldg, uint32_t d, uint32_t group,
                                                                        uint32_t mean, float* __restrict__ gx, uint64_t ldgx) {
    __shared__ double red[kWaves][4][64];
    const Chunk ck = chunk_of(group, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        // an entry past the end gathers the chunks of row 0 (in bounds, in the cache) and adds nothing
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t row[kWideInFlight], ek[kWideInFlight], n[kWideInFlight];
            f32x4 gs[kWideInFlight], gt[kWideInFlight], gb[kWideInFlight];
            u32x4 at[kWideInFlight], ab[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                row[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
                ek[i] = ok[i] ? __builtin_nontemporal_load(perm + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t off = uint64_t(row[i]) * ldg + ck.at;
                if constexpr (kSum) gs[i] = *reinterpret_cast<const f32x4*>(gsum + off);
                if constexpr (kMax) {
                    at[i] = *reinterpret_cast<const u32x4*>(amax + off);
                    gt[i] = *reinterpret_cast<const f32x4*>(gmax + off);
                }
                if constexpr (kMin) {
                    ab[i] = *reinterpret_cast<const u32x4*>(amin + off);
                    gb[i] = *reinterpret_cast<const f32x4*>(gmin + off);
                }
            }
            if constexpr (kSum) {
                if (mean) {
#pragma unroll
                    for (uint32_t i = 0; i < kWideInFlight; ++i) n[i] = row_ptr[row[i] + 1u] - row_ptr[row[i]];
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    if constexpr (kSum) {
                        if (mean) {      // the entry is one of row's n >= 1
                            const double by = static_cast<double>(n[i]);
                            acc[0] += static_cast<double>(gs[i].x) / by;
                            acc[1] += static_cast<double>(gs[i].y) / by;
                            acc[2] += static_cast<double>(gs[i].z) / by;
                            acc[3] += static_cast<double>(gs[i].w) / by;
                        } else {
                            acc[0] += static_cast<double>(gs[i].x);
                            acc[1] += static_cast<double>(gs[i].y);
                            acc[2] += static_cast<double>(gs[i].z);
                            acc[3] += static_cast<double>(gs[i].w);
                        }
                    }
                    // arg words are compared, never used as an address: one that names no entry of this column adds nothing
                    if constexpr (kMax) add_where(acc, at[i], ek[i], gt[i]);
                    if constexpr (kMin) add_where(acc, ab[i], ek[i], gb[i]);
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        float* dst = gx + uint64_t(wk.r) * ldgx + ck.at;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && ck.live)      // a column without entries has summed nothing: +0.0
                store_words<float>(dst, static_cast<float>(acc[0]), static_cast<float>(acc[1]), static_cast<float>(acc[2]), static_cast<float>(acc[3]), ck.words);
        } else {
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && ck.live)
                store_words<float>(dst, static_cast<float>(acc[0]), static_cast<float>(acc[1]), static_cast<float>(acc[2]), static_cast<float>(acc[3]), ck.words);
            __syncthreads();      // `red` is free for the workgroup's next long column
        }
    }
}

template <bool kSum, bool kMax, bool kMin>
void forward_of(const WideSide& s, const WideTable& t, bool mean, const float* x, uint64_t ldx, uint32_t d, float* ysum, float* ymax, uint32_t* amax, float* ymin, uint32_t* amin,
                uint64_t ldy, hipStream_t stream) {
    hipLaunchKernelGGL((neighbor_forward_kernel<kSum, kMax, kMin>), grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, x, ldx, d, wide_group_lanes(d),
                       mean ? 1u : 0u, ysum, ymax, amax, ymin, amin, ldy);
}

template <bool kSum, bool kMax, bool kMin>
void backward_of(const WideSide& s, const WideTable& t, const uint32_t* row_ptr, bool mean, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin,
                 const uint32_t* amin, uint64_t ldg, uint32_t d, float* gx, uint64_t ldgx, hipStream_t stream) {
    hipLaunchKernelGGL((neighbor_backward_kernel<kSum, kMax, kMin>), grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.perm, s.list, t, row_ptr, gsum, gmax,
                       amax, gmin, amin, ldg, d, wide_group_lanes(d), mean ? 1u : 0u, gx, ldgx);
}

// the instantiation of a launch: bit 0 a sum (or mean), bit 1 the maximum, bit 2 the minimum
uint32_t selector(const AggregateOps& ops) { return ((ops.sum || ops.mean) ? 1u : 0u) | (ops.max ? 2u : 0u) | (ops.min ? 4u : 0u); }

}  // namespace

hipError_t launch_neighbor_forward(const WideSide& s, AggregateOps ops, const float* x, uint64_t ldx, uint32_t d, float* ysum, float* ymax, uint32_t* amax, float* ymin,
                                   uint32_t* amin, uint64_t ldy, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD || (ops.sum && ops.mean)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    switch (selector(ops)) {
        case 1: forward_of<true, false, false>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        case 2: forward_of<false, true, false>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        case 3: forward_of<true, true, false>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        case 4: forward_of<false, false, true>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        case 5: forward_of<true, false, true>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        case 6: forward_of<false, true, true>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        case 7: forward_of<true, true, true>(s, t, ops.mean, x, ldx, d, ysum, ymax, amax, ymin, amin, ldy, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_neighbor_backward(const WideSide& s, const uint32_t* row_ptr, AggregateOps ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin,
                                    const uint32_t* amin, uint64_t ldg, uint32_t d, float* gx, uint64_t ldgx, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD || (ops.sum && ops.mean) || !s.perm || !row_ptr) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    switch (selector(ops)) {
        case 1: backward_of<true, false, false>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        case 2: backward_of<false, true, false>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        case 3: backward_of<true, true, false>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        case 4: backward_of<false, false, true>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        case 5: backward_of<true, false, true>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        case 6: backward_of<false, true, true>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        case 7: backward_of<true, true, true>(s, t, row_ptr, ops.mean, gsum, gmax, amax, gmin, amin, ldg, d, gx, ldgx, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
