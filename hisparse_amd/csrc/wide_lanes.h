// wide_lanes.h — the device side of wide_products.h's schedule, defined ONCE for every kernel that runs on it: wide_products.hip,
// pattern_attention.hip, attention_backward.hip, heads_attention.hip, heads16_attention.hip, heads_bias_attention.hip,
// heads_dropout_attention.hip, heads16_dropout_attention.hip, gat_attention.hip, gatv2_attention.hip and neighbor_aggregate.hip.  Only .hip files include it.  wide_products.h owns the table, the side and the
// constants; this header owns what a lane does with them:
//   which virtual workgroup gets which row (class_of, Work, pick) and how many trips a wavefront makes so that its shuffles stay
//     convergent (trips_of);
//   a lane's place in its group when a feature row holds several heads (Place, place_of);
//   how the groups of a team and the four wavefronts of a long row merge (merge_lanes, merge_waves; State, raise_to, merge_states for
//     the online softmax of the forward kernels; Best4, outranks, merge_best_lanes, merge_best_waves for the (value, index) pairs of
//     the neighbour aggregation's extremes);
//   the small words around them (f32x4, Sum4, dot4, store4, pick4, lse_of), and for the launchers grid_of and shape_ok.
// The kernels that share these are compared bit for bit by the tests (zero bias against the plain calls, drop_p = 0 against both), so
// the order of every sum below is part of the contract.  A change here reaches every file above: tools/device_asm_digest.py shows
// which kernels' code it moved.  Everything is __forceinline__ and leaves no symbol in a code object.
// A kernel file pulls in what it uses, `using namespace lanes;` where nothing clashes; heads16_attention.hip and
// heads16_dropout_attention.hip keep an eight-sum State under the same name and name what they take.  The two oldest files still write pick and trips_of out in a kernel body (pattern_attention_kernel,
// wide_dot_kernel; wide_gather_kernel has team_row): with the calls they compile to other code, and the header was brought in without
// moving any.  A fix to pick has those three places to visit besides this one.
#ifndef HISPARSE_WIDE_LANES_H_
#define HISPARSE_WIDE_LANES_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {
namespace lanes {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kWaves = kWideThreads / 64;

static_assert(kWideInFlight == 4, "a trip is four entries: its weights (bias words, draws) are dealt to four lanes of a group or head");
static_assert(kWaves == 4, "the long rows' merge adds four wavefronts");

// ---- the schedule ----------------------------------------------------------------------------------------------------------------------
// the class that holds virtual workgroup w: first[] never decreases, and an empty class shares its first workgroup with the next one
__device__ __forceinline__ uint32_t class_of(const WideTable& t, uint64_t w) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 1; k < kWideClasses; ++k) c += w >= t.first[k] ? 1u : 0u;
    return c;
}

// what one lane does in virtual workgroup w: row (column) r with entries lo ... hi, group g of `groups` in a team of `team` lanes
struct Work {
    uint32_t c, r, lo, hi, g, groups, team;
    bool mine;      // false: a team past the end of its class's list runs on with no entries and stores nothing
};

__device__ __forceinline__ Work pick(const WideTable& tab, uint64_t w, const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ list, uint32_t group) {
    Work k = {class_of(tab, w), 0u, 0u, 0u, 0u, 0u, 64u, true};
    if (k.c != 0) {
        k.team = min(group << (2u * k.c), 64u);
        const uint64_t slot = (w - tab.first[k.c]) * (kWideThreads / k.team) + threadIdx.x / k.team;
        k.mine = slot < tab.off[k.c + 1] - tab.off[k.c];
        if (k.mine) {
            k.r = list[tab.off[k.c] + slot];
            k.lo = ptr[k.r];
            k.hi = ptr[k.r + 1];
        }
        k.g = (threadIdx.x & (k.team - 1u)) / group;
        k.groups = k.team / group;
    } else {
        k.r = list[tab.off[0] + (w - tab.first[0])];
        k.lo = ptr[k.r];
        k.hi = ptr[k.r + 1];
        k.g = threadIdx.x / group;
        k.groups = kWideThreads / group;
    }
    return k;
}

// the trips every lane of the wavefront makes: the most any of its teams needs, so that the shuffles (and the dropout kernels' ballot)
// stay convergent
__device__ __forceinline__ uint32_t trips_of(const Work& k) {
    const uint32_t per_trip = kWideInFlight * k.groups;
    uint32_t trips = (k.hi - k.lo + per_trip - 1u) / per_trip;
#pragma unroll
    for (uint32_t k2 = 32; k2; k2 >>= 1) trips = max(trips, uint32_t(__shfl_xor(int(trips), int(k2), 64)));
    return trips;
}

// ---- a lane's place among the heads of a feature row --------------------------------------------------------------------------------------
// this lane's place in its group: its 16 bytes of a feature row and the head they belong to.  A kernel that reads no `first` or `deals`
// pays nothing for them.
struct Place {
    uint32_t at;              // first element of the chunk; 0 for a dead lane
    uint32_t head;            // 0 for a dead lane
    uint32_t head_lanes;      // d / kChunk
    int first;                // the first lane of this lane's head in the wavefront
    bool live, lead;          // lead: the first lane of a live head, which stores the head's words (lse, D, gel, ger)
    bool deals;               // one of the first kWideInFlight lanes of a live head of at least that many lanes: lane i of them stores entry i's gbias word
};

// kChunk: the elements of 16 bytes, 4 fp32 words or 8 bf16.  d is a power of two from kChunk (shape_ok).
template <uint32_t kChunk = 4>
__device__ __forceinline__ Place place_of(uint32_t group, uint32_t heads, uint32_t d) {
    const uint32_t chunk = threadIdx.x & (group - 1u);
    Place p;
    p.head_lanes = d / kChunk;
    p.live = chunk * kChunk < heads * d;
    p.at = p.live ? chunk * kChunk : 0u;
    p.head = p.live ? chunk >> (__builtin_ctz(d) - __builtin_ctz(kChunk)) : 0u;
    p.first = int(threadIdx.x & 63u & ~(p.head_lanes - 1u));
    p.lead = p.live && (chunk & (p.head_lanes - 1u)) == 0u;
    p.deals = p.live && p.head_lanes >= kWideInFlight && (chunk & (p.head_lanes - 1u)) < kWideInFlight;
    return p;
}

// ---- words of a chunk ------------------------------------------------------------------------------------------------------------------
struct Sum4 {
    double a, b, c, d;
};

// the four fp32 products of a chunk added in double
__device__ __forceinline__ double dot4(f32x4 a, f32x4 b) {
    return ((static_cast<double>(a.x * b.x) + static_cast<double>(a.y * b.y)) + static_cast<double>(a.z * b.z)) + static_cast<double>(a.w * b.w);
}

__device__ __forceinline__ void store4(float* dst, double x, double y, double z, double w) {
    f32x4 v = {static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), static_cast<float>(w)};
    *reinterpret_cast<f32x4*>(dst) = v;
}

// entry i's word of a trip's four, for i that is not known at compile time (no indexed array: that would be scratch)
template <typename T>
__device__ __forceinline__ T pick4(const T (&a)[kWideInFlight], uint32_t i) { return i == 0u ? a[0] : i == 1u ? a[1] : i == 2u ? a[2] : a[3]; }

// lse as the weights read it: a word that is not finite (a dead or bad row of the forward) makes every weight of its row and head NaN
__device__ __forceinline__ double lse_of(float l) { return __builtin_isfinite(l) ? static_cast<double>(l) : static_cast<double>(__builtin_nanf("")); }

// ---- the online softmax state of the fp32 forward kernels ------------------------------------------------------------------------------
// the online softmax state of one lane: its head's m and l, and the four sums of its chunk
struct State {
    float m;      // one of the t words, or -inf
    double l;
    Sum4 acc;
};

// NaN is never the maximum (fmaxf returns the other operand)
__device__ __forceinline__ void raise_to(State& s, float m_new) {
    if (m_new != s.m) {      // m_new > s.m: exp(-inf - finite) = 0 for a state that is still empty
        const double f = exp(static_cast<double>(s.m) - static_cast<double>(m_new));
        s.l *= f;
        s.acc.a *= f;
        s.acc.b *= f;
        s.acc.c *= f;
        s.acc.d *= f;
        s.m = m_new;
    }
}

// the states of the lanes that differ in the bits from ... to/2 of the lane index become one: the maximum first, then the rescaled sums
__device__ __forceinline__ void merge_states(State& s, uint32_t from, uint32_t to) {
    float m = s.m;
    for (uint32_t k = from; k < to; k <<= 1) m = fmaxf(m, __shfl_xor(m, int(k), 64));
    raise_to(s, m);
    for (uint32_t k = from; k < to; k <<= 1) {
        s.l += __shfl_xor(s.l, int(k), 64);
        s.acc.a += __shfl_xor(s.acc.a, int(k), 64);
        s.acc.b += __shfl_xor(s.acc.b, int(k), 64);
        s.acc.c += __shfl_xor(s.acc.c, int(k), 64);
        s.acc.d += __shfl_xor(s.acc.d, int(k), 64);
    }
}

// ---- plain sums across a team and across the wavefronts of a long row ---------------------------------------------------------------------
// the sums of the lanes that differ in the bits from ... to/2 of the lane index become one
template <uint32_t kN>
__device__ __forceinline__ void merge_lanes(double (&acc)[kN], uint32_t from, uint32_t to) {
    for (uint32_t k = from; k < to; k <<= 1) {
#pragma unroll
        for (uint32_t j = 0; j < kN; ++j) acc[j] += __shfl_xor(acc[j], int(k), 64);
    }
}

// a long row: the four wavefronts' sums through LDS into wave 0's lanes < group (the others' acc is left as it was); the caller syncs
// once more before the next use of red
template <uint32_t kN>
__device__ __forceinline__ void merge_waves(double (&red)[kWaves][kN][64], double (&acc)[kN], uint32_t lane, uint32_t wave, uint32_t group) {
    if (lane < group) {
#pragma unroll
        for (uint32_t j = 0; j < kN; ++j) red[wave][j][lane] = acc[j];
    }
    __syncthreads();
    if (wave == 0 && lane < group) {
#pragma unroll
        for (uint32_t j = 0; j < kN; ++j) acc[j] = ((red[0][j][lane] + red[1][j][lane]) + red[2][j][lane]) + red[3][j][lane];
    }
}

// ---- (value, index) pairs across a team and across the wavefronts of a long row: the extremes of neighbor_aggregate.hip ---------------------
// the four candidates of a lane's chunk: v[j] is a word of X as it was loaded (never the result of arithmetic), e[j] the CSR index of its
// entry.  An empty candidate is (-inf, ~0u) for the maximum and (+inf, ~0u) for the minimum: every entry outranks it, an entry of the
// same value by its smaller index.
struct Best4 {
    float v[4];
    uint32_t e[4];
};

// include/hisparse_aggregate.h's winner rule: (v, e) is taken over (bv, be) when it is a NaN against a non-NaN, else when the IEEE
// comparison says so (fmaxf and v_max_f32 would DROP the NaN), else, among equals (== or both NaN), when its index is the smaller.  A
// lexicographic order on (rank, e), total on the entries of a row: folding candidates in any order and any grouping gives one winner.
template <bool kMax>
__device__ __forceinline__ bool outranks(float v, uint32_t e, float bv, uint32_t be) {
    const bool vn = v != v, bn = bv != bv;
    const bool better = (kMax ? v > bv : v < bv) || (vn && !bn);
    const bool equal = v == bv || (vn && bn);
    return better || (equal && e < be);
}

template <bool kMax>
__device__ __forceinline__ void offer(Best4& b, uint32_t j, float v, uint32_t e) {
    if (outranks<kMax>(v, e, b.v[j], b.e[j])) {
        b.v[j] = v;
        b.e[j] = e;
    }
}

// the pairs of the lanes that differ in the bits from ... to/2 of the lane index become one: every such lane ends with the winner
template <bool kMax>
__device__ __forceinline__ void merge_best_lanes(Best4& b, uint32_t from, uint32_t to) {
    for (uint32_t k = from; k < to; k <<= 1) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const float v = __shfl_xor(b.v[j], int(k), 64);
            const uint32_t e = uint32_t(__shfl_xor(int(b.e[j]), int(k), 64));
            offer<kMax>(b, j, v, e);
        }
    }
}

// a long row: the four wavefronts' pairs through LDS into wave 0's lanes < group (the others' are left as they were); the caller syncs
// once more before the next use of the two arrays
template <bool kMax>
__device__ __forceinline__ void merge_best_waves(float (&red_v)[kWaves][4][64], uint32_t (&red_e)[kWaves][4][64], Best4& b, uint32_t lane, uint32_t wave, uint32_t group) {
    if (lane < group) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            red_v[wave][j][lane] = b.v[j];
            red_e[wave][j][lane] = b.e[j];
        }
    }
    __syncthreads();
    if (wave == 0 && lane < group) {
#pragma unroll
        for (uint32_t w = 1; w < kWaves; ++w) {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) offer<kMax>(b, j, red_v[w][j][lane], red_e[w][j][lane]);
        }
    }
}

// ---- for the launchers -------------------------------------------------------------------------------------------------------------------
// the grid of a launch: every virtual workgroup of the table, at most blocks_per_cu per compute unit (the kernels stride from there).  A
// launcher passes kWideBlocksPerCu, so that its launch line names both numbers of its geometry, the cap and dim3(kWideThreads); the source
// tests of each kernel file (test_schedule_is_the_wide_products_unchanged) read them there.
inline dim3 grid_of(const WideSide& s, const WideTable& t, uint32_t blocks_per_cu) {
    return dim3(std::min<uint32_t>(t.first[kWideClasses], (s.compute_units ? s.compute_units : 1u) * blocks_per_cu));
}

// what place_of relies on: d a power of two from `chunk` (the elements of 16 bytes), and a row of heads * d elements in at most
// kWideMaxD / 4 chunks (fp32: heads * d at most kWideMaxD)
inline bool shape_ok(uint32_t heads, uint32_t d, uint32_t chunk = 4u) {
    return d >= chunk && (d & (d - 1u)) == 0u && heads >= 1u && uint64_t(heads) * d <= uint64_t(kWideMaxD / 4u) * chunk;
}

}  // namespace lanes
}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_WIDE_LANES_H_
