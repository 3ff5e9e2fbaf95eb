// heads16_attention.hip — include/hisparse_heads_bf16.h's three kernels: multi-head attention over a CSR pattern, forward and backward,
// with ROW-MAJOR bf16 operands stored [index][head][feature] (heads * d <= 512 elements, d a power of two from 8) and no per-entry array.
// ONE launch forward, TWO backward.  They are heads_attention.hip's kernels with a lane owning one 16-byte chunk of EIGHT bf16 elements
// where a lane there owns four fp32 words.  Which row a lane works on (pick, trips_of), its Place (place_of<8>) and the merges of plain
// sums are wide_lanes.h's, the definitions the fp32 files use; this file owns the bf16 words (F8, widen, dot8, store8), an eight-sum
// State with its raise_to and merge_states, its trip loops, the three kernels and their launchers.  The schedule is wide_products.h's,
// unchanged, taken at the row's size in 16-byte chunks: the launchers pass heads * d / 2 where the fp32 launchers pass heads * d, so the
// group of a row is half as wide and a wavefront holds twice the entries in flight per trip.
//   head_lanes = d / 8, head = chunk / head_lanes.  The shuffles of a dot run over k < head_lanes, so every lane of a head holds the
//     head's s (and gp), and every lane carries its own head's m and l (forward) or D (backward).
//   Where a head has at least kWideInFlight lanes (d >= 32), lane i of it forms the weight of the trip's entry i and the others fetch
//     it from the head's first lane on: one exp per lane and trip.  Below that each lane forms its four weights.
//   The groups of a team merge by lane shuffles over the bits group ... team / 2, which pair the same chunk, hence the same head; the
//     four wavefronts of a long row or column merge lane by lane through LDS.
//   Lanes of a group past heads * d / 8 (3 heads of d = 16 in a group of 8) are dead: they form every address from head 0 and chunk 0,
//     take part in every shuffle (their partners are dead lanes too: heads * d / 8 is a multiple of head_lanes) and store nothing.
// An element is widened to fp32 by a shift or a mask of its dword (exact); the sums stay in double as in the fp32 kernels; an output word
// is rounded to fp32 and then to bf16, round to nearest even with NaN kept (the compiler's conversion of float to __bf16, which gfx950
// has in hardware), eight of them stored as one 16-byte word.  lse words are fp32 and D words double: the fp32 kernels' own.
// Every output word has one writer: no atomics, no scratch, no matrix engine, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "heads16_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // a chunk: eight bf16 elements, element 2 i in the low half of dword i
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// named one by one: State, raise_to and merge_states below are this file's own, under the names wide_lanes.h has for the fp32 ones
using lanes::grid_of;
using lanes::kWaves;
using lanes::lse_of;
using lanes::merge_lanes;
using lanes::merge_waves;
using lanes::pick;
using lanes::Place;
using lanes::place_of;
using lanes::shape_ok;
using lanes::trips_of;
using lanes::Work;

constexpr uint32_t kChunk = 8;               // elements per lane
constexpr uint32_t kSums = 2 * kChunk;       // backward: double sums per lane that cross lanes, a and b of the row side, gK and gV of the column side

__device__ __forceinline__ u32x4 load_chunk(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// the eight elements of a chunk as fp32: a bf16 is the upper half of the fp32 of the same value
struct F8 {
    float x[kChunk];
};
__device__ __forceinline__ F8 widen(u32x4 c) {
    F8 f;
    f.x[0] = __uint_as_float(c.x << 16);
    f.x[1] = __uint_as_float(c.x & 0xFFFF0000u);
    f.x[2] = __uint_as_float(c.y << 16);
    f.x[3] = __uint_as_float(c.y & 0xFFFF0000u);
    f.x[4] = __uint_as_float(c.z << 16);
    f.x[5] = __uint_as_float(c.z & 0xFFFF0000u);
    f.x[6] = __uint_as_float(c.w << 16);
    f.x[7] = __uint_as_float(c.w & 0xFFFF0000u);
    return f;
}

// the eight fp32 products of a chunk (each exact: two bf16 factors) added in double
__device__ __forceinline__ double dot8(const F8& a, u32x4 bc) {
    const F8 b = widen(bc);
    double s = static_cast<double>(a.x[0] * b.x[0]);
#pragma unroll
    for (uint32_t j = 1; j < kChunk; ++j) s += static_cast<double>(a.x[j] * b.x[j]);
    return s;
}

// one rounding to fp32, one from fp32 to bf16 (nearest even, NaN stays NaN), one 16-byte store
__device__ __forceinline__ void store8(uint16_t* dst, const double* x) {
    bf16x8 v;
#pragma unroll
    for (uint32_t j = 0; j < kChunk; ++j) v[j] = static_cast<__bf16>(static_cast<float>(x[j]));
    *reinterpret_cast<bf16x8*>(dst) = v;
}
__device__ __forceinline__ void store_zeros(uint16_t* dst) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(dst) = z;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// the online softmax state of one lane: its head's m and l, and the eight sums of its chunk.  An array of 8, defined here: one State<N>
// template shared with the fp32 files (four named sums) reorders the shuffles of their merge, and their device code must not move.
struct State {
    float m;      // one of the t words, or -inf
    double l;
    double acc[kChunk];
};

// NaN is never the maximum (fmaxf returns the other operand)
__device__ __forceinline__ void raise_to(State& s, float m_new) {
    if (m_new != s.m) {      // m_new > s.m: exp(-inf - finite) = 0 for a state that is still empty
        const double f = exp(static_cast<double>(s.m) - static_cast<double>(m_new));
        s.l *= f;
#pragma unroll
        for (uint32_t j = 0; j < kChunk; ++j) s.acc[j] *= f;
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
#pragma unroll
        for (uint32_t j = 0; j < kChunk; ++j) s.acc[j] += __shfl_xor(s.acc[j], int(k), 64);
    }
}

// One row's entries lo + g, lo + g + groups, ... through this lane's state.  Every lane of the wavefront makes `trips` trips; an entry
// past the end gathers row 0 of K and V (in bounds, in the cache) without reading idx, scores -inf and is not added.
__device__ __forceinline__ void attend_entries(State& st, const uint32_t* __restrict__ idx, const F8& qv, const Place& pl, const uint16_t* __restrict__ k_chunk, uint64_t ldk,
                                               const uint16_t* __restrict__ v_chunk, uint64_t ldv, float scale, const Work& wk, uint32_t trips) {
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
        bool ok[kWideInFlight];
        uint32_t col[kWideInFlight];
        u32x4 kv[kWideInFlight], vv[kWideInFlight];
        double s[kWideInFlight];
        float t[kWideInFlight];
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            const uint64_t ei = e + uint64_t(i) * wk.groups;
            ok[i] = ei < wk.hi;
            col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kv[i] = load_chunk(k_chunk + uint64_t(col[i]) * ldk);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = load_chunk(v_chunk + uint64_t(col[i]) * ldv);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] = dot8(qv, kv[i]);
        for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] += __shfl_xor(s[i], int(k), 64);
        }
        float top = -INFINITY;
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            t[i] = ok[i] ? scale * static_cast<float>(s[i]) : -INFINITY;
            top = fmaxf(top, t[i]);
        }
        raise_to(st, fmaxf(st.m, top));
        // a -inf score weighs exactly 0, also while m is -inf itself; a NaN score, or +inf under m = +inf, gives NaN
        double w[kWideInFlight];
        if (pl.head_lanes >= kWideInFlight) {      // one exp per lane: lane i of the head forms entry i's weight and the others fetch it
            const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
            const float tm = mine == 0u ? t[0] : mine == 1u ? t[1] : mine == 2u ? t[2] : t[3];
            const double wm = tm == -INFINITY ? 0.0 : exp(static_cast<double>(tm) - static_cast<double>(st.m));
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) w[i] = __shfl(wm, pl.first + int(i), 64);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) w[i] = t[i] == -INFINITY ? 0.0 : exp(static_cast<double>(t[i]) - static_cast<double>(st.m));
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            if (ok[i]) {
                const F8 x = widen(vv[i]);
                st.l += w[i];
#pragma unroll
                for (uint32_t j = 0; j < kChunk; ++j) st.acc[j] += w[i] * static_cast<double>(x.x[j]);
            }
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void heads16_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                      WideTable tab, const uint16_t* __restrict__ q, uint64_t ldq, const uint16_t* __restrict__ k, uint64_t ldk,
                                                                      const uint16_t* __restrict__ v, uint64_t ldv, uint32_t heads, uint32_t d, uint32_t group, float scale,
                                                                      uint16_t* __restrict__ y, uint64_t ldy, float* __restrict__ lse, uint64_t ldl) {
    __shared__ double red[kWaves][kChunk][64];
    __shared__ double red_l[kWaves][64];      // per lane: a lane's l and m are its head's
    __shared__ float red_m[kWaves][64];
    const Place pl = place_of<kChunk>(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const F8 qv = widen(load_chunk(q + uint64_t(wk.r) * ldq + pl.at));      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        attend_entries(st, idx, qv, pl, k + pl.at, ldk, v + pl.at, ldv, scale, wk, trips);
        merge_states(st, group, wk.team);
        uint16_t* dst = y + uint64_t(wk.r) * ldy + pl.at;
        float* dst_l = lse ? lse + uint64_t(wk.r) * ldl + pl.head : nullptr;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) {
                    store_zeros(dst);
                } else {
                    double out[kChunk];
#pragma unroll
                    for (uint32_t j = 0; j < kChunk; ++j) out[j] = st.acc[j] / st.l;
                    store8(dst, out);
                }
                if (pl.lead && dst_l) *dst_l = wk.lo == wk.hi ? -INFINITY : static_cast<float>(static_cast<double>(st.m) + log(st.l));
            }
        } else {      // a long row: the four wavefronts' states through LDS, lane by lane
            if (lane < group) {
#pragma unroll
                for (uint32_t j = 0; j < kChunk; ++j) red[wave][j][lane] = st.acc[j];
                red_l[wave][lane] = st.l;
                red_m[wave][lane] = st.m;
            }
            __syncthreads();
            if (wave == 0 && lane < group && pl.live) {
                const float m = fmaxf(fmaxf(red_m[0][lane], red_m[1][lane]), fmaxf(red_m[2][lane], red_m[3][lane]));
                double l = 0.0;
                double out[kChunk] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (uint32_t k2 = 0; k2 < kWaves; ++k2) {
                    const double f = red_m[k2][lane] == m ? 1.0 : exp(static_cast<double>(red_m[k2][lane]) - static_cast<double>(m));
                    l += f * red_l[k2][lane];
#pragma unroll
                    for (uint32_t j = 0; j < kChunk; ++j) out[j] += f * red[k2][j][lane];
                }
#pragma unroll
                for (uint32_t j = 0; j < kChunk; ++j) out[j] /= l;
                store8(dst, out);
                if (pl.lead && dst_l) *dst_l = static_cast<float>(static_cast<double>(m) + log(l));
            }
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// One trip of a group: kWideInFlight entries, their gathered chunks and this lane's head's two dots (the same words in every lane of the head).
struct Trip {
    bool ok[kWideInFlight];
    uint32_t at[kWideInFlight];      // the gathered operands' row: idx[e], 0 for an entry past the end
    u32x4 a[kWideInFlight], b[kWideInFlight];
    double s[kWideInFlight], gp[kWideInFlight];
    float ls[kWideInFlight];         // column side only: lse and D of the entry's row and this lane's head
    double ds[kWideInFlight];
};

// s[i] = ha . A[at[i]], gp[i] = hb . B[at[i]] over the head's d elements: an entry past the end gathers row 0 (in bounds, in the cache)
// without reading idx and is not added by the caller.
template <bool kPerEntry>
__device__ __forceinline__ void gather_dots(Trip& t, const uint32_t* __restrict__ idx, uint64_t e, const Work& wk, const Place& pl, const F8& ha, const F8& hb,
                                            const uint16_t* __restrict__ a_chunk, uint64_t lda, const uint16_t* __restrict__ b_chunk, uint64_t ldb, const float* __restrict__ lse,
                                            uint64_t ldl, const double* __restrict__ dsum, uint64_t ldd) {
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        const uint64_t ei = e + uint64_t(i) * wk.groups;
        t.ok[i] = ei < wk.hi;
        t.at[i] = t.ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) t.a[i] = load_chunk(a_chunk + uint64_t(t.at[i]) * lda);
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) t.b[i] = load_chunk(b_chunk + uint64_t(t.at[i]) * ldb);
    if (kPerEntry) {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            t.ls[i] = lse[uint64_t(t.at[i]) * ldl + pl.head];
            t.ds[i] = dsum[uint64_t(t.at[i]) * ldd + pl.head];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        t.s[i] = dot8(ha, t.a[i]);
        t.gp[i] = dot8(hb, t.b[i]);
    }
    for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            t.s[i] += __shfl_xor(t.s[i], int(k), 64);
            t.gp[i] += __shfl_xor(t.gp[i], int(k), 64);
        }
    }
}

// p[i] = exp(scale * (float)s[i] - lse_of(l[i])): s rounded once, one fp32 multiply, the rest double.  A -inf score under a finite lse weighs
// exactly 0 (exp(-inf)).  With at least kWideInFlight lanes in a head, lane i of it forms entry i's weight and the others fetch it.
__device__ __forceinline__ void weights(double (&p)[kWideInFlight], const double (&s)[kWideInFlight], const float (&l)[kWideInFlight], float scale, const Place& pl) {
    if (pl.head_lanes >= kWideInFlight) {
        const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
        const double sm = mine == 0u ? s[0] : mine == 1u ? s[1] : mine == 2u ? s[2] : s[3];
        const float lm = mine == 0u ? l[0] : mine == 1u ? l[1] : mine == 2u ? l[2] : l[3];
        const double pm = exp(static_cast<double>(scale * static_cast<float>(sm)) - lse_of(lm));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = __shfl(pm, pl.first + int(i), 64);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = exp(static_cast<double>(scale * static_cast<float>(s[i])) - lse_of(l[i]));
    }
}

// gQ's eight words of a lane from its sums a (0 ... 7) and b (8 ... 15) and its head's D
__device__ __forceinline__ void store_gq(uint16_t* dst, const double (&acc)[kSums], double dd, double sc) {
    double out[kChunk];
#pragma unroll
    for (uint32_t j = 0; j < kChunk; ++j) out[j] = sc * (acc[j] - dd * acc[kChunk + j]);
    store8(dst, out);
}

__global__ __launch_bounds__(kWideThreads) void heads16_backward_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                            WideTable tab, const uint16_t* __restrict__ q, uint64_t ldq, const uint16_t* __restrict__ k, uint64_t ldk,
                                                                            const uint16_t* __restrict__ v, uint64_t ldv, const uint16_t* __restrict__ gy, uint64_t ldgy,
                                                                            const float* __restrict__ lse, uint64_t ldl, uint32_t heads, uint32_t d, uint32_t group, float scale,
                                                                            uint16_t* __restrict__ gq, uint64_t ldgq, double* __restrict__ dsum, uint64_t ldd) {
    __shared__ double red[kWaves][kSums][64];
    __shared__ double red_d[kWaves][64];      // per lane: a lane's D is its head's
    const Place pl = place_of<kChunk>(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale);
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const F8 qv = widen(load_chunk(q + uint64_t(wk.r) * ldq + pl.at));      // held for the whole row
        const F8 gyv = widen(load_chunk(gy + uint64_t(wk.r) * ldgy + pl.at));
        const float l = lse[uint64_t(wk.r) * ldl + pl.head];
        double acc[kSums] = {};      // a (0 ... 7) and b (8 ... 15) of this lane's chunk
        double dd = 0.0;
        const float ls[kWideInFlight] = {l, l, l, l};
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<false>(t, idx, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, qv, gyv, k + pl.at, ldk, v + pl.at, ldv, nullptr, 0, nullptr, 0);
            double p[kWideInFlight];
            weights(p, t.s, ls, scale, pl);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double pg = p[i] * t.gp[i];
                    const F8 x = widen(t.a[i]);
                    dd += pg;
#pragma unroll
                    for (uint32_t j = 0; j < kChunk; ++j) {
                        acc[j] += pg * static_cast<double>(x.x[j]);
                        acc[kChunk + j] += p[i] * static_cast<double>(x.x[j]);
                    }
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        for (uint32_t k2 = group; k2 < wk.team; k2 <<= 1) dd += __shfl_xor(dd, int(k2), 64);
        uint16_t* dst = gq + uint64_t(wk.r) * ldgq + pl.at;
        double* dst_d = dsum + uint64_t(wk.r) * ldd + pl.head;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) {
                    store_zeros(dst);
                    dd = 0.0;
                } else {
                    store_gq(dst, acc, dd, sc);
                }
                if (pl.lead) *dst_d = dd;
            }
        } else {      // a long row: the four wavefronts' sums through LDS, lane by lane
            if (lane < group) red_d[wave][lane] = dd;
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) {
                dd = ((red_d[0][lane] + red_d[1][lane]) + red_d[2][lane]) + red_d[3][lane];
                store_gq(dst, acc, dd, sc);
                if (pl.lead) *dst_d = dd;
            }
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void heads16_backward_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                            WideTable tab, const uint16_t* __restrict__ q, uint64_t ldq, const uint16_t* __restrict__ k, uint64_t ldk,
                                                                            const uint16_t* __restrict__ v, uint64_t ldv, const uint16_t* __restrict__ gy, uint64_t ldgy,
                                                                            const float* __restrict__ lse, uint64_t ldl, const double* __restrict__ dsum, uint64_t ldd, uint32_t heads,
                                                                            uint32_t d, uint32_t group, float scale, uint16_t* __restrict__ gk, uint64_t ldgk, uint16_t* __restrict__ gv,
                                                                            uint64_t ldgv) {
    __shared__ double red[kWaves][kSums][64];
    const Place pl = place_of<kChunk>(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale);
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const F8 kv = widen(load_chunk(k + uint64_t(wk.r) * ldk + pl.at));      // held for the whole column
        const F8 vv = widen(load_chunk(v + uint64_t(wk.r) * ldv + pl.at));
        double acc[kSums] = {};      // gK (0 ... 7) and gV (8 ... 15) of this lane's chunk
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<true>(t, idx, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, kv, vv, q + pl.at, ldq, gy + pl.at, ldgy, lse, ldl, dsum, ldd);
            double p[kWideInFlight];
            weights(p, t.s, t.ls, scale, pl);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double gs = sc * (p[i] * (t.gp[i] - t.ds[i]));
                    const F8 x = widen(t.a[i]), g = widen(t.b[i]);
#pragma unroll
                    for (uint32_t j = 0; j < kChunk; ++j) {
                        acc[j] += gs * static_cast<double>(x.x[j]);
                        acc[kChunk + j] += p[i] * static_cast<double>(g.x[j]);
                    }
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        uint16_t* dst_k = gk + uint64_t(wk.r) * ldgk + pl.at;
        uint16_t* dst_v = gv + uint64_t(wk.r) * ldgv + pl.at;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {      // a column without entries has summed nothing: +0.0, the word 0x0000
                store8(dst_k, acc);
                store8(dst_v, acc + kChunk);
            }
        } else {
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) {
                store8(dst_k, acc);
                store8(dst_v, acc + kChunk);
            }
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_heads16_forward(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, uint32_t heads, uint32_t d,
                                  float scale, uint16_t* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream) {
    if (!shape_ok(heads, d, kChunk)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d / 2);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(heads16_forward_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, heads, d, wide_group_lanes(heads * d / 2),
                       scale, y, ldy, lse, ldl);
    return hipGetLastError();
}

hipError_t launch_heads16_backward_rows(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                        uint64_t ldgy, const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float scale, uint16_t* gq, uint64_t ldgq, double* dsum, uint64_t ldd,
                                        hipStream_t stream) {
    if (!shape_ok(heads, d, kChunk) || ldd < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d / 2);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(heads16_backward_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, heads, d,
                       wide_group_lanes(heads * d / 2), scale, gq, ldgq, dsum, ldd);
    return hipGetLastError();
}

hipError_t launch_heads16_backward_cols(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                        uint64_t ldgy, const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float scale, uint16_t* gk,
                                        uint64_t ldgk, uint16_t* gv, uint64_t ldgv, hipStream_t stream) {
    if (!shape_ok(heads, d, kChunk) || ldd < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d / 2);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(heads16_backward_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, dsum, ldd, heads,
                       d, wide_group_lanes(heads * d / 2), scale, gk, ldgk, gv, ldgv);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
