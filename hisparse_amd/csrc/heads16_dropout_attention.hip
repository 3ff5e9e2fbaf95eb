// heads16_dropout_attention.hip — include/hisparse_heads_dropout_bf16.h's three kernels: the multi-head attention step of
// heads16_attention.hip (ROW-MAJOR bf16 operands, a lane owning one 16-byte chunk of EIGHT elements) with the per-entry, per-head fp32
// bias and the DROPOUT ON THE ATTENTION WEIGHTS of heads_dropout_attention.hip, P'[e][h] = keep(e, h) c P[e][h] with c = 1 / (1 - drop_p),
// forward (ONE launch) and backward (TWO).  The bias is optional (a wave-uniform branch: without one no bias word is read and
// t = fl32(scale * s), the plain calls' score).  No mask is stored or read: keep(e, h) is recomputed from philox.h's generator, keyed by
// the call's seed, offset, the entry's index e IN THE CALLER'S CSR ORDER and the head.
// The schedule is wide_products.h's, unchanged, taken at the row's size in 16-byte chunks (the launchers pass heads * d / 2); Place, Work,
// pick, trips_of and the merges of plain sums are wide_lanes.h's.  The bf16 words (F8, widen, dot8, store8), the eight-sum State with its
// raise_to and merge_states are heads16_attention.hip's, restated here word for word: that file's device code must not move, and the order
// of every sum below is its order, which is what the tests compare bit for bit at drop_p = 0.  The trip loops follow
// heads_dropout_attention.hip's:
//   head_lanes = d / 8.  Where a head has at least kWideInFlight lanes (d >= 32) lane i of each four forms the score, the weight and the
//     draw of the trip's entry i alone and loads that entry's bias word (column side: its map word) alone; the keep bits reach the head's
//     lanes through ONE ballot of the wavefront, bit first + i being the decision of entry i.  Below that width (d = 8, 16) a lane forms
//     the scores and loads the bias words of its four entries itself, but still draws ONCE: a generator call yields the words of four
//     heads, so lane i of each aligned four lanes (the chunks of one such four heads) draws entry i and four ballots hand out the bits
//     (`keeps`).
//   Forward: l is summed over ALL entries of the row (lse is the words of the call without dropout) and the chunk's sums over the kept
//     ones; c multiplies each output word once.  A row whose kept set is empty in a head stores 0 / l * c = +0.0 there, the word 0x0000.
//   Backward: GP becomes w GP with w = keep ? c : 0 on both sides, and the column side weighs gV with w P; D, GS and gbias keep their form.
//     The column side takes the entry's CSR index from the map word perm[e'], which it streams beside idx.
//   With drop_p = 0 every word is kept and c = 1.0, and x * 1.0 = x; a bias of +0.0 leaves t's value: the outputs are
//     heads16_attention.hip's bit for bit.
// An output word is rounded to fp32 and then to bf16 (nearest even, NaN kept), eight of them stored as one 16-byte word; lse and gbias
// words are fp32 and D words double.  Every output word has one writer: no atomics, no scratch, no matrix engine, no inline assembly, and
// no more LDS than the kernels of heads16_attention.hip declare.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "heads16_dropout_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // a chunk: eight bf16 elements, element 2 i in the low half of dword i
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// named one by one: State, raise_to and merge_states below are the eight-sum ones, under the names wide_lanes.h has for the fp32 ones
using lanes::grid_of;
using lanes::kWaves;
using lanes::lse_of;
using lanes::merge_lanes;
using lanes::merge_waves;
using lanes::pick;
using lanes::pick4;
using lanes::Place;
using lanes::place_of;
using lanes::shape_ok;
using lanes::trips_of;
using lanes::Work;

constexpr uint32_t kChunk = 8;               // elements per lane
constexpr uint32_t kSums = 2 * kChunk;       // backward: double sums per lane that cross lanes, a and b of the row side, gK and gV of the column side

// ---- the bf16 words of heads16_attention.hip ----------------------------------------------------------------------------------------------
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

// the online softmax state of one lane: its head's m and l, and the eight sums of its chunk
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

// ---- the bias and the draws of heads_dropout_attention.hip ----------------------------------------------------------------------------------
// t = fl32(fl32(scale * s) + b) with a bias: one fp32 multiply, then one fp32 add; t = fl32(scale * s) without
__device__ __forceinline__ float score(float scale, double s, float b, bool has_bias) {
    const float t = __fmul_rn(scale, static_cast<float>(s));
    return has_bias ? __fadd_rn(t, b) : t;
}

// The keep decisions of a trip's four entries for this lane's head.  ent[i] is entry i's index in the caller's CSR order and entm the one
// of the entry this lane deals (lane i of each four: entry i); an entry past the end carries index 0 or an index past the end, its draw
// reads no memory and its decision is never used.  With at least kWideInFlight lanes in a head each lane draws once and the wavefront
// shares the bits by one ballot (every lane of the wavefront is here: the trip loops are uniform).  Below that width (d = 8, 16) one
// generator call still yields the words of the FOUR heads 4 q ... 4 q + 3 of an entry, and four neighbouring lanes of a group of at
// least four hold chunks of one such four (one or two lanes a head): lane i of each aligned four draws entry i's four words alone,
// four ballots hand out the bits (ballot h & 3 is head h's, bit `four + i` entry i's), and a lane still draws once per trip.  A dead
// lane draws for the heads its chunk would hold, so that a live lane beside it finds its bits.  Only a group of fewer than four lanes
// ((1, 8), (2, 8), (1, 16)) is left to draw four times per lane.
__device__ __forceinline__ void keeps(bool (&kp)[kWideInFlight], const philox::Dropout& dr, const uint32_t (&ent)[kWideInFlight], uint32_t entm, const Place& pl, uint32_t group) {
    if (pl.head_lanes >= kWideInFlight) {
        const uint64_t kept = __ballot(philox::keep(dr, entm, pl.head));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kp[i] = ((kept >> (uint32_t(pl.first) + i)) & 1u) != 0u;
    } else if (group >= kWideInFlight) {
        const uint32_t head_at = (threadIdx.x & (group - 1u)) >> (pl.head_lanes >> 1);      // head_lanes is 1 or 2 here
        const philox::Words x = philox::philox4x32_10(pick4(ent, threadIdx.x & (kWideInFlight - 1u)), head_at >> 2, dr.off0, dr.off1, dr.key0, dr.key1);
        const uint64_t k0 = __ballot(x.a >= dr.thr), k1 = __ballot(x.b >= dr.thr), k2 = __ballot(x.c >= dr.thr), k3 = __ballot(x.d >= dr.thr);
        const uint32_t h = pl.head & 3u;
        const uint64_t kept = h == 0u ? k0 : h == 1u ? k1 : h == 2u ? k2 : k3;
        const uint32_t four = threadIdx.x & 63u & ~(kWideInFlight - 1u);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kp[i] = ((kept >> (four + i)) & 1u) != 0u;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kp[i] = philox::keep(dr, ent[i], pl.head);
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// One row's entries lo + g, lo + g + groups, ... through this lane's state: m and l over all entries, the eight sums over the kept ones.
// Every lane of the wavefront makes `trips` trips; an entry past the end gathers row 0 of K and V (in bounds, in the cache) without reading
// idx or bias, scores -inf and is not added.  bias_head = bias + this lane's head (never dereferenced without a bias).
__device__ __forceinline__ void attend_entries(State& st, const uint32_t* __restrict__ idx, const F8& qv, const Place& pl, const uint16_t* __restrict__ k_chunk, uint64_t ldk,
                                               const uint16_t* __restrict__ v_chunk, uint64_t ldv, const float* __restrict__ bias_head, uint64_t ldb, float scale,
                                               const philox::Dropout& dr, const Work& wk, uint32_t trips, uint32_t group) {
    const bool has_bias = bias_head != nullptr;
    const bool deal = pl.head_lanes >= kWideInFlight;      // one bias word, one score, one exp and one draw per lane and trip instead of four
    const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
        bool ok[kWideInFlight], kp[kWideInFlight];
        uint32_t col[kWideInFlight], ent[kWideInFlight];
        u32x4 kv[kWideInFlight], vv[kWideInFlight];
        double s[kWideInFlight];
        float t[kWideInFlight], b[kWideInFlight];
        const uint64_t em = e + uint64_t(mine) * wk.groups;
        float bm = 0.0f;
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            const uint64_t ei = e + uint64_t(i) * wk.groups;
            ok[i] = ei < wk.hi;
            ent[i] = uint32_t(ei);
            col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            b[i] = has_bias && !deal && ok[i] ? __builtin_nontemporal_load(bias_head + ei * ldb) : 0.0f;
        }
        if (has_bias && deal && em < wk.hi) bm = __builtin_nontemporal_load(bias_head + em * ldb);
        keeps(kp, dr, ent, uint32_t(em), pl, group);      // integer work under the loads above; its temporaries are gone before the gathers land
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
        // a -inf score weighs exactly 0, also while m is -inf itself; a NaN score, or +inf under m = +inf, gives NaN
        double w[kWideInFlight];
        if (deal) {      // lane i of each four forms entry i's score and weight, the four share the maximum, and the others fetch the weight
            const float tm = em < wk.hi ? score(scale, pick4(s, mine), bm, has_bias) : -INFINITY;
            float top = tm;
            top = fmaxf(top, __shfl_xor(top, 1, 64));      // NaN is never the maximum, in any order
            top = fmaxf(top, __shfl_xor(top, 2, 64));
            raise_to(st, fmaxf(st.m, top));
            const double wm = tm == -INFINITY ? 0.0 : exp(static_cast<double>(tm) - static_cast<double>(st.m));
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) w[i] = __shfl(wm, pl.first + int(i), 64);
        } else {
            float top = -INFINITY;
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                t[i] = ok[i] ? score(scale, s[i], b[i], has_bias) : -INFINITY;
                top = fmaxf(top, t[i]);
            }
            raise_to(st, fmaxf(st.m, top));
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) w[i] = t[i] == -INFINITY ? 0.0 : exp(static_cast<double>(t[i]) - static_cast<double>(st.m));
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            if (ok[i]) {
                const F8 x = widen(vv[i]);
                const double wv = kp[i] ? w[i] : 0.0;      // l takes every entry, the sums the kept ones
                st.l += w[i];
#pragma unroll
                for (uint32_t j = 0; j < kChunk; ++j) st.acc[j] += wv * static_cast<double>(x.x[j]);
            }
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void bf16_drop_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                        WideTable tab, const uint16_t* __restrict__ q, uint64_t ldq, const uint16_t* __restrict__ k, uint64_t ldk,
                                                                        const uint16_t* __restrict__ v, uint64_t ldv, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                        uint32_t d, uint32_t group, float scale, philox::Dropout dr, uint16_t* __restrict__ y, uint64_t ldy,
                                                                        float* __restrict__ lse, uint64_t ldl) {
    __shared__ double red[kWaves][kChunk][64];
    __shared__ double red_l[kWaves][64];      // per lane: a lane's l and m are its head's
    __shared__ float red_m[kWaves][64];
    const Place pl = place_of<kChunk>(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double c = dr.c;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const F8 qv = widen(load_chunk(q + uint64_t(wk.r) * ldq + pl.at));      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        attend_entries(st, idx, qv, pl, k + pl.at, ldk, v + pl.at, ldv, bias ? bias + pl.head : nullptr, ldb, scale, dr, wk, trips, group);
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
                    for (uint32_t j = 0; j < kChunk; ++j) out[j] = st.acc[j] / st.l * c;
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
                for (uint32_t j = 0; j < kChunk; ++j) out[j] = out[j] / l * c;
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
    bool kp[kWideInFlight];          // the keep decisions of the four entries for this lane's head
    uint32_t at[kWideInFlight];      // the gathered operands' row: idx[e], 0 for an entry past the end
    u32x4 a[kWideInFlight], b[kWideInFlight];
    double s[kWideInFlight], gp[kWideInFlight];
    // Where a head has fewer than kWideInFlight lanes: the bias word of this lane's head (0 past the end or without a bias) and the CSR
    // index of each entry (its own index on the row side, the map word on the column side).  Otherwise lane i of each four holds those of
    // entry i alone, in bm and mem, and okm = that entry exists.
    float bw[kWideInFlight];
    uint32_t me[kWideInFlight];
    float bm;
    uint32_t mem;
    bool okm;
    // column side only: lse and D of the entry's row and this lane's head
    float ls[kWideInFlight];
    double ds[kWideInFlight];
};

// s[i] = ha . A[at[i]], gp[i] = hb . B[at[i]] over the head's d elements, and kp[i]: an entry past the end gathers row 0 (in bounds, in
// the cache) without reading idx, the map or bias and is not added by the caller.  Row side (kPerEntry false): the entry's own index finds
// its bias word, a streamed load, and keys its draw.  Column side: the map word, streamed beside idx, does both, the bias word being a
// gather.  bias_head = bias + this lane's head (never dereferenced without a bias).
template <bool kPerEntry>
__device__ __forceinline__ void gather_dots(Trip& t, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm, uint64_t e, const Work& wk, const Place& pl, const F8& ha,
                                            const F8& hb, const uint16_t* __restrict__ a_chunk, uint64_t lda, const uint16_t* __restrict__ b_chunk, uint64_t ldb,
                                            const float* __restrict__ bias_head, uint64_t ldbias, const philox::Dropout& dr, const float* __restrict__ lse, uint64_t ldl,
                                            const double* __restrict__ dsum, uint64_t ldd, uint32_t group) {
    const bool has_bias = bias_head != nullptr;
    const bool deal = pl.head_lanes >= kWideInFlight;      // one map word, one bias word and one draw per lane and trip instead of four
    const uint64_t em = e + uint64_t(threadIdx.x & (kWideInFlight - 1u)) * wk.groups;
    t.okm = deal && em < wk.hi;
    t.bm = 0.0f;
    t.mem = kPerEntry ? 0u : uint32_t(em);
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        const uint64_t ei = e + uint64_t(i) * wk.groups;
        t.ok[i] = ei < wk.hi;
        t.at[i] = t.ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
        t.me[i] = kPerEntry ? 0u : uint32_t(ei);
        t.bw[i] = 0.0f;
        if (!deal && t.ok[i]) {
            if (kPerEntry) t.me[i] = __builtin_nontemporal_load(perm + ei);
            else if (has_bias) t.bw[i] = __builtin_nontemporal_load(bias_head + ei * ldbias);
        }
    }
    if (t.okm) {
        if (kPerEntry) t.mem = __builtin_nontemporal_load(perm + em);
        else if (has_bias) t.bm = __builtin_nontemporal_load(bias_head + em * ldbias);
    }
    keeps(t.kp, dr, t.me, t.mem, pl, group);      // integer work; its temporaries are gone before the gathers land
    if (kPerEntry && has_bias) {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) t.bw[i] = !deal && t.ok[i] ? bias_head[uint64_t(t.me[i]) * ldbias] : 0.0f;
        if (t.okm) t.bm = bias_head[uint64_t(t.mem) * ldbias];
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

// p[i] = exp(t[i] - lse_of(l[i])), the weight WITHOUT dropout, with t[i] the score as score() forms it, the rest double.  A -inf score
// under a finite lse weighs exactly 0 (exp(-inf)).  With at least kWideInFlight lanes in a head, lane i of it forms entry i's weight and
// the others fetch it.
__device__ __forceinline__ void weights(double (&p)[kWideInFlight], const double (&s)[kWideInFlight], const float (&b)[kWideInFlight], float bm, const float (&l)[kWideInFlight],
                                        float scale, bool has_bias, const Place& pl) {
    if (pl.head_lanes >= kWideInFlight) {
        const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
        const double pm = exp(static_cast<double>(score(scale, pick4(s, mine), bm, has_bias)) - lse_of(pick4(l, mine)));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = __shfl(pm, pl.first + int(i), 64);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = exp(static_cast<double>(score(scale, s[i], b[i], has_bias)) - lse_of(l[i]));
    }
}

// gQ's eight words of a lane from its sums a (0 ... 7) and b (8 ... 15) and its head's D
__device__ __forceinline__ void store_gq(uint16_t* dst, const double (&acc)[kSums], double dd, double sc) {
    double out[kChunk];
#pragma unroll
    for (uint32_t j = 0; j < kChunk; ++j) out[j] = sc * (acc[j] - dd * acc[kChunk + j]);
    store8(dst, out);
}

__global__ __launch_bounds__(kWideThreads) void bf16_drop_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                     WideTable tab, const uint16_t* __restrict__ q, uint64_t ldq, const uint16_t* __restrict__ k, uint64_t ldk,
                                                                     const uint16_t* __restrict__ v, uint64_t ldv, const uint16_t* __restrict__ gy, uint64_t ldgy,
                                                                     const float* __restrict__ lse, uint64_t ldl, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                     uint32_t d, uint32_t group, float scale, philox::Dropout dr, uint16_t* __restrict__ gq, uint64_t ldgq,
                                                                     double* __restrict__ dsum, uint64_t ldd) {
    __shared__ double red[kWaves][kSums][64];
    __shared__ double red_d[kWaves][64];      // per lane: a lane's D is its head's
    const Place pl = place_of<kChunk>(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale), c = dr.c;
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
            gather_dots<false>(t, idx, nullptr, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, qv, gyv, k + pl.at, ldk, v + pl.at, ldv,
                               bias ? bias + pl.head : nullptr, ldb, dr, nullptr, 0, nullptr, 0, group);
            double p[kWideInFlight];
            weights(p, t.s, t.bw, t.bm, ls, scale, bias != nullptr, pl);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double pg = p[i] * ((t.kp[i] ? c : 0.0) * t.gp[i]);      // P (w GP)
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

__global__ __launch_bounds__(kWideThreads) void bf16_drop_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                                     const uint32_t* __restrict__ list, WideTable tab, const uint16_t* __restrict__ q, uint64_t ldq,
                                                                     const uint16_t* __restrict__ k, uint64_t ldk, const uint16_t* __restrict__ v, uint64_t ldv,
                                                                     const uint16_t* __restrict__ gy, uint64_t ldgy, const float* __restrict__ lse, uint64_t ldl,
                                                                     const double* __restrict__ dsum, uint64_t ldd, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                     uint32_t d, uint32_t group, float scale, philox::Dropout dr, uint16_t* __restrict__ gk, uint64_t ldgk,
                                                                     uint16_t* __restrict__ gv, uint64_t ldgv, float* __restrict__ gbias, uint64_t ldgb) {
    __shared__ double red[kWaves][kSums][64];
    const Place pl = place_of<kChunk>(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale), c = dr.c;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const F8 kv = widen(load_chunk(k + uint64_t(wk.r) * ldk + pl.at));      // held for the whole column
        const F8 vv = widen(load_chunk(v + uint64_t(wk.r) * ldv + pl.at));
        double acc[kSums] = {};      // gK (0 ... 7) and gV (8 ... 15) of this lane's chunk
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<true>(t, idx, perm, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, kv, vv, q + pl.at, ldq, gy + pl.at, ldgy,
                              bias ? bias + pl.head : nullptr, ldb, dr, lse, ldl, dsum, ldd, group);
            double p[kWideInFlight], wt[kWideInFlight];
            weights(p, t.s, t.bw, t.bm, t.ls, scale, bias != nullptr, pl);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) wt[i] = t.kp[i] ? c : 0.0;
            if (gbias && t.okm && pl.deals) {      // lane i of the head's first four stores entry i's word: its one writer, the same p (w gp - D) as below
                const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
                gbias[uint64_t(t.mem) * ldgb + pl.head] = static_cast<float>(pick4(p, mine) * (pick4(wt, mine) * pick4(t.gp, mine) - pick4(t.ds, mine)));
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double gb = p[i] * (wt[i] * t.gp[i] - t.ds[i]), gs = sc * gb, pw = wt[i] * p[i];
                    if (gbias && pl.lead && pl.head_lanes < kWideInFlight) gbias[uint64_t(t.me[i]) * ldgb + pl.head] = static_cast<float>(gb);      // the entry's one writer per head
                    const F8 x = widen(t.a[i]), g = widen(t.b[i]);
#pragma unroll
                    for (uint32_t j = 0; j < kChunk; ++j) {
                        acc[j] += gs * static_cast<double>(x.x[j]);
                        acc[kChunk + j] += pw * static_cast<double>(g.x[j]);
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

hipError_t launch_bf16_drop_forward(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const float* bias,
                                    uint64_t ldb, uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr, uint16_t* y, uint64_t ldy, float* lse, uint64_t ldl,
                                    hipStream_t stream) {
    if (!shape_ok(heads, d, kChunk) || (bias && ldb < heads)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d / 2);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(bf16_drop_forward_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, bias, ldb, heads, d,
                       wide_group_lanes(heads * d / 2), scale, dr, y, ldy, lse, ldl);
    return hipGetLastError();
}

hipError_t launch_bf16_drop_rows(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                 uint64_t ldgy, const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr,
                                 uint16_t* gq, uint64_t ldgq, double* dsum, uint64_t ldd, hipStream_t stream) {
    if (!shape_ok(heads, d, kChunk) || ldd < heads || (bias && ldb < heads)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d / 2);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf16_drop_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, bias, ldb,
                       heads, d, wide_group_lanes(heads * d / 2), scale, dr, gq, ldgq, dsum, ldd);
    return hipGetLastError();
}

hipError_t launch_bf16_drop_cols(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                 uint64_t ldgy, const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d,
                                 float scale, const philox::Dropout& dr, uint16_t* gk, uint64_t ldgk, uint16_t* gv, uint64_t ldgv, float* gbias, uint64_t ldgb, hipStream_t stream) {
    if (!shape_ok(heads, d, kChunk) || ldd < heads || (bias && ldb < heads) || (gbias && ldgb < heads) || !s.perm) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d / 2);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf16_drop_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.perm, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, dsum,
                       ldd, bias, ldb, heads, d, wide_group_lanes(heads * d / 2), scale, dr, gk, ldgk, gv, ldgv, gbias, ldgb);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
