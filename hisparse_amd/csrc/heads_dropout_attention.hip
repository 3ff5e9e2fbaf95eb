// heads_dropout_attention.hip — include/hisparse_heads_dropout.h's three kernels: the multi-head attention step of heads_bias_attention.hip
// with DROPOUT ON THE ATTENTION WEIGHTS, P'[e][h] = keep(e, h) c P[e][h] with c = 1 / (1 - drop_p), forward (ONE launch) and backward (TWO),
// with or without the per-entry, per-head bias (a wave-uniform branch: without one no bias word is read and t = fl32(scale * s), the plain
// calls' score).  No mask is stored or read: keep(e, h) is recomputed wherever it is needed from the counter-based generator of philox.h,
// keyed by the call's seed, offset, the entry's index e IN THE CALLER'S CSR ORDER and the head.
// The schedule, Place and Work, the online softmax State and the merges are wide_lanes.h's, the very definitions heads_attention.hip and
// heads_bias_attention.hip use; the dots inside a head and the dealing of a trip's weights and of its bias words follow the latter's trip
// loops.  This file owns its trip loops (attend_entries; Trip, gather_dots, weights), `score`, `keeps`, the three kernels and their
// launchers.  What is new:
//   Forward and row side know the entry's index directly; the column side takes it from the map word perm[e'], which it streams anyway.
//   Where a head has at least kWideInFlight lanes (d >= 16) lane i of each four draws the Philox words of the trip's entry i alone, one
//     generator call per lane and trip, and the keep bits reach the head's lanes through ONE ballot of the wavefront: bit first + i is the
//     decision of entry i.  Below that width a lane draws for its four entries itself.  One draw serves four heads; lanes of different
//     heads of the same four recompute it.
//   Forward: l is summed over ALL entries of the row (lse is the words of the call without dropout) and the chunk's sums over the kept
//     ones (a dropped entry's weight is exactly 0, as a masked one's); c multiplies each output word once.  A row whose kept set is empty
//     in a head stores 0 / l * c = +0.0 there.
//   Backward: GP becomes w GP with w = keep ? c : 0 on both sides, and the column side weighs gV with w P; D, GS and gbias keep their form.
//   With drop_p = 0 every word is kept and c = 1.0, and x * 1.0 = x: every sum is formed in the same order from the same words, so the
//     outputs are heads_bias_attention.hip's (with a bias) or heads_attention.hip's (without) bit for bit.
// Every output word has one writer: no atomics, no scratch, no matrix engine, no inline assembly, and no more LDS than the kernels of
// heads_bias_attention.hip declare.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "heads_dropout_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

constexpr uint32_t kSums = 8;      // backward: double sums per lane that cross lanes, a and b of the row side, gK and gV of the column side

// t = fl32(fl32(scale * s) + b) with a bias: one fp32 multiply, then one fp32 add; t = fl32(scale * s) without
__device__ __forceinline__ float score(float scale, double s, float b, bool has_bias) {
    const float t = __fmul_rn(scale, static_cast<float>(s));
    return has_bias ? __fadd_rn(t, b) : t;
}

// The keep decisions of a trip's four entries for this lane's head.  ent[i] is entry i's index in the caller's CSR order and entm the one
// of the entry this lane deals (lane i of each four: entry i); an entry past the end carries index 0 or an index past the end, its draw
// reads no memory and its decision is never used.  With at least kWideInFlight lanes in a head each lane draws once and the wavefront
// shares the bits by one ballot (every lane of the wavefront is here: the trip loops are uniform); otherwise a lane draws four times.
__device__ __forceinline__ void keeps(bool (&kp)[kWideInFlight], const philox::Dropout& dr, const uint32_t (&ent)[kWideInFlight], uint32_t entm, const Place& pl) {
    if (pl.head_lanes >= kWideInFlight) {
        const uint64_t kept = __ballot(philox::keep(dr, entm, pl.head));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kp[i] = ((kept >> (uint32_t(pl.first) + i)) & 1u) != 0u;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kp[i] = philox::keep(dr, ent[i], pl.head);
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// One row's entries lo + g, lo + g + groups, ... through this lane's state: m and l over all entries, the four sums over the kept ones.
// Every lane of the wavefront makes `trips` trips; an entry past the end gathers row 0 of K and V (in bounds, in the cache) without reading
// idx or bias, scores -inf and is not added.  bias_head = bias + this lane's head (never dereferenced without a bias).
__device__ __forceinline__ void attend_entries(State& st, const uint32_t* __restrict__ idx, f32x4 qv, const Place& pl, const float* __restrict__ k_chunk, uint64_t ldk,
                                               const float* __restrict__ v_chunk, uint64_t ldv, const float* __restrict__ bias_head, uint64_t ldb, float scale,
                                               const philox::Dropout& dr, const Work& wk, uint32_t trips) {
    const bool has_bias = bias_head != nullptr;
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
        bool ok[kWideInFlight], kp[kWideInFlight];
        uint32_t col[kWideInFlight], ent[kWideInFlight];
        f32x4 kv[kWideInFlight], vv[kWideInFlight];
        double s[kWideInFlight];
        float t[kWideInFlight], b[kWideInFlight];
        // Where a head has at least kWideInFlight lanes, lane i of each four forms the score, the weight and the draw of the trip's entry i
        // alone and loads that entry's bias word alone: one load and one generator call per lane and trip instead of four.
        const bool deal = pl.head_lanes >= kWideInFlight;
        const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
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
        keeps(kp, dr, ent, uint32_t(em), pl);      // integer work under the loads above; its temporaries are gone before the gathers land
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kv[i] = *reinterpret_cast<const f32x4*>(k_chunk + uint64_t(col[i]) * ldk);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(v_chunk + uint64_t(col[i]) * ldv);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] = dot4(qv, kv[i]);
        for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] += __shfl_xor(s[i], int(k), 64);
        }
        // a -inf score weighs exactly 0, also while m is -inf itself; a NaN score, or +inf under m = +inf, gives NaN
        double w[kWideInFlight];
        if (deal) {      // one score and one exp per lane: lane i of each four forms entry i's, the four share the maximum, and the others fetch the weight
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
                const double wv = kp[i] ? w[i] : 0.0;      // l takes every entry, the sums the kept ones
                st.l += w[i];
                st.acc.a += wv * static_cast<double>(vv[i].x);
                st.acc.b += wv * static_cast<double>(vv[i].y);
                st.acc.c += wv * static_cast<double>(vv[i].z);
                st.acc.d += wv * static_cast<double>(vv[i].w);
            }
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void dropout_attention_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx,
                                                                                const uint32_t* __restrict__ list, WideTable tab, const float* __restrict__ q, uint64_t ldq,
                                                                                const float* __restrict__ k, uint64_t ldk, const float* __restrict__ v, uint64_t ldv,
                                                                                const float* __restrict__ bias, uint64_t ldb, uint32_t heads, uint32_t d, uint32_t group, float scale,
                                                                                philox::Dropout dr, float* __restrict__ y, uint64_t ldy, float* __restrict__ lse, uint64_t ldl) {
    __shared__ double red[kWaves][4][64];
    __shared__ double red_l[kWaves][64];      // per lane: a lane's l and m are its head's
    __shared__ float red_m[kWaves][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double c = dr.c;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 qv = *reinterpret_cast<const f32x4*>(q + uint64_t(wk.r) * ldq + pl.at);      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0}};
        attend_entries(st, idx, qv, pl, k + pl.at, ldk, v + pl.at, ldv, bias ? bias + pl.head : nullptr, ldb, scale, dr, wk, trips);
        merge_states(st, group, wk.team);
        float* dst = y + uint64_t(wk.r) * ldy + pl.at;
        float* dst_l = lse ? lse + uint64_t(wk.r) * ldl + pl.head : nullptr;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) store4(dst, 0.0, 0.0, 0.0, 0.0);
                else store4(dst, st.acc.a / st.l * c, st.acc.b / st.l * c, st.acc.c / st.l * c, st.acc.d / st.l * c);
                if (pl.lead && dst_l) *dst_l = wk.lo == wk.hi ? -INFINITY : static_cast<float>(static_cast<double>(st.m) + log(st.l));
            }
        } else {      // a long row: the four wavefronts' states through LDS, lane by lane
            if (lane < group) {
                red[wave][0][lane] = st.acc.a;
                red[wave][1][lane] = st.acc.b;
                red[wave][2][lane] = st.acc.c;
                red[wave][3][lane] = st.acc.d;
                red_l[wave][lane] = st.l;
                red_m[wave][lane] = st.m;
            }
            __syncthreads();
            if (wave == 0 && lane < group && pl.live) {
                const float m = fmaxf(fmaxf(red_m[0][lane], red_m[1][lane]), fmaxf(red_m[2][lane], red_m[3][lane]));
                State sum = {m, 0.0, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
                for (uint32_t k2 = 0; k2 < kWaves; ++k2) {
                    const double f = red_m[k2][lane] == m ? 1.0 : exp(static_cast<double>(red_m[k2][lane]) - static_cast<double>(m));
                    sum.l += f * red_l[k2][lane];
                    sum.acc.a += f * red[k2][0][lane];
                    sum.acc.b += f * red[k2][1][lane];
                    sum.acc.c += f * red[k2][2][lane];
                    sum.acc.d += f * red[k2][3][lane];
                }
                store4(dst, sum.acc.a / sum.l * c, sum.acc.b / sum.l * c, sum.acc.c / sum.l * c, sum.acc.d / sum.l * c);
                if (pl.lead && dst_l) *dst_l = static_cast<float>(static_cast<double>(m) + log(sum.l));
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
    f32x4 a[kWideInFlight], b[kWideInFlight];
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

// s[i] = ha . A[at[i]], gp[i] = hb . B[at[i]] over the head's d words, and kp[i]: an entry past the end gathers row 0 (in bounds, in the
// cache) without reading idx, the map or bias and is not added by the caller.  Row side (kPerEntry false): the entry's own index finds its
// bias word, a streamed load, and keys its draw.  Column side: the map word, streamed beside idx, does both, the bias word being a gather.
// bias_head = bias + this lane's head (never dereferenced without a bias).
template <bool kPerEntry>
__device__ __forceinline__ void gather_dots(Trip& t, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm, uint64_t e, const Work& wk, const Place& pl, f32x4 ha,
                                            f32x4 hb, const float* __restrict__ a_chunk, uint64_t lda, const float* __restrict__ b_chunk, uint64_t ldb,
                                            const float* __restrict__ bias_head, uint64_t ldbias, const philox::Dropout& dr, const float* __restrict__ lse, uint64_t ldl,
                                            const double* __restrict__ dsum, uint64_t ldd) {
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
    keeps(t.kp, dr, t.me, t.mem, pl);      // integer work; its temporaries are gone before the gathers land
    if (kPerEntry && has_bias) {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) t.bw[i] = !deal && t.ok[i] ? bias_head[uint64_t(t.me[i]) * ldbias] : 0.0f;
        if (t.okm) t.bm = bias_head[uint64_t(t.mem) * ldbias];
    }
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) t.a[i] = *reinterpret_cast<const f32x4*>(a_chunk + uint64_t(t.at[i]) * lda);
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) t.b[i] = *reinterpret_cast<const f32x4*>(b_chunk + uint64_t(t.at[i]) * ldb);
    if (kPerEntry) {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            t.ls[i] = lse[uint64_t(t.at[i]) * ldl + pl.head];
            t.ds[i] = dsum[uint64_t(t.at[i]) * ldd + pl.head];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        t.s[i] = dot4(ha, t.a[i]);
        t.gp[i] = dot4(hb, t.b[i]);
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
        const double sm = mine == 0u ? s[0] : mine == 1u ? s[1] : mine == 2u ? s[2] : s[3];
        const float lm = mine == 0u ? l[0] : mine == 1u ? l[1] : mine == 2u ? l[2] : l[3];
        const double pm = exp(static_cast<double>(score(scale, sm, bm, has_bias)) - lse_of(lm));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = __shfl(pm, pl.first + int(i), 64);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = exp(static_cast<double>(score(scale, s[i], b[i], has_bias)) - lse_of(l[i]));
    }
}

__global__ __launch_bounds__(kWideThreads) void dropout_attention_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                             WideTable tab, const float* __restrict__ q, uint64_t ldq, const float* __restrict__ k, uint64_t ldk,
                                                                             const float* __restrict__ v, uint64_t ldv, const float* __restrict__ gy, uint64_t ldgy,
                                                                             const float* __restrict__ lse, uint64_t ldl, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                             uint32_t d, uint32_t group, float scale, philox::Dropout dr, float* __restrict__ gq, uint64_t ldgq,
                                                                             double* __restrict__ dsum, uint64_t ldd) {
    __shared__ double red[kWaves][kSums][64];
    __shared__ double red_d[kWaves][64];      // per lane: a lane's D is its head's
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale), c = dr.c;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 qv = *reinterpret_cast<const f32x4*>(q + uint64_t(wk.r) * ldq + pl.at);      // held for the whole row
        const f32x4 gyv = *reinterpret_cast<const f32x4*>(gy + uint64_t(wk.r) * ldgy + pl.at);
        const float l = lse[uint64_t(wk.r) * ldl + pl.head];
        double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // a (0 ... 3) and b (4 ... 7) of this lane's chunk
        double dd = 0.0;
        const float ls[kWideInFlight] = {l, l, l, l};
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<false>(t, idx, nullptr, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, qv, gyv, k + pl.at, ldk, v + pl.at, ldv,
                               bias ? bias + pl.head : nullptr, ldb, dr, nullptr, 0, nullptr, 0);
            double p[kWideInFlight];
            weights(p, t.s, t.bw, t.bm, ls, scale, bias != nullptr, pl);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double pg = p[i] * ((t.kp[i] ? c : 0.0) * t.gp[i]);      // P (w GP)
                    dd += pg;
                    acc[0] += pg * static_cast<double>(t.a[i].x);
                    acc[1] += pg * static_cast<double>(t.a[i].y);
                    acc[2] += pg * static_cast<double>(t.a[i].z);
                    acc[3] += pg * static_cast<double>(t.a[i].w);
                    acc[4] += p[i] * static_cast<double>(t.a[i].x);
                    acc[5] += p[i] * static_cast<double>(t.a[i].y);
                    acc[6] += p[i] * static_cast<double>(t.a[i].z);
                    acc[7] += p[i] * static_cast<double>(t.a[i].w);
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        for (uint32_t k2 = group; k2 < wk.team; k2 <<= 1) dd += __shfl_xor(dd, int(k2), 64);
        float* dst = gq + uint64_t(wk.r) * ldgq + pl.at;
        double* dst_d = dsum + uint64_t(wk.r) * ldd + pl.head;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) {
                    store4(dst, 0.0, 0.0, 0.0, 0.0);
                    dd = 0.0;
                } else {
                    store4(dst, sc * (acc[0] - dd * acc[4]), sc * (acc[1] - dd * acc[5]), sc * (acc[2] - dd * acc[6]), sc * (acc[3] - dd * acc[7]));
                }
                if (pl.lead) *dst_d = dd;
            }
        } else {      // a long row: the four wavefronts' sums through LDS, lane by lane
            if (lane < group) red_d[wave][lane] = dd;
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) {
                dd = ((red_d[0][lane] + red_d[1][lane]) + red_d[2][lane]) + red_d[3][lane];
                store4(dst, sc * (acc[0] - dd * acc[4]), sc * (acc[1] - dd * acc[5]), sc * (acc[2] - dd * acc[6]), sc * (acc[3] - dd * acc[7]));
                if (pl.lead) *dst_d = dd;
            }
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void dropout_attention_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                                             const uint32_t* __restrict__ list, WideTable tab, const float* __restrict__ q, uint64_t ldq,
                                                                             const float* __restrict__ k, uint64_t ldk, const float* __restrict__ v, uint64_t ldv,
                                                                             const float* __restrict__ gy, uint64_t ldgy, const float* __restrict__ lse, uint64_t ldl,
                                                                             const double* __restrict__ dsum, uint64_t ldd, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                             uint32_t d, uint32_t group, float scale, philox::Dropout dr, float* __restrict__ gk, uint64_t ldgk,
                                                                             float* __restrict__ gv, uint64_t ldgv, float* __restrict__ gbias, uint64_t ldgb) {
    __shared__ double red[kWaves][kSums][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale), c = dr.c;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const f32x4 kv = *reinterpret_cast<const f32x4*>(k + uint64_t(wk.r) * ldk + pl.at);      // held for the whole column
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + uint64_t(wk.r) * ldv + pl.at);
        double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // gK (0 ... 3) and gV (4 ... 7) of this lane's chunk
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<true>(t, idx, perm, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, kv, vv, q + pl.at, ldq, gy + pl.at, ldgy,
                              bias ? bias + pl.head : nullptr, ldb, dr, lse, ldl, dsum, ldd);
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
                    acc[0] += gs * static_cast<double>(t.a[i].x);
                    acc[1] += gs * static_cast<double>(t.a[i].y);
                    acc[2] += gs * static_cast<double>(t.a[i].z);
                    acc[3] += gs * static_cast<double>(t.a[i].w);
                    acc[4] += pw * static_cast<double>(t.b[i].x);
                    acc[5] += pw * static_cast<double>(t.b[i].y);
                    acc[6] += pw * static_cast<double>(t.b[i].z);
                    acc[7] += pw * static_cast<double>(t.b[i].w);
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        float* dst_k = gk + uint64_t(wk.r) * ldgk + pl.at;
        float* dst_v = gv + uint64_t(wk.r) * ldgv + pl.at;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {      // a column without entries has summed nothing: +0.0
                store4(dst_k, acc[0], acc[1], acc[2], acc[3]);
                store4(dst_v, acc[4], acc[5], acc[6], acc[7]);
            }
        } else {
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) {
                store4(dst_k, acc[0], acc[1], acc[2], acc[3]);
                store4(dst_v, acc[4], acc[5], acc[6], acc[7]);
            }
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_dropout_forward(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* bias, uint64_t ldb,
                                  uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr, float* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream) {
    if (!shape_ok(heads, d) || (bias && ldb < heads)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(dropout_attention_forward_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, bias, ldb, heads, d, wide_group_lanes(heads * d), scale, dr,
                       y, ldy, lse, ldl);
    return hipGetLastError();
}

hipError_t launch_dropout_rows(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                               const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr, float* gq,
                               uint64_t ldgq, double* dsum, uint64_t ldd, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldd < heads || (bias && ldb < heads)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dropout_attention_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, bias, ldb, heads, d,
                       wide_group_lanes(heads * d), scale, dr, gq, ldgq, dsum, ldd);
    return hipGetLastError();
}

hipError_t launch_dropout_cols(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                               const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale,
                               const philox::Dropout& dr, float* gk, uint64_t ldgk, float* gv, uint64_t ldgv, float* gbias, uint64_t ldgb, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldd < heads || (bias && ldb < heads) || (gbias && ldgb < heads) || !s.perm) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dropout_attention_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.perm, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, dsum, ldd, bias, ldb, heads, d,
                       wide_group_lanes(heads * d), scale, dr, gk, ldgk, gv, ldgv, gbias, ldgb);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
