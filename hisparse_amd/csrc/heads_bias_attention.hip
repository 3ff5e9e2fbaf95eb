// heads_bias_attention.hip — include/hisparse_heads_bias.h's three kernels: the multi-head attention step of heads_attention.hip with a
// per-entry, per-head additive bias, t[e][h] = (scale * s[e][h]) + bias[e][h], forward (ONE launch) and backward (TWO), and the gradient of
// the bias, gB[e][h] = P[e][h] (GP[e][h] - D[row(e)][h]), out of the column side.  bias and gbias are the caller's fp32 arrays stored
// [entry][head] in the CSR order of the pattern, rows of ldb and ldgb words.
// The schedule, Place and Work, the online softmax State and the merges are wide_lanes.h's, the very definitions heads_attention.hip
// uses; the dots inside a head and the dealing of a trip's weights follow that file's trip loops, so with every bias word +0.0 each sum
// is formed in the same order from the same words and the outputs are those kernels' bit for bit.  This file owns its trip loops
// (attend_entries; Trip, gather_dots, weights), `biased`, the three kernels and their launchers.  What is new:
//   Forward and row side: a lane knows its entry's index ei, and the lanes of a head read ONE address, bias[ei * ldb + head], as a
//     non-temporal load issued with the load of idx[ei], before the first use of the gathers.  An entry past the end loads nothing.
//   Column side: per transposed entry e' the map word perm[e'] (the entry's CSR index) is streamed beside idx[e'], the bias word is gathered
//     from bias[perm * ldb + head], and, where gbias is given, one lane of each head of the group that owns the entry stores
//     p (gp - D), formed in double and rounded once, to gbias[perm * ldgb + head]: the heads words of an entry are one contiguous piece.
//     gB comes from this side because D of a row is complete only after the row's last entry.
//   Where a head has at least kWideInFlight lanes (d >= 16) the dealing of a trip's weights extends to the bias: lane i of each four lanes
//     loads the map and bias word of the trip's entry i alone and forms that entry's score alone (the forward's four lanes share the
//     maximum by two shuffles), and lane i of the head's first four stores entry i's gbias word -- one load, one gather and one store per
//     lane and trip instead of four each.  A load instruction of a wavefront costs its 64 lanes whatever they fetch, and the four loads of
//     16 bytes each were what made the first version of these kernels 1.2 (forward) to 1.45 (backward) times the plain calls.
//   Dead lanes form every address from head 0, as before.
// t is two fp32 roundings, spelled with __fmul_rn and __fadd_rn so that no build contracts them.  Every output word, gbias included, has
// one writer: no atomics, no scratch, no matrix engine, no inline assembly, and no more LDS than heads_attention.hip's kernels declare.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "heads_bias_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

constexpr uint32_t kSums = 8;      // backward: double sums per lane that cross lanes, a and b of the row side, gK and gV of the column side

// t = fl32(fl32(scale * s) + b): one fp32 multiply, then one fp32 add
__device__ __forceinline__ float biased(float scale, double s, float b) { return __fadd_rn(__fmul_rn(scale, static_cast<float>(s)), b); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// One row's entries lo + g, lo + g + groups, ... through this lane's state.  Every lane of the wavefront makes `trips` trips; an entry
// past the end gathers row 0 of K and V (in bounds, in the cache) without reading idx or bias, scores -inf and is not added.  bias_head =
// bias + this lane's head.
__device__ __forceinline__ void attend_entries(State& st, const uint32_t* __restrict__ idx, f32x4 qv, const Place& pl, const float* __restrict__ k_chunk, uint64_t ldk,
                                               const float* __restrict__ v_chunk, uint64_t ldv, const float* __restrict__ bias_head, uint64_t ldb, float scale, const Work& wk,
                                               uint32_t trips) {
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
        bool ok[kWideInFlight];
        uint32_t col[kWideInFlight];
        f32x4 kv[kWideInFlight], vv[kWideInFlight];
        double s[kWideInFlight];
        float t[kWideInFlight], b[kWideInFlight];
        // Where a head has at least kWideInFlight lanes, lane i of each four forms the score and the weight of the trip's entry i alone and
        // loads that entry's bias word alone: one load per lane and trip instead of four.
        const bool deal = pl.head_lanes >= kWideInFlight;
        const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
        const uint64_t em = e + uint64_t(mine) * wk.groups;
        float bm = 0.0f;
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            const uint64_t ei = e + uint64_t(i) * wk.groups;
            ok[i] = ei < wk.hi;
            col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            b[i] = !deal && ok[i] ? __builtin_nontemporal_load(bias_head + ei * ldb) : 0.0f;
        }
        if (deal && em < wk.hi) bm = __builtin_nontemporal_load(bias_head + em * ldb);
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
            const float tm = em < wk.hi ? biased(scale, pick4(s, mine), bm) : -INFINITY;
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
                t[i] = ok[i] ? biased(scale, s[i], b[i]) : -INFINITY;
                top = fmaxf(top, t[i]);
            }
            raise_to(st, fmaxf(st.m, top));
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) w[i] = t[i] == -INFINITY ? 0.0 : exp(static_cast<double>(t[i]) - static_cast<double>(st.m));
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            if (ok[i]) {
                st.l += w[i];
                st.acc.a += w[i] * static_cast<double>(vv[i].x);
                st.acc.b += w[i] * static_cast<double>(vv[i].y);
                st.acc.c += w[i] * static_cast<double>(vv[i].z);
                st.acc.d += w[i] * static_cast<double>(vv[i].w);
            }
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void biased_attention_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx,
                                                                               const uint32_t* __restrict__ list, WideTable tab, const float* __restrict__ q, uint64_t ldq,
                                                                               const float* __restrict__ k, uint64_t ldk, const float* __restrict__ v, uint64_t ldv,
                                                                               const float* __restrict__ bias, uint64_t ldb, uint32_t heads, uint32_t d, uint32_t group, float scale,
                                                                               float* __restrict__ y, uint64_t ldy, float* __restrict__ lse, uint64_t ldl) {
    __shared__ double red[kWaves][4][64];
    __shared__ double red_l[kWaves][64];      // per lane: a lane's l and m are its head's
    __shared__ float red_m[kWaves][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 qv = *reinterpret_cast<const f32x4*>(q + uint64_t(wk.r) * ldq + pl.at);      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0}};
        attend_entries(st, idx, qv, pl, k + pl.at, ldk, v + pl.at, ldv, bias + pl.head, ldb, scale, wk, trips);
        merge_states(st, group, wk.team);
        float* dst = y + uint64_t(wk.r) * ldy + pl.at;
        float* dst_l = lse ? lse + uint64_t(wk.r) * ldl + pl.head : nullptr;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) store4(dst, 0.0, 0.0, 0.0, 0.0); else store4(dst, st.acc.a / st.l, st.acc.b / st.l, st.acc.c / st.l, st.acc.d / st.l);
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
                store4(dst, sum.acc.a / sum.l, sum.acc.b / sum.l, sum.acc.c / sum.l, sum.acc.d / sum.l);
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
    uint32_t at[kWideInFlight];      // the gathered operands' row: idx[e], 0 for an entry past the end
    f32x4 a[kWideInFlight], b[kWideInFlight];
    double s[kWideInFlight], gp[kWideInFlight];
    // Where a head has fewer than kWideInFlight lanes: the bias word of this lane's head (0 past the end) and, column side only, the CSR index
    // (the map word) of each entry.  Otherwise lane i of each four holds those of entry i alone, in bm and mem, and okm = that entry exists.
    float bw[kWideInFlight];
    uint32_t me[kWideInFlight];
    float bm;
    uint32_t mem;
    bool okm;
    // column side only: lse and D of the entry's row and this lane's head
    float ls[kWideInFlight];
    double ds[kWideInFlight];
};

// s[i] = ha . A[at[i]], gp[i] = hb . B[at[i]] over the head's d words: an entry past the end gathers row 0 (in bounds, in the cache) without
// reading idx, the map or bias and is not added by the caller.  Row side (kPerEntry false): the entry's own index finds its bias word, a
// streamed load.  Column side: the map word, streamed beside idx, finds it, a gather.  bias_head = bias + this lane's head.
template <bool kPerEntry>
__device__ __forceinline__ void gather_dots(Trip& t, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm, uint64_t e, const Work& wk, const Place& pl, f32x4 ha,
                                            f32x4 hb, const float* __restrict__ a_chunk, uint64_t lda, const float* __restrict__ b_chunk, uint64_t ldb,
                                            const float* __restrict__ bias_head, uint64_t ldbias, const float* __restrict__ lse, uint64_t ldl, const double* __restrict__ dsum,
                                            uint64_t ldd) {
    const bool deal = pl.head_lanes >= kWideInFlight;      // one map word and one bias word per lane and trip instead of four
    const uint64_t em = e + uint64_t(threadIdx.x & (kWideInFlight - 1u)) * wk.groups;
    t.okm = deal && em < wk.hi;
    t.bm = 0.0f;
    t.mem = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        const uint64_t ei = e + uint64_t(i) * wk.groups;
        t.ok[i] = ei < wk.hi;
        t.at[i] = t.ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
        t.me[i] = 0u;
        t.bw[i] = 0.0f;
        if (!deal && t.ok[i]) {
            if (kPerEntry) t.me[i] = __builtin_nontemporal_load(perm + ei);
            else t.bw[i] = __builtin_nontemporal_load(bias_head + ei * ldbias);
        }
    }
    if (t.okm) {
        if (kPerEntry) t.mem = __builtin_nontemporal_load(perm + em);
        else t.bm = __builtin_nontemporal_load(bias_head + em * ldbias);
    }
    if (kPerEntry) {
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

// p[i] = exp(t[i] - lse_of(l[i])) with t[i] = (scale * (float)s[i]) + b[i]: s rounded once, one fp32 multiply, one fp32 add, the rest double.
// A -inf score under a finite lse weighs exactly 0 (exp(-inf)).  With at least kWideInFlight lanes in a head, lane i of it forms entry
// i's weight and the others fetch it.
__device__ __forceinline__ void weights(double (&p)[kWideInFlight], const double (&s)[kWideInFlight], const float (&b)[kWideInFlight], float bm, const float (&l)[kWideInFlight],
                                        float scale, const Place& pl) {
    if (pl.head_lanes >= kWideInFlight) {
        const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
        const double sm = mine == 0u ? s[0] : mine == 1u ? s[1] : mine == 2u ? s[2] : s[3];
        const float lm = mine == 0u ? l[0] : mine == 1u ? l[1] : mine == 2u ? l[2] : l[3];
        const double pm = exp(static_cast<double>(biased(scale, sm, bm)) - lse_of(lm));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = __shfl(pm, pl.first + int(i), 64);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = exp(static_cast<double>(biased(scale, s[i], b[i])) - lse_of(l[i]));
    }
}

__global__ __launch_bounds__(kWideThreads) void biased_attention_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                            WideTable tab, const float* __restrict__ q, uint64_t ldq, const float* __restrict__ k, uint64_t ldk,
                                                                            const float* __restrict__ v, uint64_t ldv, const float* __restrict__ gy, uint64_t ldgy,
                                                                            const float* __restrict__ lse, uint64_t ldl, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                            uint32_t d, uint32_t group, float scale, float* __restrict__ gq, uint64_t ldgq, double* __restrict__ dsum,
                                                                            uint64_t ldd) {
    __shared__ double red[kWaves][kSums][64];
    __shared__ double red_d[kWaves][64];      // per lane: a lane's D is its head's
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale);
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
            gather_dots<false>(t, idx, nullptr, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, qv, gyv, k + pl.at, ldk, v + pl.at, ldv, bias + pl.head,
                               ldb, nullptr, 0, nullptr, 0);
            double p[kWideInFlight];
            weights(p, t.s, t.bw, t.bm, ls, scale, pl);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double pg = p[i] * t.gp[i];
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

__global__ __launch_bounds__(kWideThreads) void biased_attention_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                                            const uint32_t* __restrict__ list, WideTable tab, const float* __restrict__ q, uint64_t ldq,
                                                                            const float* __restrict__ k, uint64_t ldk, const float* __restrict__ v, uint64_t ldv,
                                                                            const float* __restrict__ gy, uint64_t ldgy, const float* __restrict__ lse, uint64_t ldl,
                                                                            const double* __restrict__ dsum, uint64_t ldd, const float* __restrict__ bias, uint64_t ldb, uint32_t heads,
                                                                            uint32_t d, uint32_t group, float scale, float* __restrict__ gk, uint64_t ldgk, float* __restrict__ gv,
                                                                            uint64_t ldgv, float* __restrict__ gbias, uint64_t ldgb) {
    __shared__ double red[kWaves][kSums][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale);
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const f32x4 kv = *reinterpret_cast<const f32x4*>(k + uint64_t(wk.r) * ldk + pl.at);      // held for the whole column
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + uint64_t(wk.r) * ldv + pl.at);
        double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // gK (0 ... 3) and gV (4 ... 7) of this lane's chunk
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<true>(t, idx, perm, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk, pl, kv, vv, q + pl.at, ldq, gy + pl.at, ldgy, bias + pl.head, ldb,
                              lse, ldl, dsum, ldd);
            double p[kWideInFlight];
            weights(p, t.s, t.bw, t.bm, t.ls, scale, pl);
            if (gbias && t.okm && pl.deals) {      // lane i of the head's first four stores entry i's word: its one writer, the same p (gp - D) as below
                const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
                gbias[uint64_t(t.mem) * ldgb + pl.head] = static_cast<float>(pick4(p, mine) * (pick4(t.gp, mine) - pick4(t.ds, mine)));
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double gb = p[i] * (t.gp[i] - t.ds[i]), gs = sc * gb;
                    if (gbias && pl.lead && pl.head_lanes < kWideInFlight) gbias[uint64_t(t.me[i]) * ldgb + pl.head] = static_cast<float>(gb);      // the entry's one writer per head
                    acc[0] += gs * static_cast<double>(t.a[i].x);
                    acc[1] += gs * static_cast<double>(t.a[i].y);
                    acc[2] += gs * static_cast<double>(t.a[i].z);
                    acc[3] += gs * static_cast<double>(t.a[i].w);
                    acc[4] += p[i] * static_cast<double>(t.b[i].x);
                    acc[5] += p[i] * static_cast<double>(t.b[i].y);
                    acc[6] += p[i] * static_cast<double>(t.b[i].z);
                    acc[7] += p[i] * static_cast<double>(t.b[i].w);
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

hipError_t launch_biased_forward(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* bias, uint64_t ldb,
                                 uint32_t heads, uint32_t d, float scale, float* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldb < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(biased_attention_forward_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, bias, ldb, heads, d,
                       wide_group_lanes(heads * d), scale, y, ldy, lse, ldl);
    return hipGetLastError();
}

hipError_t launch_biased_rows(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                              const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float* gq, uint64_t ldgq, double* dsum,
                              uint64_t ldd, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldd < heads || ldb < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(biased_attention_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, bias, ldb, heads, d,
                       wide_group_lanes(heads * d), scale, gq, ldgq, dsum, ldd);
    return hipGetLastError();
}

hipError_t launch_biased_cols(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                              const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float* gk,
                              uint64_t ldgk, float* gv, uint64_t ldgv, float* gbias, uint64_t ldgb, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldd < heads || ldb < heads || (gbias && ldgb < heads) || !s.perm) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(biased_attention_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.perm, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, dsum, ldd,
                       bias, ldb, heads, d, wide_group_lanes(heads * d), scale, gk, ldgk, gv, ldgv, gbias, ldgb);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
