// attention_backward.hip — include/hisparse_attention_backward.h's two kernels: from (Q, K, V, gY, lse) to (gQ, gK, gV) over a CSR pattern
// with ROW-MAJOR operands (d <= 256 features) and no per-entry array.  TWO launches per call, on one stream.
// Both use the schedule of wide_products.h, unchanged (groups that cover a feature row in 16-byte chunks, teams of groups by the length
// class, more than kWideLong entries on a whole workgroup and started first, a grid capped per CU that strides over the virtual
// workgroups).  Per entry both form the same two dots, s = Q[r] . K[c] and gp = gY[r] . V[c], and p = exp(scale * s - lse[r]):
//   attention_backward_rows_kernel, over the pattern: the row's chunks of Q and gY stay in registers; per trip a group gathers
//     kWideInFlight rows of K and as many of V before the first use and adds both dots over its lanes by shuffles in double.  ONE pass with
//     nine double sums per lane, a_j += p gp K_j, b_j += p K_j, D += p gp, then gQ_j = scale (a_j - D b_j): lse is known, so there is
//     no running maximum and no rescale.  It stores gQ and the row's D as a double (dsum);
//   attention_backward_cols_kernel, over the transposed pattern: the column's chunks of K and V stay in registers; per entry it gathers
//     Q[r] and gY[r], reads lse[r] and dsum[r], forms gs = scale p (gp - D_r) and adds gK_j += gs Q_j, gV_j += p gY_j.
//   Where a group has at least kWideInFlight lanes, lane i of it forms the weight of the trip's entry i and the others fetch it by a
//   shuffle: one exp per lane and trip.  The groups of a team merge by lane shuffles, a long row's (column's) four wavefronts through LDS.
// This file owns Trip, gather_dots, weights and store_chunk (a row of any d <= 256: the last chunk may hold fewer than four words), the two
// kernels and their launchers.  Which row a lane works on (pick, trips_of) and the merges (merge_lanes, merge_waves) are wide_lanes.h's.
// A row whose lse word is not finite has p = NaN in every entry: NaN in its gQ, its D and in gK and gV of every column it touches.
// Every output word has one writer: no atomics, no scratch, no matrix engine, no inline assembly.  Arithmetic: the header's ARITHMETIC
// block -- fp32 products added in double, s rounded once to fp32 and multiplied by scale in fp32, gp kept double, everything after that
// in double with the library's exp, one rounding per output word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "attention_backward.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

constexpr uint32_t kSums = 8;      // double sums per lane that cross lanes: a and b of the row side, gK and gV of the column side

// One trip of a group: kWideInFlight entries, their gathered chunks and their two dots (the same words in every lane of the group).
struct Trip {
    bool ok[kWideInFlight];
    uint32_t at[kWideInFlight];      // the gathered operands' row: idx[e], 0 for an entry past the end
    f32x4 a[kWideInFlight], b[kWideInFlight];
    double s[kWideInFlight], gp[kWideInFlight];
    float ls[kWideInFlight];         // column side only: lse and D of the entry's row
    double ds[kWideInFlight];
};

// s[i] = ha . A[at[i]], gp[i] = hb . B[at[i]] over the first d words: an entry past the end gathers row 0 (in bounds, in the cache) without
// reading idx and is not added by the caller.  Words past d of the last chunk were loaded and are not used: a NaN there reaches nothing.
template <bool kPerEntry>
__device__ __forceinline__ void gather_dots(Trip& t, const uint32_t* __restrict__ idx, uint64_t e, uint32_t hi, uint32_t groups, uint32_t group, uint32_t words, f32x4 ha, f32x4 hb,
                                            const float* __restrict__ a_chunk, uint64_t lda, const float* __restrict__ b_chunk, uint64_t ldb, const float* __restrict__ lse,
                                            const double* __restrict__ dsum) {
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        const uint64_t ei = e + uint64_t(i) * groups;
        t.ok[i] = ei < hi;
        t.at[i] = t.ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) t.a[i] = *reinterpret_cast<const f32x4*>(a_chunk + uint64_t(t.at[i]) * lda);
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) t.b[i] = *reinterpret_cast<const f32x4*>(b_chunk + uint64_t(t.at[i]) * ldb);
    if (kPerEntry) {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            t.ls[i] = lse[t.at[i]];
            t.ds[i] = dsum[t.at[i]];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kWideInFlight; ++i) {
        t.s[i] = words >= 1u ? static_cast<double>(ha.x * t.a[i].x) : 0.0;
        if (words >= 2u) t.s[i] += static_cast<double>(ha.y * t.a[i].y);
        if (words >= 3u) t.s[i] += static_cast<double>(ha.z * t.a[i].z);
        if (words >= 4u) t.s[i] += static_cast<double>(ha.w * t.a[i].w);
        t.gp[i] = words >= 1u ? static_cast<double>(hb.x * t.b[i].x) : 0.0;
        if (words >= 2u) t.gp[i] += static_cast<double>(hb.y * t.b[i].y);
        if (words >= 3u) t.gp[i] += static_cast<double>(hb.z * t.b[i].z);
        if (words >= 4u) t.gp[i] += static_cast<double>(hb.w * t.b[i].w);
    }
    for (uint32_t k = 1; k < group; k <<= 1) {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            t.s[i] += __shfl_xor(t.s[i], int(k), 64);
            t.gp[i] += __shfl_xor(t.gp[i], int(k), 64);
        }
    }
}

// p[i] = exp(scale * (float)s[i] - lse_of(l[i])): s rounded once, one fp32 multiply, the rest double.  A -inf score under a finite lse weighs
// exactly 0 (exp(-inf)).  With at least kWideInFlight lanes in a group, lane i forms entry i's weight and the others fetch it.
__device__ __forceinline__ void weights(double (&p)[kWideInFlight], const double (&s)[kWideInFlight], const float (&l)[kWideInFlight], float scale, uint32_t group) {
    if (group >= kWideInFlight) {
        const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
        const double sm = mine == 0u ? s[0] : mine == 1u ? s[1] : mine == 2u ? s[2] : s[3];
        const float lm = mine == 0u ? l[0] : mine == 1u ? l[1] : mine == 2u ? l[2] : l[3];
        const double pm = exp(static_cast<double>(scale * static_cast<float>(sm)) - lse_of(lm));
        const int first = int(threadIdx.x & 63u & ~(group - 1u));
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = __shfl(pm, first + int(i), 64);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) p[i] = exp(static_cast<double>(scale * static_cast<float>(s[i])) - lse_of(l[i]));
    }
}

// the first `words` (1 ... 4) of a chunk
__device__ __forceinline__ void store_chunk(float* dst, double x, double y, double z, double w, uint32_t words) {
    const float a = static_cast<float>(x), b = static_cast<float>(y), c = static_cast<float>(z), d = static_cast<float>(w);
    if (words >= 4u) {
        f32x4 v = {a, b, c, d};
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        dst[0] = a;
        if (words >= 2u) dst[1] = b;
        if (words >= 3u) dst[2] = c;
    }
}

__global__ __launch_bounds__(kWideThreads) void attention_backward_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                              WideTable tab, const float* __restrict__ q, uint64_t ldq, const float* __restrict__ k, uint64_t ldk,
                                                                              const float* __restrict__ v, uint64_t ldv, const float* __restrict__ gy, uint64_t ldgy,
                                                                              const float* __restrict__ lse, uint32_t d, uint32_t group, float scale, float* __restrict__ gq,
                                                                              uint64_t ldgq, double* __restrict__ dsum) {
    __shared__ double red[kWaves][kSums][64];
    __shared__ double red_d[kWaves];
    const uint32_t chunk = threadIdx.x & (group - 1u);          // this lane's 16 bytes of a feature row
    const bool live = chunk * 4u < d;
    const uint32_t at = live ? chunk * 4u : 0u;
    const uint32_t words = live ? min(d - at, 4u) : 0u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 qv = *reinterpret_cast<const f32x4*>(q + uint64_t(wk.r) * ldq + at);      // held for the whole row
        const f32x4 gyv = *reinterpret_cast<const f32x4*>(gy + uint64_t(wk.r) * ldgy + at);
        const float l = lse[wk.r];
        double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // a (0 ... 3) and b (4 ... 7) of this lane's chunk
        double dd = 0.0;
        const float ls[kWideInFlight] = {l, l, l, l};
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<false>(t, idx, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk.hi, wk.groups, group, words, qv, gyv, k + at, ldk, v + at, ldv,
                               nullptr, nullptr);
            double p[kWideInFlight];
            weights(p, t.s, ls, scale, group);
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
        float* dst = gq + uint64_t(wk.r) * ldgq + at;
        const double sc = static_cast<double>(scale);
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && live) {
                if (wk.lo == wk.hi) {
                    store_chunk(dst, 0.0, 0.0, 0.0, 0.0, words);
                    dd = 0.0;
                } else {
                    store_chunk(dst, sc * (acc[0] - dd * acc[4]), sc * (acc[1] - dd * acc[5]), sc * (acc[2] - dd * acc[6]), sc * (acc[3] - dd * acc[7]), words);
                }
                if (chunk == 0) dsum[wk.r] = dd;
            }
        } else {      // a long row: the four wavefronts' sums through LDS
            if (lane == 0) red_d[wave] = dd;
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && live) {
                dd = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
                store_chunk(dst, sc * (acc[0] - dd * acc[4]), sc * (acc[1] - dd * acc[5]), sc * (acc[2] - dd * acc[6]), sc * (acc[3] - dd * acc[7]), words);
                if (lane == 0) dsum[wk.r] = dd;
            }
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void attention_backward_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                              WideTable tab, const float* __restrict__ q, uint64_t ldq, const float* __restrict__ k, uint64_t ldk,
                                                                              const float* __restrict__ v, uint64_t ldv, const float* __restrict__ gy, uint64_t ldgy,
                                                                              const float* __restrict__ lse, const double* __restrict__ dsum, uint32_t d, uint32_t group, float scale,
                                                                              float* __restrict__ gk, uint64_t ldgk, float* __restrict__ gv, uint64_t ldgv) {
    __shared__ double red[kWaves][kSums][64];
    const uint32_t chunk = threadIdx.x & (group - 1u);
    const bool live = chunk * 4u < d;
    const uint32_t at = live ? chunk * 4u : 0u;
    const uint32_t words = live ? min(d - at, 4u) : 0u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const double sc = static_cast<double>(scale);
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const f32x4 kv = *reinterpret_cast<const f32x4*>(k + uint64_t(wk.r) * ldk + at);      // held for the whole column
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + uint64_t(wk.r) * ldv + at);
        double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // gK (0 ... 3) and gV (4 ... 7) of this lane's chunk
        for (uint32_t trip = 0; trip < trips; ++trip) {
            Trip t;
            gather_dots<true>(t, idx, uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g, wk.hi, wk.groups, group, words, kv, vv, q + at, ldq, gy + at, ldgy, lse,
                              dsum);
            double p[kWideInFlight];
            weights(p, t.s, t.ls, scale, group);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (t.ok[i]) {
                    const double gs = sc * (p[i] * (t.gp[i] - t.ds[i]));
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
        float* dst_k = gk + uint64_t(wk.r) * ldgk + at;
        float* dst_v = gv + uint64_t(wk.r) * ldgv + at;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && live) {      // a column without entries has summed nothing: +0.0
                store_chunk(dst_k, acc[0], acc[1], acc[2], acc[3], words);
                store_chunk(dst_v, acc[4], acc[5], acc[6], acc[7], words);
            }
        } else {
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && live) {
                store_chunk(dst_k, acc[0], acc[1], acc[2], acc[3], words);
                store_chunk(dst_v, acc[4], acc[5], acc[6], acc[7], words);
            }
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_attention_backward_rows(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                          const float* lse, uint32_t d, float scale, float* gq, uint64_t ldgq, double* dsum, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(attention_backward_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, d,
                       wide_group_lanes(d), scale, gq, ldgq, dsum);
    return hipGetLastError();
}

hipError_t launch_attention_backward_cols(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                          const float* lse, const double* dsum, uint32_t d, float scale, float* gk, uint64_t ldgk, float* gv, uint64_t ldgv, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_backward_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, dsum, d,
                       wide_group_lanes(d), scale, gk, ldgk, gv, ldgv);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
