// pattern_attention.hip — include/hisparse_attention.h's one kernel: per row of a CSR pattern the scores Q[r] . K[col(e)], their softmax and
// the weighted sum of the rows V[col(e)], with ROW-MAJOR operands (d <= 256 features) and no per-entry array.  ONE launch per call.
// The schedule is wide_products.h's, unchanged (groups that cover a feature row in 16-byte chunks, teams of groups by the row's length
// class, long rows on a whole workgroup and started first, a grid capped per CU that strides over the virtual workgroups).  Per row:
//   the row's chunk of Q stays in registers; per trip a group takes kWideInFlight entries and issues their gathers of K AND of V (16 bytes
//   each, 2 kWideInFlight per lane) before the first use; the lanes of a group add each entry's dot by shuffles in double, so every
//   lane of the group holds the same s, rounds it to fp32 and multiplies by scale;
//   the group keeps an online softmax state: m (the largest t so far, -inf at the start), l (the sum of the weights exp(t - m)) and the four
//   sums of w * V of its chunk, all double.  A trip raises m to the trip's maximum first and rescales l and the sums ONCE, by
//   exp(m_old - m_new), only when m has moved (while m is -inf nothing is formed from it: a weight of a -inf score is 0 by definition, never
//   exp(-inf - -inf)); where a group has at least kWideInFlight lanes, lane i of it forms the weight of the trip's entry i and the others
//   fetch it by a shuffle: one exp per lane and trip, not four, and the same words;
//   the groups of a team merge by lane shuffles -- the maximum first, then each group's rescaled sums are added -- and a long row's four
//   wavefronts through LDS (the 8 KiB of doubles of the gather kernel, plus m and l per wavefront).
// This file owns attend_entries, the stores of a last chunk of fewer than four words (a row of any d <= 256), the kernel and its launcher.
// The State with its raise_to and merge_states, and class_of, are wide_lanes.h's.  The kernel writes that header's pick and trips_of out
// in its own body, one of the two copies left beside the header (wide_dot_kernel has the other): with the calls it compiles to other
// code, and the header was made without moving any kernel's code.
// Every output word has one writer: no atomics, no scratch, no matrix engine, no inline assembly.  Arithmetic: the header's ARITHMETIC
// block -- fp32 products of Q and K added in double and rounded once, one fp32 multiply by scale, everything after that in double with
// the library's exp and log, one rounding per output word.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "pattern_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;      // State is one group's here: every lane of a group holds the same m and l

// the first `words` (1 ... 4) of a chunk of Y = acc / l
__device__ __forceinline__ void store_chunk(float* dst, const Sum4& s, double l, uint32_t words) {
    const float a = static_cast<float>(s.a / l), b = static_cast<float>(s.b / l), c = static_cast<float>(s.c / l), d = static_cast<float>(s.d / l);
    if (words >= 4u) {
        f32x4 v = {a, b, c, d};
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        dst[0] = a;
        if (words >= 2u) dst[1] = b;
        if (words >= 3u) dst[2] = c;
    }
}

__device__ __forceinline__ void store_zeros(float* dst, uint32_t words) {
    if (words >= 4u) {
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        dst[0] = 0.0f;
        if (words >= 2u) dst[1] = 0.0f;
        if (words >= 3u) dst[2] = 0.0f;
    }
}

// One row's entries lo + g, lo + g + groups, ... through this group's state.  Every lane of the wavefront makes `trips` trips (the most
// any of its teams needs: the shuffles stay convergent); an entry past the end gathers row 0 of K and V (in bounds, in the cache) without
// reading idx, scores -inf and is not added.
__device__ __forceinline__ void attend_entries(State& st, const uint32_t* __restrict__ idx, f32x4 qv, uint32_t words, const float* __restrict__ k_chunk, uint64_t ldk,
                                               const float* __restrict__ v_chunk, uint64_t ldv, float scale, uint32_t lo, uint32_t hi, uint32_t g, uint32_t groups, uint32_t group,
                                               uint32_t trips) {
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t e = uint64_t(lo) + uint64_t(trip) * kWideInFlight * groups + g;
        bool ok[kWideInFlight];
        uint32_t col[kWideInFlight];
        f32x4 kv[kWideInFlight], vv[kWideInFlight];
        double s[kWideInFlight];
        float t[kWideInFlight];
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            const uint64_t ei = e + uint64_t(i) * groups;
            ok[i] = ei < hi;
            col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) kv[i] = *reinterpret_cast<const f32x4*>(k_chunk + uint64_t(col[i]) * ldk);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(v_chunk + uint64_t(col[i]) * ldv);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            // words past d of the row's last chunk were loaded and are not used: a NaN there reaches nothing
            s[i] = words >= 1u ? static_cast<double>(qv.x * kv[i].x) : 0.0;
            if (words >= 2u) s[i] += static_cast<double>(qv.y * kv[i].y);
            if (words >= 3u) s[i] += static_cast<double>(qv.z * kv[i].z);
            if (words >= 4u) s[i] += static_cast<double>(qv.w * kv[i].w);
        }
        for (uint32_t k = 1; k < group; k <<= 1) {
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
        if (group >= kWideInFlight) {      // one exp per lane: lane i of the group forms entry i's weight and the others fetch it
            const uint32_t mine = threadIdx.x & (kWideInFlight - 1u);
            const float tm = mine == 0u ? t[0] : mine == 1u ? t[1] : mine == 2u ? t[2] : t[3];
            const double wm = tm == -INFINITY ? 0.0 : exp(static_cast<double>(tm) - static_cast<double>(st.m));
            const int first = int(threadIdx.x & 63u & ~(group - 1u));
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) w[i] = __shfl(wm, first + int(i), 64);
        } else {
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

__global__ __launch_bounds__(kWideThreads) void pattern_attention_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                        WideTable tab, const float* __restrict__ q, uint64_t ldq, const float* __restrict__ k, uint64_t ldk,
                                                                        const float* __restrict__ v, uint64_t ldv, uint32_t d, uint32_t group, float scale,
                                                                        float* __restrict__ y, uint64_t ldy, float* __restrict__ lse) {
    __shared__ double red[kWaves][4][64];
    __shared__ double red_l[kWaves];
    __shared__ float red_m[kWaves];
    const uint32_t chunk = threadIdx.x & (group - 1u);          // this lane's 16 bytes of a feature row
    const bool live = chunk * 4u < d;
    const uint32_t at = live ? chunk * 4u : 0u;
    const uint32_t words = live ? min(d - at, 4u) : 0u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        // pick and trips_of of wide_lanes.h written out: with the calls this kernel compiles to other code (tools/device_asm_digest.py)
        const uint32_t c = class_of(tab, w);
        uint32_t r = 0, lo = 0, hi = 0, g, groups, team = 64u;
        bool mine = true;
        if (c != 0) {
            team = min(group << (2u * c), 64u);
            const uint64_t slot = (w - tab.first[c]) * (kWideThreads / team) + threadIdx.x / team;
            mine = slot < tab.off[c + 1] - tab.off[c];      // a team past the end of its class's list runs on with no entries and stores nothing
            if (mine) {
                r = list[tab.off[c] + slot];
                lo = ptr[r];
                hi = ptr[r + 1];
            }
            g = (threadIdx.x & (team - 1u)) / group;
            groups = team / group;
        } else {
            r = list[tab.off[0] + (w - tab.first[0])];
            lo = ptr[r];
            hi = ptr[r + 1];
            g = threadIdx.x / group;
            groups = kWideThreads / group;
        }
        const uint32_t per_trip = kWideInFlight * groups;
        uint32_t trips = (hi - lo + per_trip - 1u) / per_trip;
#pragma unroll
        for (uint32_t k2 = 32; k2; k2 >>= 1) trips = max(trips, uint32_t(__shfl_xor(int(trips), int(k2), 64)));
        const f32x4 qv = *reinterpret_cast<const f32x4*>(q + uint64_t(r) * ldq + at);      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0}};
        attend_entries(st, idx, qv, words, k + at, ldk, v + at, ldv, scale, lo, hi, g, groups, group, trips);
        merge_states(st, group, team);
        float* dst = y + uint64_t(r) * ldy + at;
        if (c != 0) {
            if (mine && g == 0 && live) {
                if (lo == hi) store_zeros(dst, words); else store_chunk(dst, st.acc, st.l, words);
                if (chunk == 0 && lse) lse[r] = lo == hi ? -INFINITY : static_cast<float>(static_cast<double>(st.m) + log(st.l));
            }
        } else {      // a long row: the four wavefronts' states through LDS
            if (lane < group) {
                red[wave][0][lane] = st.acc.a;
                red[wave][1][lane] = st.acc.b;
                red[wave][2][lane] = st.acc.c;
                red[wave][3][lane] = st.acc.d;
            }
            if (lane == 0) {
                red_m[wave] = st.m;
                red_l[wave] = st.l;
            }
            __syncthreads();
            if (wave == 0 && lane < group && live) {
                const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
                State sum = {m, 0.0, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
                for (uint32_t k2 = 0; k2 < kWaves; ++k2) {
                    const double f = red_m[k2] == m ? 1.0 : exp(static_cast<double>(red_m[k2]) - static_cast<double>(m));
                    sum.l += f * red_l[k2];
                    sum.acc.a += f * red[k2][0][lane];
                    sum.acc.b += f * red[k2][1][lane];
                    sum.acc.c += f * red[k2][2][lane];
                    sum.acc.d += f * red[k2][3][lane];
                }
                store_chunk(dst, sum.acc, sum.l, words);
                if (lane == 0 && lse) lse[r] = static_cast<float>(static_cast<double>(m) + log(sum.l));
            }
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
}

}  // namespace

hipError_t launch_pattern_attention(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, uint32_t d, float scale, float* y,
                                    uint64_t ldy, float* lse, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (t.first[kWideClasses] == 0) return hipSuccess;
    hipLaunchKernelGGL(pattern_attention_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, q, ldq, k, ldk, v, ldv, d, wide_group_lanes(d), scale, y, ldy, lse);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
