// gat_attention.hip — include/hisparse_gat.h's three kernels: the graph attention (GAT) step over a CSR pattern, all heads of a call in one
// pass, forward (ONE launch) and backward (TWO).  The score of an entry is additive, x[e][h] = el[row(e)][h] + er[col(e)][h] and
// t = LeakyReLU(x): there is no Q, no K and no dot in the forward, and per entry a lane gathers its 16 bytes of V[col(e)] and ONE word of er.
// The schedule, Place and Work, the online softmax State and the merges are wide_lanes.h's, the very definitions heads_attention.hip uses;
// this file owns `score_of`, `leaky`, `slope_at`, the trip loops written out in its three kernels, and their launchers.  What differs:
//   Forward: a lane reads its head's el word once per row; per trip the four gathers of V and the four one-word loads of er are issued
//     before the first use.  The lanes of a head load the same er word, so every lane forms x and t itself: no shuffle inside a head.
//   Row side of the backward: the row's gY chunk, el word and lse word stay in registers; the lanes of a head add the partial dots of
//     gY . V by shuffles, and every lane keeps three sums in double, D = sum P GP, A = sum P GP dx, B = sum P dx, which are the same in all
//     lanes of a head; gel = A - D B, stored by the head's first lane with the D word.
//   Column side, over the transposed pattern: the column's V chunk and er word stay in registers; per entry the row's gY chunk and its
//     el, lse and D words are gathered; five sums per lane, four of gV and one of ger.
//   Dead lanes form every address from head 0 and store nothing.
// x and t are one fp32 add and one fp32 multiply, spelled with __fadd_rn and __fmul_rn so that no build contracts them.  Every output
// word has one writer: no atomics, no scratch, no matrix engine, no inline assembly; LDS holds only the per-wavefront, per-lane sums of
// the long rows' merge.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gat_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

constexpr uint32_t kRowSums = 3;      // row side: D, A and B of this lane's head
constexpr uint32_t kColSums = 5;      // column side: gV of this lane's chunk (0 ... 3) and ger of its head (4)

// x = fl32(a + b): one fp32 add
__device__ __forceinline__ float score_of(float a, float b) { return __fadd_rn(a, b); }
// t = x > 0 ? x : fl32(slope * x): one fp32 multiply; x == 0 and a NaN take the slope branch
__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.0f ? x : __fmul_rn(slope, x); }
// dt / dx as torch's leaky_relu has it, at x == 0 too
__device__ __forceinline__ double slope_at(float x, float slope) { return x > 0.0f ? 1.0 : static_cast<double>(slope); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWideThreads) void gat_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, WideTable tab,
                                                                  const float* __restrict__ el, uint64_t ldel, const float* __restrict__ er, uint64_t lder,
                                                                  const float* __restrict__ v, uint64_t ldv, uint32_t heads, uint32_t d, uint32_t group, float slope,
                                                                  float* __restrict__ y, uint64_t ldy, float* __restrict__ lse, uint64_t ldl) {
    __shared__ double red[kWaves][4][64];
    __shared__ double red_l[kWaves][64];      // per lane: a lane's l and m are its head's
    __shared__ float red_m[kWaves][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ v_chunk = v + pl.at;
    const float* __restrict__ er_head = er + pl.head;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const float a = el[uint64_t(wk.r) * ldel + pl.head];      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0}};
        // the row's entries lo + g, lo + g + groups, ...: an entry past the end gathers row 0 of V and of er (in bounds, in the cache)
        // without reading idx, scores -inf and is not added
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t col[kWideInFlight];
            f32x4 vv[kWideInFlight];
            float b[kWideInFlight], t[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(v_chunk + uint64_t(col[i]) * ldv);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) b[i] = er_head[uint64_t(col[i]) * lder];
            float top = -INFINITY;
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                t[i] = ok[i] ? leaky(score_of(a, b[i]), slope) : -INFINITY;
                top = fmaxf(top, t[i]);
            }
            raise_to(st, fmaxf(st.m, top));
            // a -inf score weighs exactly 0, also while m is -inf itself; a NaN score, or +inf under m = +inf, gives NaN
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    const double wi = t[i] == -INFINITY ? 0.0 : exp(static_cast<double>(t[i]) - static_cast<double>(st.m));
                    st.l += wi;
                    st.acc.a += wi * static_cast<double>(vv[i].x);
                    st.acc.b += wi * static_cast<double>(vv[i].y);
                    st.acc.c += wi * static_cast<double>(vv[i].z);
                    st.acc.d += wi * static_cast<double>(vv[i].w);
                }
            }
        }
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
__global__ __launch_bounds__(kWideThreads) void gat_backward_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                        WideTable tab, const float* __restrict__ el, uint64_t ldel, const float* __restrict__ er, uint64_t lder,
                                                                        const float* __restrict__ v, uint64_t ldv, const float* __restrict__ gy, uint64_t ldgy,
                                                                        const float* __restrict__ lse, uint64_t ldl, uint32_t heads, uint32_t d, uint32_t group, float slope,
                                                                        float* __restrict__ gel, uint64_t ldgel, double* __restrict__ dsum, uint64_t ldd) {
    __shared__ double red[kWaves][kRowSums][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ v_chunk = v + pl.at;
    const float* __restrict__ er_head = er + pl.head;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 gyv = *reinterpret_cast<const f32x4*>(gy + uint64_t(wk.r) * ldgy + pl.at);      // held for the whole row
        const float a = el[uint64_t(wk.r) * ldel + pl.head];
        const double l = lse_of(lse[uint64_t(wk.r) * ldl + pl.head]);
        double acc[kRowSums] = {0.0, 0.0, 0.0};      // D, A and B of this lane's head, the same words in every lane of the head
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t col[kWideInFlight];
            f32x4 vv[kWideInFlight];
            float b[kWideInFlight];
            double gp[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(v_chunk + uint64_t(col[i]) * ldv);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) b[i] = er_head[uint64_t(col[i]) * lder];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) gp[i] = dot4(gyv, vv[i]);
            for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) gp[i] += __shfl_xor(gp[i], int(k), 64);
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    const float x = score_of(a, b[i]);
                    const double p = exp(static_cast<double>(leaky(x, slope)) - l);      // a -inf score under a finite lse weighs exactly 0
                    const double pg = p * gp[i], dx = slope_at(x, slope);
                    acc[0] += pg;
                    acc[1] += pg * dx;
                    acc[2] += p * dx;
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        float* dst = gel + uint64_t(wk.r) * ldgel + pl.head;
        double* dst_d = dsum + uint64_t(wk.r) * ldd + pl.head;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.lead) {
                if (wk.lo == wk.hi) {
                    *dst = 0.0f;
                    *dst_d = 0.0;
                } else {
                    *dst = static_cast<float>(acc[1] - acc[0] * acc[2]);
                    *dst_d = acc[0];
                }
            }
        } else {      // a long row: the four wavefronts' sums through LDS, lane by lane
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.lead) {
                *dst = static_cast<float>(acc[1] - acc[0] * acc[2]);
                *dst_d = acc[0];
            }
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
}

__global__ __launch_bounds__(kWideThreads) void gat_backward_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                        WideTable tab, const float* __restrict__ el, uint64_t ldel, const float* __restrict__ er, uint64_t lder,
                                                                        const float* __restrict__ v, uint64_t ldv, const float* __restrict__ gy, uint64_t ldgy,
                                                                        const float* __restrict__ lse, uint64_t ldl, const double* __restrict__ dsum, uint64_t ldd, uint32_t heads,
                                                                        uint32_t d, uint32_t group, float slope, float* __restrict__ ger, uint64_t ldger, float* __restrict__ gv,
                                                                        uint64_t ldgv) {
    __shared__ double red[kWaves][kColSums][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ gy_chunk = gy + pl.at;
    const float* __restrict__ el_head = el + pl.head;
    const float* __restrict__ lse_head = lse + pl.head;
    const double* __restrict__ d_head = dsum + pl.head;
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + uint64_t(wk.r) * ldv + pl.at);      // held for the whole column
        const float b = er[uint64_t(wk.r) * lder + pl.head];
        double acc[kColSums] = {0.0, 0.0, 0.0, 0.0, 0.0};      // gV of this lane's chunk (0 ... 3), ger of its head (4)
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t row[kWideInFlight];
            f32x4 g[kWideInFlight];
            float a[kWideInFlight], ls[kWideInFlight];
            double ds[kWideInFlight], gp[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                row[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) g[i] = *reinterpret_cast<const f32x4*>(gy_chunk + uint64_t(row[i]) * ldgy);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                a[i] = el_head[uint64_t(row[i]) * ldel];
                ls[i] = lse_head[uint64_t(row[i]) * ldl];
                ds[i] = d_head[uint64_t(row[i]) * ldd];
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) gp[i] = dot4(g[i], vv);
            for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) gp[i] += __shfl_xor(gp[i], int(k), 64);
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    const float x = score_of(a[i], b);
                    const double p = exp(static_cast<double>(leaky(x, slope)) - lse_of(ls[i]));
                    acc[0] += p * static_cast<double>(g[i].x);
                    acc[1] += p * static_cast<double>(g[i].y);
                    acc[2] += p * static_cast<double>(g[i].z);
                    acc[3] += p * static_cast<double>(g[i].w);
                    acc[4] += (p * (gp[i] - ds[i])) * slope_at(x, slope);
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        float* dst_v = gv + uint64_t(wk.r) * ldgv + pl.at;
        float* dst_r = ger + uint64_t(wk.r) * ldger + pl.head;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {      // a column without entries has summed nothing: +0.0
                store4(dst_v, acc[0], acc[1], acc[2], acc[3]);
                if (pl.lead) *dst_r = static_cast<float>(acc[4]);
            }
        } else {
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) {
                store4(dst_v, acc[0], acc[1], acc[2], acc[3]);
                if (pl.lead) *dst_r = static_cast<float>(acc[4]);
            }
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_gat_forward(const WideSide& s, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, uint32_t heads, uint32_t d, float slope,
                              float* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldel < heads || lder < heads || (lse && ldl < heads)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(gat_forward_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, el, ldel, er, lder, v, ldv, heads, d, wide_group_lanes(heads * d), slope, y,
                       ldy, lse, ldl);
    return hipGetLastError();
}

hipError_t launch_gat_backward_rows(const WideSide& s, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                    const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gel, uint64_t ldgel, double* dsum, uint64_t ldd,
                                    hipStream_t stream) {
    if (!shape_ok(heads, d) || ldel < heads || lder < heads || ldl < heads || ldgel < heads || ldd < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gat_backward_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, el, ldel, er, lder, v, ldv, gy, ldgy, lse, ldl, heads, d,
                       wide_group_lanes(heads * d), slope, gel, ldgel, dsum, ldd);
    return hipGetLastError();
}

hipError_t launch_gat_backward_cols(const WideSide& s, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                    const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float slope, float* ger, uint64_t ldger, float* gv,
                                    uint64_t ldgv, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldel < heads || lder < heads || ldl < heads || ldger < heads || ldd < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gat_backward_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, el, ldel, er, lder, v, ldv, gy, ldgy, lse, ldl, dsum, ldd, heads, d,
                       wide_group_lanes(heads * d), slope, ger, ldger, gv, ldgv);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
