// gatv2_attention.hip — include/hisparse_gatv2.h's four kernels: the GATv2 step over a CSR pattern, all heads of a call in one pass,
// forward (ONE launch) and backward (THREE).  The score of an entry is t[e][h] = a[h] . LeakyReLU(XD[row(e)][h] + XS[col(e)][h]), a d-term
// dot over a non-linearity of a sum of two rows, and the value is the same row XS[col(e)]: per entry a lane gathers its 16 bytes of
// XS[col(e)] and nothing else.  The schedule, Place and Work, the online softmax State and the merges are wide_lanes.h's, the very
// definitions heads_attention.hip uses; this file owns `sum_of`, `leaky`, `slope_at`, the trip loops written out in its kernels, and their
// launchers.
//   Forward: a's chunk is read once per lane and XD[r]'s once per row; per trip the four gathers of XS are issued before the first use,
//     every lane forms z and w of its chunk itself, and the d / 4 lanes of a head add the partial dots a . w by the shuffle tree of the
//     dot-product kernels.  The rest is hisparse_heads.h's online softmax.
//   Row side of the backward: the same single gather; two dots per entry, a . w and gY . XS.  Seventeen sums per lane in double: D of
//     its head, and for its four words A_j = sum P GP dz_j, B_j = sum P dz_j, A'_j = sum P GP w_j and B'_j = sum P w_j.  At the end of
//     a row gXD_j = a_j (A_j - D B_j), and A'_j - D B'_j, the row's share of ga_j, is added to four double sums that persist over the rows
//     the workgroup walks: the chunk a lane owns does not depend on the row.  At the end of the kernel the lanes of the same chunk are
//     added through LDS in a fixed order and the workgroup stores ONE vector of heads * d doubles, work[block][.].
//   Column side, over the transposed pattern: XS[c]'s and a's chunks stay in registers; per entry the row's gY and XD chunks and its lse
//     and D words are gathered; eight sums per lane, four of P gY_j and four of GT dz_j; gXS_j = the first + a_j times the second.
//   gatv2_reduce_kernel adds the workgroups' vectors in index order and rounds once: ga.
//   Dead lanes form every address from head 0 and store nothing.
// z and w are one fp32 add and one fp32 multiply, spelled with __fadd_rn and __fmul_rn so that no build contracts them.  Every output
// word has one writer: no atomics, no scratch, no matrix engine, no inline assembly; LDS holds only the per-wavefront, per-lane sums of
// the long rows' merge, which the row side uses once more for its ga sums.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "gatv2_attention.h"
#include "wide_lanes.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

constexpr uint32_t kRowSums = 17;      // row side: D (0), A_j (1 ... 4), B_j (5 ... 8), A'_j (9 ... 12), B'_j (13 ... 16)
constexpr uint32_t kColSums = 8;       // column side: sum P gY_j (0 ... 3), sum GT dz_j (4 ... 7)

// z = fl32(a + b): one fp32 add per word
__device__ __forceinline__ f32x4 sum_of(f32x4 a, f32x4 b) {
    f32x4 z = {__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)};
    return z;
}
// w = z > 0 ? z : fl32(slope * z): one fp32 multiply; z == 0 and a NaN take the slope branch
__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.0f ? z : __fmul_rn(slope, z); }
__device__ __forceinline__ f32x4 leaky(f32x4 z, float slope) {
    f32x4 w = {leaky(z.x, slope), leaky(z.y, slope), leaky(z.z, slope), leaky(z.w, slope)};
    return w;
}
// dw / dz as torch's leaky_relu has it, at z == 0 too
__device__ __forceinline__ double slope_at(float z, float slope) { return z > 0.0f ? 1.0 : static_cast<double>(slope); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWideThreads) void gatv2_forward_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, WideTable tab,
                                                                    const float* __restrict__ xd, uint64_t ldxd, const float* __restrict__ xs, uint64_t ldxs,
                                                                    const float* __restrict__ a, uint32_t heads, uint32_t d, uint32_t group, float slope, float* __restrict__ y,
                                                                    uint64_t ldy, float* __restrict__ lse, uint64_t ldl) {
    __shared__ double red[kWaves][4][64];
    __shared__ double red_l[kWaves][64];      // per lane: a lane's l and m are its head's
    __shared__ float red_m[kWaves][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ xs_chunk = xs + pl.at;
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + pl.at);      // held for the whole kernel: a lane's chunk does not depend on the row
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 xdv = *reinterpret_cast<const f32x4*>(xd + uint64_t(wk.r) * ldxd + pl.at);      // held for the whole row
        State st = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0}};
        // the row's entries lo + g, lo + g + groups, ...: an entry past the end gathers row 0 of XS (in bounds, in the cache) without
        // reading idx, scores -inf and is not added
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t col[kWideInFlight];
            f32x4 vv[kWideInFlight];
            double s[kWideInFlight];
            float t[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(xs_chunk + uint64_t(col[i]) * ldxs);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] = dot4(av, leaky(sum_of(xdv, vv[i]), slope));
            for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] += __shfl_xor(s[i], int(k), 64);
            }
            float top = -INFINITY;
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                t[i] = ok[i] ? static_cast<float>(s[i]) : -INFINITY;
                top = fmaxf(top, t[i]);
            }
            raise_to(st, fmaxf(st.m, top));
            // a -inf score weighs exactly 0, also while m is -inf itself; a NaN score, or +inf under m = +inf, gives NaN
            double wt[kWideInFlight];
            if (pl.head_lanes >= kWideInFlight) {      // one exp per lane: lane i of the head forms entry i's weight and the others fetch it
                const float tm = pick4(t, threadIdx.x & (kWideInFlight - 1u));
                const double wm = tm == -INFINITY ? 0.0 : exp(static_cast<double>(tm) - static_cast<double>(st.m));
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) wt[i] = __shfl(wm, pl.first + int(i), 64);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) wt[i] = t[i] == -INFINITY ? 0.0 : exp(static_cast<double>(t[i]) - static_cast<double>(st.m));
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    st.l += wt[i];
                    st.acc.a += wt[i] * static_cast<double>(vv[i].x);
                    st.acc.b += wt[i] * static_cast<double>(vv[i].y);
                    st.acc.c += wt[i] * static_cast<double>(vv[i].z);
                    st.acc.d += wt[i] * static_cast<double>(vv[i].w);
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
// the end of a row on the lane that stores it: gXD of its chunk, the head's D word, and the row's share of ga into the lane's own sums
__device__ __forceinline__ void finish_row(const double (&acc)[kRowSums], f32x4 av, bool lead, float* dst, double* dst_d, double (&ga)[4]) {
    store4(dst, static_cast<double>(av.x) * (acc[1] - acc[0] * acc[5]), static_cast<double>(av.y) * (acc[2] - acc[0] * acc[6]),
           static_cast<double>(av.z) * (acc[3] - acc[0] * acc[7]), static_cast<double>(av.w) * (acc[4] - acc[0] * acc[8]));
    if (lead) *dst_d = acc[0];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) ga[j] += acc[9 + j] - acc[0] * acc[13 + j];
}

__global__ __launch_bounds__(kWideThreads) void gatv2_backward_rows_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                          WideTable tab, const float* __restrict__ xd, uint64_t ldxd, const float* __restrict__ xs, uint64_t ldxs,
                                                                          const float* __restrict__ a, const float* __restrict__ gy, uint64_t ldgy, const float* __restrict__ lse,
                                                                          uint64_t ldl, uint32_t heads, uint32_t d, uint32_t group, float slope, float* __restrict__ gxd,
                                                                          uint64_t ldgxd, double* __restrict__ dsum, uint64_t ldd, double* __restrict__ work) {
    __shared__ double red[kWaves][kRowSums][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ xs_chunk = xs + pl.at;
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + pl.at);      // held for the whole kernel
    double ga[4] = {0.0, 0.0, 0.0, 0.0};                                // this lane's share of ga of its chunk, over every row it stores
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);
        const uint32_t trips = trips_of(wk);
        const f32x4 xdv = *reinterpret_cast<const f32x4*>(xd + uint64_t(wk.r) * ldxd + pl.at);      // held for the whole row
        const f32x4 gyv = *reinterpret_cast<const f32x4*>(gy + uint64_t(wk.r) * ldgy + pl.at);
        const double l = lse_of(lse[uint64_t(wk.r) * ldl + pl.head]);
        double acc[kRowSums];
#pragma unroll
        for (uint32_t j = 0; j < kRowSums; ++j) acc[j] = 0.0;
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t col[kWideInFlight];
            f32x4 vv[kWideInFlight];
            double s[kWideInFlight], gp[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                col[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(xs_chunk + uint64_t(col[i]) * ldxs);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                s[i] = dot4(av, leaky(sum_of(xdv, vv[i]), slope));
                gp[i] = dot4(gyv, vv[i]);
            }
            for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) {
                    s[i] += __shfl_xor(s[i], int(k), 64);
                    gp[i] += __shfl_xor(gp[i], int(k), 64);
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    const double p = exp(static_cast<double>(static_cast<float>(s[i])) - l);      // a -inf score under a finite lse weighs exactly 0
                    const double pg = p * gp[i];
                    const f32x4 z = sum_of(xdv, vv[i]);
                    const float zj[4] = {z.x, z.y, z.z, z.w};
                    acc[0] += pg;
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const double dz = slope_at(zj[j], slope), wj = static_cast<double>(leaky(zj[j], slope));
                        acc[1 + j] += pg * dz;
                        acc[5 + j] += p * dz;
                        acc[9 + j] += pg * wj;
                        acc[13 + j] += p * wj;
                    }
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        float* dst = gxd + uint64_t(wk.r) * ldgxd + pl.at;
        double* dst_d = dsum + uint64_t(wk.r) * ldd + pl.head;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) {      // a row without entries: +0.0 whatever a holds, and nothing for ga
                    store4(dst, 0.0, 0.0, 0.0, 0.0);
                    if (pl.lead) *dst_d = 0.0;
                } else {
                    finish_row(acc, av, pl.lead, dst, dst_d, ga);
                }
            }
        } else {      // a long row: the four wavefronts' sums through LDS, lane by lane
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) finish_row(acc, av, pl.lead, dst, dst_d, ga);
            __syncthreads();      // the LDS words are free for the workgroup's next long row
        }
    }
    // the workgroup's vector: the lanes that own the same chunk, wavefront by wavefront and lane by lane in ascending order
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) red[wave][j][lane] = ga[j];
    __syncthreads();
    if (wave == 0 && lane < group && pl.live) {
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t k2 = 0; k2 < kWaves; ++k2) {
            for (uint32_t l2 = lane; l2 < 64u; l2 += group) {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) sum[j] += red[k2][j][l2];
            }
        }
        double* dst_w = work + uint64_t(blockIdx.x) * (heads * d) + pl.at;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) dst_w[j] = sum[j];
    }
}

__global__ __launch_bounds__(kWideThreads) void gatv2_backward_cols_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list,
                                                                          WideTable tab, const float* __restrict__ xd, uint64_t ldxd, const float* __restrict__ xs, uint64_t ldxs,
                                                                          const float* __restrict__ a, const float* __restrict__ gy, uint64_t ldgy, const float* __restrict__ lse,
                                                                          uint64_t ldl, const double* __restrict__ dsum, uint64_t ldd, uint32_t heads, uint32_t d, uint32_t group,
                                                                          float slope, float* __restrict__ gxs, uint64_t ldgxs) {
    __shared__ double red[kWaves][kColSums][64];
    const Place pl = place_of(group, heads, d);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float* __restrict__ gy_chunk = gy + pl.at;
    const float* __restrict__ xd_chunk = xd + pl.at;
    const float* __restrict__ lse_head = lse + pl.head;
    const double* __restrict__ d_head = dsum + pl.head;
    const f32x4 av = *reinterpret_cast<const f32x4*>(a + pl.at);      // held for the whole kernel
    for (uint64_t w = blockIdx.x; w < tab.first[kWideClasses]; w += gridDim.x) {
        const Work wk = pick(tab, w, ptr, list, group);      // r is a column here, idx holds the rows of its entries
        const uint32_t trips = trips_of(wk);
        const f32x4 xsv = *reinterpret_cast<const f32x4*>(xs + uint64_t(wk.r) * ldxs + pl.at);      // held for the whole column
        double acc[kColSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t trip = 0; trip < trips; ++trip) {
            const uint64_t e = uint64_t(wk.lo) + uint64_t(trip) * kWideInFlight * wk.groups + wk.g;
            bool ok[kWideInFlight];
            uint32_t row[kWideInFlight];
            f32x4 g[kWideInFlight], x[kWideInFlight];
            float ls[kWideInFlight];
            double ds[kWideInFlight], s[kWideInFlight], gp[kWideInFlight];
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                const uint64_t ei = e + uint64_t(i) * wk.groups;
                ok[i] = ei < wk.hi;
                row[i] = ok[i] ? __builtin_nontemporal_load(idx + ei) : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) g[i] = *reinterpret_cast<const f32x4*>(gy_chunk + uint64_t(row[i]) * ldgy);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) x[i] = *reinterpret_cast<const f32x4*>(xd_chunk + uint64_t(row[i]) * ldxd);
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                ls[i] = lse_head[uint64_t(row[i]) * ldl];
                ds[i] = d_head[uint64_t(row[i]) * ldd];
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                s[i] = dot4(av, leaky(sum_of(x[i], xsv), slope));
                gp[i] = dot4(g[i], xsv);
            }
            for (uint32_t k = 1; k < pl.head_lanes; k <<= 1) {      // inside the head only
#pragma unroll
                for (uint32_t i = 0; i < kWideInFlight; ++i) {
                    s[i] += __shfl_xor(s[i], int(k), 64);
                    gp[i] += __shfl_xor(gp[i], int(k), 64);
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) {
                if (ok[i]) {
                    const double p = exp(static_cast<double>(static_cast<float>(s[i])) - lse_of(ls[i]));
                    const double gt = p * (gp[i] - ds[i]);
                    const f32x4 z = sum_of(x[i], xsv);
                    acc[0] += p * static_cast<double>(g[i].x);
                    acc[1] += p * static_cast<double>(g[i].y);
                    acc[2] += p * static_cast<double>(g[i].z);
                    acc[3] += p * static_cast<double>(g[i].w);
                    acc[4] += gt * slope_at(z.x, slope);
                    acc[5] += gt * slope_at(z.y, slope);
                    acc[6] += gt * slope_at(z.z, slope);
                    acc[7] += gt * slope_at(z.w, slope);
                }
            }
        }
        merge_lanes(acc, group, wk.team);
        float* dst = gxs + uint64_t(wk.r) * ldgxs + pl.at;
        if (wk.c != 0) {
            if (wk.mine && wk.g == 0 && pl.live) {
                if (wk.lo == wk.hi) {      // a column without entries: +0.0 whatever a holds
                    store4(dst, 0.0, 0.0, 0.0, 0.0);
                } else {
                    store4(dst, acc[0] + static_cast<double>(av.x) * acc[4], acc[1] + static_cast<double>(av.y) * acc[5], acc[2] + static_cast<double>(av.z) * acc[6],
                           acc[3] + static_cast<double>(av.w) * acc[7]);
                }
            }
        } else {
            merge_waves(red, acc, lane, wave, group);
            if (wave == 0 && lane < group && pl.live) {
                store4(dst, acc[0] + static_cast<double>(av.x) * acc[4], acc[1] + static_cast<double>(av.y) * acc[5], acc[2] + static_cast<double>(av.z) * acc[6],
                       acc[3] + static_cast<double>(av.w) * acc[7]);
            }
            __syncthreads();
        }
    }
}

// ga[k] = work[0][k] + work[1][k] + ... in index order, one rounding
__global__ __launch_bounds__(kWideThreads) void gatv2_reduce_kernel(const double* __restrict__ work, uint32_t vectors, uint32_t width, float* __restrict__ ga) {
    const uint32_t k = threadIdx.x;
    if (k < width) {
        double sum = 0.0;
#pragma unroll 8
        for (uint32_t v = 0; v < vectors; ++v) sum += work[uint64_t(v) * width + k];
        ga[k] = static_cast<float>(sum);
    }
}

}  // namespace

hipError_t launch_gatv2_forward(const WideSide& s, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, uint32_t heads, uint32_t d, float slope, float* y,
                                uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream) {
    if (!shape_ok(heads, d) || (lse && ldl < heads)) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;      // a side has at least one row, and an empty row is of class 1
    hipLaunchKernelGGL(gatv2_forward_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, xd, ldxd, xs, ldxs, a, heads, d,
                       wide_group_lanes(heads * d), slope, y, ldy, lse, ldl);
    return hipGetLastError();
}

uint32_t gatv2_row_vectors(const WideSide& s, uint32_t heads, uint32_t d) {
    if (!shape_ok(heads, d)) return 0;
    return grid_of(s, wide_table(s.count, heads * d), kWideBlocksPerCu).x;
}

hipError_t launch_gatv2_backward_rows(const WideSide& s, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, const float* gy, uint64_t ldgy, const float* lse,
                                      uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gxd, uint64_t ldgxd, double* dsum, uint64_t ldd, double* work, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldl < heads || ldd < heads || !work) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gatv2_backward_rows_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, xd, ldxd, xs, ldxs, a, gy, ldgy, lse, ldl, heads, d,
                       wide_group_lanes(heads * d), slope, gxd, ldgxd, dsum, ldd, work);
    return hipGetLastError();
}

hipError_t launch_gatv2_backward_cols(const WideSide& s, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, const float* gy, uint64_t ldgy, const float* lse,
                                      uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float slope, float* gxs, uint64_t ldgxs, hipStream_t stream) {
    if (!shape_ok(heads, d) || ldl < heads || ldd < heads) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, heads * d);
    if (t.first[kWideClasses] == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gatv2_backward_cols_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, xd, ldxd, xs, ldxs, a, gy, ldgy, lse, ldl, dsum, ldd,
                       heads, d, wide_group_lanes(heads * d), slope, gxs, ldgxs);
    return hipGetLastError();
}

hipError_t launch_gatv2_reduce(const double* work, uint32_t vectors, uint32_t width, float* ga, hipStream_t stream) {
    if (!work || !ga || vectors == 0 || width == 0 || width > kWideThreads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gatv2_reduce_kernel, dim3(1), dim3(kWideThreads), 0, stream, work, vectors, width, ga);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
