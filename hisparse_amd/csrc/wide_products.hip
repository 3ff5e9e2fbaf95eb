// wide_products.hip — the three products of include/hisparse_wide.h over a CSR pattern, with ROW-MAJOR dense operands ([index][feature],
// d <= 256 features).  Two kernels and ONE launch per call:
//   wide_dot_kernel      out[e] = sum_j U[row(e)][j] V[col(e)][j]                                      (hsw_sddmm_device)
//   wide_gather_kernel   Y[r][j] = sum_{e in row r} w[e] X[col(e)][j]                                  (hsw_spmm_device; with the transposed
//                        pattern and its map back to CSR order, kPerm, hsw_spmm_t_device)
// Work is scheduled by row (wide_products.h): hsw_create has sorted the rows into four classes by length and the host lays the classes
// out as ranges of virtual workgroups for the call's d; a workgroup strides over them and finds the class of each with scalar compares.
//   group   the lanes that cover one feature row, a 16-byte chunk each (lanes past ceil(d / 4) of a group whose size was rounded up to a
//           power of two gather chunk 0 again and their sums are never stored);
//   team    the groups that work on one row: they take different entries, kWideInFlight of them per trip, so every lane has that many
//           16-byte gathers in flight (each is an L2 / Infinity Cache round trip); short rows share a wavefront, team beside team, a row
//           of more than kWideLong entries has the whole workgroup.
// Sums are doubles in registers.  The gather kernel adds its groups' partial rows by lane shuffles and, for a long row, the four
// wavefronts' through 8 KiB of LDS; the dot kernel holds U's chunk in registers for the whole row, adds the lanes of a group by shuffles
// per entry and needs no LDS.  Every output word has one writer: no atomics, no scratch, no matrix engine, no inline assembly.
// Arithmetic: the header's ARITHMETIC block -- one fp32 multiply per product (-ffp-contract=off), added in double, rounded once.
// class_of, Sum4 and grid_of are wide_lanes.h's, the device side of this schedule that the attention kernels share.  These two kernels
// keep their own reading of a team's row (team_row: no trip count on the gather side), older than that header's pick.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "wide_lanes.h"
#include "wide_products.h"

namespace hisparse {
namespace dev {
namespace {

using namespace lanes;

__device__ __forceinline__ void add_row(Sum4& s, float w, f32x4 x) {
    s.a += static_cast<double>(w * x.x);
    s.b += static_cast<double>(w * x.y);
    s.c += static_cast<double>(w * x.z);
    s.d += static_cast<double>(w * x.w);
}

__device__ __forceinline__ void add_lane(Sum4& s, uint32_t mask) {
    s.a += __shfl_xor(s.a, int(mask), 64);
    s.b += __shfl_xor(s.b, int(mask), 64);
    s.c += __shfl_xor(s.c, int(mask), 64);
    s.d += __shfl_xor(s.d, int(mask), 64);
}

// the first `words` (1 ... 4) of a chunk: one 16-byte store, or narrower ones for the last chunk of a row with d % 4 != 0
__device__ __forceinline__ void store_chunk(float* dst, const Sum4& s, uint32_t words) {
    const float a = static_cast<float>(s.a), b = static_cast<float>(s.b), c = static_cast<float>(s.c), d = static_cast<float>(s.d);
    if (words >= 4u) {
        f32x4 v = {a, b, c, d};
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
        dst[0] = a;
        if (words >= 2u) dst[1] = b;
        if (words >= 3u) dst[2] = c;
    }
}

// The row of this lane's team in virtual workgroup w of class c: r, its entries [lo, hi) and whether there is one (a team past the end of
// its class's list runs on with no entries and stores nothing: every lane takes part in every shuffle).  team = lanes per team.
__device__ __forceinline__ bool team_row(const WideTable& t, uint32_t c, uint64_t w, uint32_t team, const uint32_t* ptr, const uint32_t* list, uint32_t& r,
                                         uint32_t& lo, uint32_t& hi) {
    const uint64_t slot = (w - t.first[c]) * (kWideThreads / team) + threadIdx.x / team;
    r = lo = hi = 0;
    if (slot >= t.off[c + 1] - t.off[c]) return false;
    r = list[t.off[c] + slot];
    lo = ptr[r];
    hi = ptr[r + 1];
    return true;
}

// this group's share of the row's entries: lo + g, lo + g + groups, ...; kWideInFlight entries per trip, the ones past the end read the
// trip's first entry again (an address that is in bounds and in the cache) and are not added
template <bool kPerm>
__device__ __forceinline__ void gather_entries(Sum4& s, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm, const float* __restrict__ w,
                                               const float* __restrict__ x_chunk, uint64_t ldx, uint32_t lo, uint32_t hi, uint32_t g, uint32_t groups) {
    for (uint64_t e = uint64_t(lo) + g; e < hi; e += uint64_t(kWideInFlight) * groups) {
        bool ok[kWideInFlight];
        uint32_t col[kWideInFlight];
        float wv[kWideInFlight];
        f32x4 xv[kWideInFlight];
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            const uint64_t ei = e + uint64_t(i) * groups;
            ok[i] = ei < hi;
            const uint64_t at = ok[i] ? ei : e;
            col[i] = __builtin_nontemporal_load(idx + at);
            wv[i] = kPerm ? w[perm[at]] : __builtin_nontemporal_load(w + at);
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) xv[i] = *reinterpret_cast<const f32x4*>(x_chunk + uint64_t(col[i]) * ldx);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i)
            if (ok[i]) add_row(s, wv[i], xv[i]);
    }
}

template <bool kPerm>
__global__ __launch_bounds__(kWideThreads) void wide_gather_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ perm,
                                                                  const uint32_t* __restrict__ list, WideTable t, const float* __restrict__ w, const float* __restrict__ x,
                                                                  uint64_t ldx, uint32_t d, uint32_t group, float* __restrict__ y, uint64_t ldy) {
    __shared__ double red[kWaves][4][64];
    const uint32_t chunk = threadIdx.x & (group - 1u);          // this lane's 16 bytes of a feature row
    const bool live = chunk * 4u < d;
    const uint32_t at = live ? chunk * 4u : 0u;
    const uint32_t words = live ? min(d - at, 4u) : 0u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t v = blockIdx.x; v < t.first[kWideClasses]; v += gridDim.x) {
        const uint32_t c = class_of(t, v);
        Sum4 s = {0.0, 0.0, 0.0, 0.0};
        if (c != 0) {
            const uint32_t team = min(group << (2u * c), 64u);
            uint32_t r, lo, hi;
            const bool mine = team_row(t, c, v, team, ptr, list, r, lo, hi);
            const uint32_t g = (threadIdx.x & (team - 1u)) / group;
            gather_entries<kPerm>(s, idx, perm, w, x + at, ldx, lo, hi, g, team / group);
            for (uint32_t m = group; m < team; m <<= 1) add_lane(s, m);
            if (mine && g == 0 && live) store_chunk(y + uint64_t(r) * ldy + at, s, words);
        } else {      // a long row: the whole workgroup
            const uint32_t r = list[t.off[0] + (v - t.first[0])];
            gather_entries<kPerm>(s, idx, perm, w, x + at, ldx, ptr[r], ptr[r + 1], threadIdx.x / group, kWideThreads / group);
            for (uint32_t m = group; m < 64u; m <<= 1) add_lane(s, m);
            if (lane < group) {
                red[wave][0][lane] = s.a;
                red[wave][1][lane] = s.b;
                red[wave][2][lane] = s.c;
                red[wave][3][lane] = s.d;
            }
            __syncthreads();
            if (wave == 0 && lane < group && live) {
                Sum4 sum;
                sum.a = (red[0][0][lane] + red[1][0][lane]) + (red[2][0][lane] + red[3][0][lane]);
                sum.b = (red[0][1][lane] + red[1][1][lane]) + (red[2][1][lane] + red[3][1][lane]);
                sum.c = (red[0][2][lane] + red[1][2][lane]) + (red[2][2][lane] + red[3][2][lane]);
                sum.d = (red[0][3][lane] + red[1][3][lane]) + (red[2][3][lane] + red[3][3][lane]);
                store_chunk(y + uint64_t(r) * ldy + at, sum, words);
            }
            __syncthreads();      // `red` is free for the workgroup's next long row
        }
    }
}

// One row of the dot kernel: every lane of the wavefront makes `trips` trips (the most any of its teams needs: the shuffles below stay
// convergent), a group takes entries lo + g, + groups, ...; the lanes of a group add their chunks' sums and the first one stores.
__device__ __forceinline__ void dot_entries(const uint32_t* __restrict__ idx, f32x4 u, uint32_t words, const float* __restrict__ v_chunk, uint64_t ldv, uint32_t lo, uint32_t hi,
                                            uint32_t g, uint32_t groups, uint32_t group, uint32_t chunk, uint32_t trips, float* __restrict__ out) {
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t e = uint64_t(lo) + uint64_t(trip) * kWideInFlight * groups + g;
        bool ok[kWideInFlight];
        uint32_t col[kWideInFlight];
        f32x4 vv[kWideInFlight];
        double s[kWideInFlight];
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            const uint64_t ei = e + uint64_t(i) * groups;
            ok[i] = ei < hi;
            col[i] = __builtin_nontemporal_load(idx + (ok[i] ? ei : 0u));      // entry 0 exists: a pattern without entries is not launched
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) vv[i] = *reinterpret_cast<const f32x4*>(v_chunk + uint64_t(col[i]) * ldv);
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i) {
            // words past d of the row's last chunk were loaded and are not used: a NaN there reaches nothing
            s[i] = words >= 1u ? static_cast<double>(u.x * vv[i].x) : 0.0;
            if (words >= 2u) s[i] += static_cast<double>(u.y * vv[i].y);
            if (words >= 3u) s[i] += static_cast<double>(u.z * vv[i].z);
            if (words >= 4u) s[i] += static_cast<double>(u.w * vv[i].w);
        }
        for (uint32_t m = 1; m < group; m <<= 1) {
#pragma unroll
            for (uint32_t i = 0; i < kWideInFlight; ++i) s[i] += __shfl_xor(s[i], int(m), 64);
        }
#pragma unroll
        for (uint32_t i = 0; i < kWideInFlight; ++i)
            if (ok[i] && chunk == 0) out[e + uint64_t(i) * groups] = static_cast<float>(s[i]);
    }
}

__global__ __launch_bounds__(kWideThreads) void wide_dot_kernel(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, WideTable t,
                                                               const float* __restrict__ u, uint64_t ldu, const float* __restrict__ v, uint64_t ldv, uint32_t d, uint32_t group,
                                                               float* __restrict__ out) {
    const uint32_t chunk = threadIdx.x & (group - 1u);
    const bool live = chunk * 4u < d;
    const uint32_t at = live ? chunk * 4u : 0u;
    const uint32_t words = live ? min(d - at, 4u) : 0u;
    for (uint64_t w = blockIdx.x; w < t.first[kWideClasses]; w += gridDim.x) {
        // pick and trips_of of wide_lanes.h written out (team_row): with the calls this kernel compiles to other code (tools/device_asm_digest.py)
        const uint32_t c = class_of(t, w);
        uint32_t r, lo, hi, g, groups;
        if (c != 0) {
            const uint32_t team = min(group << (2u * c), 64u);
            (void)team_row(t, c, w, team, ptr, list, r, lo, hi);
            g = (threadIdx.x & (team - 1u)) / group;
            groups = team / group;
        } else {
            r = list[t.off[0] + (w - t.first[0])];
            lo = ptr[r];
            hi = ptr[r + 1];
            g = threadIdx.x / group;
            groups = kWideThreads / group;
        }
        const uint32_t per_trip = kWideInFlight * groups;
        uint32_t trips = (hi - lo + per_trip - 1u) / per_trip;
#pragma unroll
        for (uint32_t m = 32; m; m >>= 1) trips = max(trips, uint32_t(__shfl_xor(int(trips), int(m), 64)));
        const f32x4 uv = *reinterpret_cast<const f32x4*>(u + uint64_t(r) * ldu + at);      // held for the whole row
        dot_entries(idx, uv, words, v + at, ldv, lo, hi, g, groups, group, chunk, trips, out);
    }
}

}  // namespace

hipError_t launch_wide_dot(const WideSide& s, const float* u, uint64_t ldu, const float* v, uint64_t ldv, uint32_t d, float* out, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (s.entries == 0) return hipSuccess;      // nothing to write
    hipLaunchKernelGGL(wide_dot_kernel, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.list, t, u, ldu, v, ldv, d, wide_group_lanes(d), out);
    return hipGetLastError();
}

hipError_t launch_wide_gather(const WideSide& s, const float* w, const float* x, uint64_t ldx, uint32_t d, float* y, uint64_t ldy, hipStream_t stream) {
    if (d == 0 || d > kWideMaxD) return hipErrorInvalidValue;
    const WideTable t = wide_table(s.count, d);
    if (t.first[kWideClasses] == 0) return hipSuccess;
    if (s.perm) hipLaunchKernelGGL(wide_gather_kernel<true>, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.perm, s.list, t, w, x, ldx, d, wide_group_lanes(d), y, ldy);
    else hipLaunchKernelGGL(wide_gather_kernel<false>, grid_of(s, t, kWideBlocksPerCu), dim3(kWideThreads), 0, stream, s.ptr, s.idx, s.perm, s.list, t, w, x, ldx, d, wide_group_lanes(d), y, ldy);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
