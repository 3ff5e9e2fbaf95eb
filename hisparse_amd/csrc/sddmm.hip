// sddmm.hip — the sampled dense product over a CSR pattern (include/hisparse_pattern.h): out[e] = sum_{j<k} U_j[row(e)] (x) V_j[col(e)].
// Three kernels:
//   expand_rows_kernel   create time: indptr -> row[e], one search of indptr per entry (empty rows anywhere, rows of any length, nnz = 0);
//   stage4_kernel        per call with k >= 2: k vectors -> [group][index][4] words, the interleaving spmm_sweep.hip uses for X, so that
//                        ONE 16-byte gather brings four vectors' words of a row or a column; the vectors beyond k of the last group are
//                        zero words in BOTH operands (padding products are 0 x 0, never 0 x inf);
//   sddmm_kernel         one pass over the entries whatever k is.  A lane takes four consecutive entries: one 16-byte load of row[] and
//                        one of col[] (streamed once: non-temporal), per group one 16-byte gather from U4[g][row] and one from V4[g][col]
//                        per entry (rows are sorted: the U gathers of neighbouring lanes hit the same lines; V is the scattered operand
//                        and lives in L2), four products into the entry's register accumulator -- a double, or a u64 clamped once at the
//                        end -- and one 16-byte store of four results (with accumulate, a 16-byte load of the old words first).
//                        Grid-stride, scalar tail for nnz mod 4.  No atomics (every word has one writer), no LDS, no scratch.
// Arithmetic: the header's ARITHMETIC block.  The products are spmv_device.h's (q8_24_mul / one fp32 multiply, -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "sddmm.h"
#include "spmv_device.h"

namespace hisparse {
namespace dev {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kExpandThreads = 256;
constexpr uint32_t kStageThreads = 256;

// the largest r with indptr[r] <= e: indptr[0] = 0 <= e < nnz = indptr[num_rows], so the answer is a row that holds e, and an empty
// row (indptr[r] == indptr[r + 1]) is never it
__global__ __launch_bounds__(kExpandThreads) void expand_rows_kernel(const uint32_t* __restrict__ indptr, uint32_t num_rows, uint64_t nnz, uint32_t* __restrict__ row) {
    const uint64_t stride = uint64_t(gridDim.x) * kExpandThreads;
    for (uint64_t e = uint64_t(blockIdx.x) * kExpandThreads + threadIdx.x; e < nnz; e += stride) {
        uint32_t lo = 0, hi = num_rows;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (indptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        row[e] = lo;
    }
}

// dst[g][i] = words i of vectors 4 g ... 4 g + 3 (zero beyond k); blockIdx.y = g
__global__ __launch_bounds__(kStageThreads) void stage4_kernel(const uint32_t* __restrict__ src, uint64_t ld, uint32_t k, uint32_t n, u32x4* __restrict__ dst) {
    const uint32_t i = blockIdx.x * kStageThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t j0 = blockIdx.y * 4u;
    u32x4 w;
    w.x = src[uint64_t(j0) * ld + i];
    w.y = j0 + 1u < k ? src[uint64_t(j0 + 1u) * ld + i] : 0u;
    w.z = j0 + 2u < k ? src[uint64_t(j0 + 2u) * ld + i] : 0u;
    w.w = j0 + 3u < k ? src[uint64_t(j0 + 3u) * ld + i] : 0u;
    dst[uint64_t(blockIdx.y) * n + i] = w;
}

template <bool kFixed>
struct Entry {
    using acc_t = typename std::conditional<kFixed, unsigned long long, double>::type;
    static __device__ __forceinline__ void add(acc_t& s, uint32_t a, uint32_t b) {
        if constexpr (kFixed) s += q8_24_mul(a, b);
        else s += static_cast<double>(__uint_as_float(a) * __uint_as_float(b));
    }
    static __device__ __forceinline__ void add4(acc_t& s, u32x4 a, u32x4 b) {      // ascending j
        add(s, a.x, b.x);
        add(s, a.y, b.y);
        add(s, a.z, b.z);
        add(s, a.w, b.w);
    }
    // fixed: at most 64 products and the old word, each below 2^32: no wrap before the one clamp
    template <bool kAcc>
    static __device__ __forceinline__ uint32_t finish(acc_t s, uint32_t old) {
        if constexpr (kFixed) {
            if (kAcc) s += old;
            return s > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(s);
        } else {
            float r = static_cast<float>(s);
            if (kAcc) r = __uint_as_float(old) + r;
            return __float_as_uint(r);
        }
    }
};

// kStaged: u / v are the staging buffers (u32x4 per index, `groups` groups of num_rows / num_cols); else the caller's single vectors
template <bool kFixed, bool kStaged, bool kAcc>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ col, uint64_t nnz,
                                                             const uint32_t* __restrict__ u, const uint32_t* __restrict__ v, uint32_t groups,
                                                             uint32_t num_rows, uint32_t num_cols, uint32_t* __restrict__ out) {
    using E = Entry<kFixed>;
    using acc_t = typename E::acc_t;
    const uint64_t stride = uint64_t(gridDim.x) * kSddmmThreads;
    const uint64_t t = uint64_t(blockIdx.x) * kSddmmThreads + threadIdx.x;
    const u32x4* u4 = reinterpret_cast<const u32x4*>(u);
    const u32x4* v4 = reinterpret_cast<const u32x4*>(v);
    const uint64_t quads = nnz / kSddmmEntriesPerLane;
    for (uint64_t q = t; q < quads; q += stride) {
        const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + q);
        const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(col) + q);
        acc_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        if constexpr (kStaged) {
            for (uint32_t g = 0; g < groups; ++g) {
                const u32x4* ug = u4 + uint64_t(g) * num_rows;
                const u32x4* vg = v4 + uint64_t(g) * num_cols;
                const u32x4 a0 = ug[r.x], a1 = ug[r.y], a2 = ug[r.z], a3 = ug[r.w];
                const u32x4 b0 = vg[c.x], b1 = vg[c.y], b2 = vg[c.z], b3 = vg[c.w];
                E::add4(s0, a0, b0);
                E::add4(s1, a1, b1);
                E::add4(s2, a2, b2);
                E::add4(s3, a3, b3);
            }
        } else {
            const uint32_t a0 = u[r.x], a1 = u[r.y], a2 = u[r.z], a3 = u[r.w];
            const uint32_t b0 = v[c.x], b1 = v[c.y], b2 = v[c.z], b3 = v[c.w];
            E::add(s0, a0, b0);
            E::add(s1, a1, b1);
            E::add(s2, a2, b2);
            E::add(s3, a3, b3);
        }
        u32x4* dst = reinterpret_cast<u32x4*>(out) + q;
        u32x4 old = {0u, 0u, 0u, 0u};
        if (kAcc) old = *dst;
        u32x4 res;
        res.x = E::template finish<kAcc>(s0, old.x);
        res.y = E::template finish<kAcc>(s1, old.y);
        res.z = E::template finish<kAcc>(s2, old.z);
        res.w = E::template finish<kAcc>(s3, old.w);
        *dst = res;
    }
    for (uint64_t e = quads * kSddmmEntriesPerLane + t; e < nnz; e += stride) {      // nnz mod 4 entries
        const uint32_t r = row[e], c = col[e];
        acc_t s = 0;
        if constexpr (kStaged) {
            for (uint32_t g = 0; g < groups; ++g) E::add4(s, u4[uint64_t(g) * num_rows + r], v4[uint64_t(g) * num_cols + c]);
        } else {
            E::add(s, u[r], v[c]);
        }
        out[e] = E::template finish<kAcc>(s, kAcc ? out[e] : 0u);
    }
}

template <bool kFixed, bool kStaged>
void launch_product(dim3 grid, hipStream_t stream, const SddmmLaunch& a, const uint32_t* u, const uint32_t* v, uint32_t groups) {
    if (a.accumulate) hipLaunchKernelGGL((sddmm_kernel<kFixed, kStaged, true>), grid, dim3(kSddmmThreads), 0, stream, a.row, a.col, a.nnz, u, v, groups, a.num_rows, a.num_cols, a.out);
    else hipLaunchKernelGGL((sddmm_kernel<kFixed, kStaged, false>), grid, dim3(kSddmmThreads), 0, stream, a.row, a.col, a.nnz, u, v, groups, a.num_rows, a.num_cols, a.out);
}

}  // namespace

hipError_t launch_expand_rows(const uint32_t* indptr, uint32_t num_rows, uint64_t nnz, uint32_t* row, uint32_t compute_units, hipStream_t stream) {
    if (nnz == 0) return hipSuccess;
    const uint64_t want = (nnz + kExpandThreads - 1) / kExpandThreads;
    const dim3 grid(uint32_t(std::min<uint64_t>(want, uint64_t(compute_units ? compute_units : 1) * kSddmmBlocksPerCu)));
    hipLaunchKernelGGL(expand_rows_kernel, grid, dim3(kExpandThreads), 0, stream, indptr, num_rows, nnz, row);
    return hipGetLastError();
}

hipError_t launch_sddmm(bool fixed, const SddmmLaunch& a, hipStream_t stream) {
    if (a.k == 0 || a.k > 64u || a.num_rows == 0 || a.num_cols == 0) return hipErrorInvalidValue;
    if (a.nnz == 0) return hipSuccess;
    const bool staged = a.k >= 2;
    const uint32_t groups = (a.k + 3u) / 4u;
    if (staged) {
        hipLaunchKernelGGL(stage4_kernel, dim3((a.num_rows + kStageThreads - 1) / kStageThreads, groups), dim3(kStageThreads), 0, stream, a.u, a.ldu, a.k, a.num_rows,
                           reinterpret_cast<u32x4*>(a.u4));
        hipLaunchKernelGGL(stage4_kernel, dim3((a.num_cols + kStageThreads - 1) / kStageThreads, groups), dim3(kStageThreads), 0, stream, a.v, a.ldv, a.k, a.num_cols,
                           reinterpret_cast<u32x4*>(a.v4));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint64_t lanes = (a.nnz + kSddmmEntriesPerLane - 1) / kSddmmEntriesPerLane;
    const uint64_t want = (lanes + kSddmmThreads - 1) / kSddmmThreads;
    const dim3 grid(uint32_t(std::min<uint64_t>(want, uint64_t(a.compute_units ? a.compute_units : 1) * kSddmmBlocksPerCu)));
    const uint32_t* u = staged ? a.u4 : a.u;
    const uint32_t* v = staged ? a.v4 : a.v;
    if (fixed) {
        if (staged) launch_product<true, true>(grid, stream, a, u, v, groups);
        else launch_product<true, false>(grid, stream, a, u, v, groups);
    } else {
        if (staged) launch_product<false, true>(grid, stream, a, u, v, groups);
        else launch_product<false, false>(grid, stream, a, u, v, groups);
    }
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
