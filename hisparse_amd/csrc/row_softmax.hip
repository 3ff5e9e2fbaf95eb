// row_softmax.hip — the row softmax over a CSR pattern and its backward (include/hisparse_rows.h).  Two kernels, one per direction,
// and ONE launch per call: hsr_create has sorted the non-empty rows into six classes by length (row_softmax.h) and laid the classes out
// as ranges of virtual workgroups, the long rows first; a workgroup strides over the virtual workgroups, finds the class of each from the 16-word table with
// scalar compares (the index is uniform) and runs that class's template instance:
//   group<G>   G = 4 ... 64 lanes per row, n <= 4 G.  Lane j of the group holds entries j, j + G, j + 2 G, j + 3 G in registers (every
//              load and store of a group is one contiguous run), the row is read once and written once, max and sum go round the group
//              by __shfl_xor.  All 64 lanes take part in every shuffle: a group past the end of its class's list runs with n = 0.
//   long       n > 256: the whole workgroup on one row.  Passes max, sum, write (backward: sum, write) separated by workgroup barriers;
//              a wavefront reduces by shuffles, the four wavefronts through 32 bytes of LDS.  The first 1024 entries stay in registers,
//              the rest is read again in every pass (from L2 for any row that fits there).  A row never runs on one wavefront alone, and
//              a row of any length runs on one workgroup.
// No atomics (every output word has one writer), no scratch, no matrix engine, no inline assembly.  In place (p == s, gs == gp): an entry
// is read and written by the same lane, and a long row's barriers separate the last read of a pass from the first write.
// Arithmetic: the header's ARITHMETIC block.  expf is the device library's (-ffp-contract=off keeps scale * s and t - m apart).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "row_softmax.h"

namespace hisparse {
namespace dev {
namespace {

constexpr uint32_t kWaves = kRowsThreads / 64;
constexpr uint32_t kRegEntries = kRowsThreads * kRowsPerLane;      // a long row's entries held in registers

template <uint32_t G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (uint32_t m = G / 2; m; m >>= 1) v = fmaxf(v, __shfl_xor(v, int(m), 64));
    return v;
}

template <uint32_t G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (uint32_t m = G / 2; m; m >>= 1) v += __shfl_xor(v, int(m), 64);
    return v;
}

// over the workgroup; the second barrier frees `red` for the next reduction
__device__ __forceinline__ float block_max(float v, double* red) {
    v = group_max<64>(v);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = double(v);
    __syncthreads();
    const float r = fmaxf(fmaxf(float(red[0]), float(red[1])), fmaxf(float(red[2]), float(red[3])));
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}
static_assert(kWaves == 4, "block_max / block_sum read four words");

__device__ __forceinline__ float quotient(float e, double sum) { return static_cast<float>(static_cast<double>(e) / sum); }
__device__ __forceinline__ float gradient(float scale, float p, float g, double D) {
    return static_cast<float>((static_cast<double>(scale) * static_cast<double>(p)) * (static_cast<double>(g) - D));
}

// the row of this lane's group: entries [base, base + n), n = 0 past the end of the class's list
template <uint32_t G>
__device__ __forceinline__ void group_row(uint64_t first_slot, const uint32_t* list, uint32_t count, const uint32_t* indptr, uint64_t& base, uint32_t& n) {
    const uint64_t slot = first_slot + threadIdx.x / G;
    base = 0;
    n = 0;
    if (slot < count) {
        const uint32_t r = list[slot];
        base = indptr[r];
        n = indptr[r + 1] - indptr[r];
    }
}

template <uint32_t G>
__device__ __forceinline__ void forward_group(uint64_t first_slot, const uint32_t* list, uint32_t count, const uint32_t* indptr, const float* s, float scale, float* p) {
    uint64_t base;
    uint32_t n;
    group_row<G>(first_slot, list, count, indptr, base, n);
    const uint32_t j = threadIdx.x % G;
    const float* src = s + base;
    float* dst = p + base;
    float t[kRowsPerLane];
    float m = -__builtin_inff();
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = j + i * G;
        t[i] = idx < n ? scale * src[idx] : -__builtin_inff();
        m = fmaxf(m, t[i]);
    }
    m = group_max<G>(m);
    float e[kRowsPerLane];
    double sum = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        e[i] = expf(t[i] - m);
        if (j + i * G < n) sum += static_cast<double>(e[i]);
    }
    sum = group_sum<G>(sum);
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = j + i * G;
        if (idx < n) dst[idx] = quotient(e[i], sum);
    }
}

template <uint32_t G>
__device__ __forceinline__ void backward_group(uint64_t first_slot, const uint32_t* list, uint32_t count, const uint32_t* indptr, const float* p, const float* gp, float scale,
                                               float* gs) {
    uint64_t base;
    uint32_t n;
    group_row<G>(first_slot, list, count, indptr, base, n);
    const uint32_t j = threadIdx.x % G;
    float pv[kRowsPerLane], gv[kRowsPerLane];
    double D = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = j + i * G;
        pv[i] = gv[i] = 0.0f;
        if (idx < n) {
            pv[i] = p[base + idx];
            gv[i] = gp[base + idx];
            D += static_cast<double>(pv[i]) * static_cast<double>(gv[i]);
        }
    }
    D = group_sum<G>(D);
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = j + i * G;
        if (idx < n) gs[base + idx] = gradient(scale, pv[i], gv[i], D);
    }
}

__device__ __forceinline__ void forward_long(uint32_t r, const uint32_t* indptr, const float* s, float scale, float* p, double* red) {
    const uint64_t n = indptr[r + 1] - indptr[r];
    const float* src = s + indptr[r];
    float* dst = p + indptr[r];
    float t[kRowsPerLane];
    float m = -__builtin_inff();
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = threadIdx.x + i * kRowsThreads;
        t[i] = idx < n ? scale * src[idx] : -__builtin_inff();
        m = fmaxf(m, t[i]);
    }
    for (uint64_t idx = kRegEntries + threadIdx.x; idx < n; idx += kRowsThreads) m = fmaxf(m, scale * src[idx]);
    m = block_max(m, red);
    float e[kRowsPerLane];
    double sum = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        e[i] = expf(t[i] - m);
        if (threadIdx.x + i * kRowsThreads < n) sum += static_cast<double>(e[i]);
    }
    for (uint64_t idx = kRegEntries + threadIdx.x; idx < n; idx += kRowsThreads) sum += static_cast<double>(expf(scale * src[idx] - m));
    sum = block_sum(sum, red);      // its barriers: every read of this row is done before the first write (in place)
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = threadIdx.x + i * kRowsThreads;
        if (idx < n) dst[idx] = quotient(e[i], sum);
    }
    for (uint64_t idx = kRegEntries + threadIdx.x; idx < n; idx += kRowsThreads) dst[idx] = quotient(expf(scale * src[idx] - m), sum);
}

__device__ __forceinline__ void backward_long(uint32_t r, const uint32_t* indptr, const float* p, const float* gp, float scale, float* gs, double* red) {
    const uint64_t n = indptr[r + 1] - indptr[r];
    const float* ps = p + indptr[r];
    const float* gsrc = gp + indptr[r];
    float* dst = gs + indptr[r];
    float pv[kRowsPerLane], gv[kRowsPerLane];
    double D = 0.0;
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = threadIdx.x + i * kRowsThreads;
        pv[i] = gv[i] = 0.0f;
        if (idx < n) {
            pv[i] = ps[idx];
            gv[i] = gsrc[idx];
            D += static_cast<double>(pv[i]) * static_cast<double>(gv[i]);
        }
    }
    for (uint64_t idx = kRegEntries + threadIdx.x; idx < n; idx += kRowsThreads) D += static_cast<double>(ps[idx]) * static_cast<double>(gsrc[idx]);
    D = block_sum(D, red);
#pragma unroll
    for (uint32_t i = 0; i < kRowsPerLane; ++i) {
        const uint32_t idx = threadIdx.x + i * kRowsThreads;
        if (idx < n) dst[idx] = gradient(scale, pv[i], gv[i], D);
    }
    for (uint64_t idx = kRegEntries + threadIdx.x; idx < n; idx += kRowsThreads) dst[idx] = gradient(scale, ps[idx], gsrc[idx], D);
}

// forward: a = s, b unused, out = p.  backward: a = p, b = gp, out = gs.  `out` may be `a` (forward) or `b` (backward): no __restrict__.
template <bool kBackward>
__global__ __launch_bounds__(kRowsThreads) void row_softmax_kernel(const uint32_t* __restrict__ indptr, const uint32_t* __restrict__ list, const uint32_t* __restrict__ table,
                                                                  const float* a, const float* b, float scale, float* out) {
    __shared__ double red[kWaves];
    uint32_t first[kRowsClasses + 1], off[kRowsClasses + 1];
#pragma unroll
    for (uint32_t c = 0; c <= kRowsClasses; ++c) {
        first[c] = table[c];
        off[c] = table[8 + c];
    }
    for (uint64_t w = blockIdx.x; w < first[kRowsClasses]; w += gridDim.x) {
        // the class that holds w: first[] never decreases, and an empty class shares its first workgroup with the next one
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 1; k < kRowsClasses; ++k) c += w >= first[k] ? 1u : 0u;
#define HSR_GROUP(C)                                                                                                                    \
    case C: {                                                                                                                           \
        constexpr uint32_t G = 4u << (C - 1);                                                                                               \
        const uint64_t slot = (w - first[C]) * (kRowsThreads / G);                                                                      \
        if constexpr (kBackward) backward_group<G>(slot, list + off[C], off[C + 1] - off[C], indptr, a, b, scale, out);                 \
        else forward_group<G>(slot, list + off[C], off[C + 1] - off[C], indptr, a, scale, out);                                         \
        break;                                                                                                                          \
    }
        switch (c) {
            HSR_GROUP(1)
            HSR_GROUP(2)
            HSR_GROUP(3)
            HSR_GROUP(4)
            HSR_GROUP(5)
            default: {      // class 0: the long rows, laid out first so that they start first
                const uint32_t r = list[off[0] + (w - first[0])];
                if constexpr (kBackward) backward_long(r, indptr, a, b, scale, out, red);
                else forward_long(r, indptr, a, scale, out, red);
                break;
            }
        }
#undef HSR_GROUP
    }
}

dim3 grid_of(const RowSoftmaxLaunch& a) {
    return dim3(std::min<uint32_t>(a.workgroups, (a.compute_units ? a.compute_units : 1u) * kRowsBlocksPerCu));
}

}  // namespace

hipError_t launch_row_softmax(const RowSoftmaxLaunch& a, const float* s, float scale, float* p, hipStream_t stream) {
    if (a.workgroups == 0) return hipSuccess;      // nnz = 0
    hipLaunchKernelGGL(row_softmax_kernel<false>, grid_of(a), dim3(kRowsThreads), 0, stream, a.indptr, a.list, a.table, s, static_cast<const float*>(nullptr), scale, p);
    return hipGetLastError();
}

hipError_t launch_row_softmax_backward(const RowSoftmaxLaunch& a, const float* p, const float* gp, float scale, float* gs, hipStream_t stream) {
    if (a.workgroups == 0) return hipSuccess;
    hipLaunchKernelGGL(row_softmax_kernel<true>, grid_of(a), dim3(kRowsThreads), 0, stream, a.indptr, a.list, a.table, p, gp, scale, gs);
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
