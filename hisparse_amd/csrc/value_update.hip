// value_update.hip — hs_update_values: new values for a loaded matrix, written into the image in place through the value map
// (gpu_tiles.h; option value_map).  The map holds, per non-zero in CSR order, the 32-bit word index its value word has in the image (and
// in the matrix-engine image of a float BITMAP matrix).  One pass streams the new values and the map(s) with 16-byte loads (four
// non-zeros per lane), converts each value with the load's own value_word() (value_word.h) and scatters 4-byte stores -- the image then
// holds the bytes a fresh load of the new values would build.  No atomics (every word has exactly one non-zero), no LDS, no scratch.
// Stream order does the rest: the SpMV launched next on the same stream sees the stores through the kernel-boundary release / acquire,
// as it sees the load's emit kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "spmv_kernels.h"
#include "value_word.h"

namespace hisparse {
namespace dev {
namespace {

constexpr uint32_t kUpdateThreads = 256;
constexpr uint32_t kUpdateBlocksPerCu = 8;      // 32 waves per CU in flight: enough stores outstanding to cover the scatter's latency

// a map entry past the image (0xffffffff: a non-zero the builder gave no word) is skipped: the image is the only thing written.
// Plain stores: the same kernel with the non-temporal hint on them took 1.85 ms on ogbl-ppa against 0.58 (profiles/value_update_times.txt)
__device__ __forceinline__ void put_word(uint32_t* __restrict__ image, uint64_t words, uint32_t at, uint32_t w) {
    if (at < words) image[at] = w;
}

// kVec: `values` is 16-byte aligned (the map always is: hipMalloc) -> four non-zeros per lane and load; else one.  kTwo: a second map /
// image (the matrix-engine image of a float BITMAP matrix).
template <bool kFixed, bool kVec, bool kTwo>
__global__ __launch_bounds__(kUpdateThreads) void value_update_kernel(const float* __restrict__ values, uint64_t n, const uint32_t* __restrict__ map,
                                                                     uint32_t* __restrict__ image, uint64_t image_words, const uint32_t* __restrict__ map2,
                                                                     uint32_t* __restrict__ image2, uint64_t image2_words) {
    const uint64_t stride = uint64_t(gridDim.x) * kUpdateThreads;
    const uint64_t t = uint64_t(blockIdx.x) * kUpdateThreads + threadIdx.x;
    uint64_t tail = 0;
    if (kVec) {
        const uint64_t quads = n / 4;
        const float4* v4 = reinterpret_cast<const float4*>(values);
        const uint4* m4 = reinterpret_cast<const uint4*>(map);
        const uint4* n4 = reinterpret_cast<const uint4*>(map2);
        for (uint64_t q = t; q < quads; q += stride) {
            const float4 v = v4[q];
            const uint4 m = m4[q];
            const uint32_t w0 = value_word(v.x, kFixed), w1 = value_word(v.y, kFixed), w2 = value_word(v.z, kFixed), w3 = value_word(v.w, kFixed);
            put_word(image, image_words, m.x, w0);
            put_word(image, image_words, m.y, w1);
            put_word(image, image_words, m.z, w2);
            put_word(image, image_words, m.w, w3);
            if (kTwo) {
                const uint4 m2 = n4[q];
                put_word(image2, image2_words, m2.x, w0);
                put_word(image2, image2_words, m2.y, w1);
                put_word(image2, image2_words, m2.z, w2);
                put_word(image2, image2_words, m2.w, w3);
            }
        }
        tail = quads * 4;
    }
    for (uint64_t e = tail + t; e < n; e += stride) {
        const uint32_t w = value_word(values[e], kFixed);
        put_word(image, image_words, map[e], w);
        if (kTwo) put_word(image2, image2_words, map2[e], w);
    }
}

template <bool kFixed, bool kVec>
void launch_one(dim3 grid, hipStream_t stream, const float* values, uint64_t n, const uint32_t* map, uint32_t* image, uint64_t image_words,
                const uint32_t* map2, uint32_t* image2, uint64_t image2_words) {
    if (map2) hipLaunchKernelGGL((value_update_kernel<kFixed, kVec, true>), grid, dim3(kUpdateThreads), 0, stream, values, n, map, image, image_words, map2, image2, image2_words);
    else hipLaunchKernelGGL((value_update_kernel<kFixed, kVec, false>), grid, dim3(kUpdateThreads), 0, stream, values, n, map, image, image_words, map2, image2, image2_words);
}

}  // namespace

hipError_t launch_value_update(bool fixed, const float* values, uint64_t n, const uint32_t* map, uint32_t* image, uint64_t image_words, const uint32_t* map2,
                               uint32_t* image2, uint64_t image2_words, uint32_t compute_units, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const bool vec = reinterpret_cast<uintptr_t>(values) % 16 == 0;
    const uint64_t lanes = vec ? (n + 3) / 4 : n;
    const uint64_t want = (lanes + kUpdateThreads - 1) / kUpdateThreads;
    const dim3 grid(uint32_t(std::min<uint64_t>(want, uint64_t(compute_units ? compute_units : 1) * kUpdateBlocksPerCu)));
    if (fixed) {
        if (vec) launch_one<true, true>(grid, stream, values, n, map, image, image_words, map2, image2, image2_words);
        else launch_one<true, false>(grid, stream, values, n, map, image, image_words, map2, image2, image2_words);
    } else {
        if (vec) launch_one<false, true>(grid, stream, values, n, map, image, image_words, map2, image2, image2_words);
        else launch_one<false, false>(grid, stream, values, n, map, image, image_words, map2, image2, image2_words);
    }
    return hipGetLastError();
}

}  // namespace dev
}  // namespace hisparse
