// sddmm.h — launchers of the sampled dense product's kernels (sddmm.hip), called by hsp_api.cpp.
#ifndef HISPARSE_SDDMM_H_
#define HISPARSE_SDDMM_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace hisparse {
namespace dev {

// launch geometry of the product kernel (as value_update.hip): the grid never exceeds compute_units * kSddmmBlocksPerCu workgroups, every
// lane takes kSddmmEntriesPerLane consecutive entries per trip and strides from there.  hisparse_amd/pattern.py restates the three
// numbers (tests assert that a pattern is larger than one pass from them).
constexpr uint32_t kSddmmThreads = 256;
constexpr uint32_t kSddmmBlocksPerCu = 8;
constexpr uint32_t kSddmmEntriesPerLane = 4;

// row[e] = the row that holds entry e, for e < nnz = indptr[num_rows] (indptr in device memory)
hipError_t launch_expand_rows(const uint32_t* indptr, uint32_t num_rows, uint64_t nnz, uint32_t* row, uint32_t compute_units, hipStream_t stream);

struct SddmmLaunch {
    const uint32_t* row = nullptr;      // per entry, 16-byte aligned
    const uint32_t* col = nullptr;
    uint64_t nnz = 0;
    uint32_t num_rows = 0, num_cols = 0;
    const uint32_t* u = nullptr;        // U_j at u + j * ldu
    const uint32_t* v = nullptr;
    uint64_t ldu = 0, ldv = 0;
    uint32_t k = 0;
    uint32_t* u4 = nullptr;             // staging: ceil(k / 4) groups of num_rows x 4 words, and of num_cols x 4 words
    uint32_t* v4 = nullptr;
    uint32_t* out = nullptr;            // nnz words, 16-byte aligned
    bool accumulate = false;
    uint32_t compute_units = 0;
};
// staging (k >= 2) and the product, on `stream`
hipError_t launch_sddmm(bool fixed, const SddmmLaunch& a, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_SDDMM_H_
