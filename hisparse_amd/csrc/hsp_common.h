// hsp_common.h — what the two implementations of include/hisparse_pattern.h share (hsp_api.cpp on the HIP runtime, hsp_cpu.cpp on host
// threads): the limits and the argument / pattern checks, so that both refuse the same calls with the same codes.  Host code only.
#ifndef HISPARSE_HSP_COMMON_H_
#define HISPARSE_HSP_COMMON_H_

#include <cstdint>
#include <string>

#include "hisparse_hip.h"
#include "hisparse_pattern.h"

namespace hisparse {
namespace hsp {

constexpr uint32_t kMaxK = 64;       // vectors per call (accumulate = 1 for more)
constexpr uint32_t kGroup = 4;       // vectors per staging group: one 16-byte gather brings a row's / column's words of four vectors

inline uint64_t round_up4(uint64_t n) { return (n + 3u) & ~uint64_t(3); }

// hsp_create's arguments and the pattern itself; HS_OK or the code, with `why` set
inline int check_pattern(int impl, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_k, std::string& why) {
    if (impl != HS_IMPL_FIXED && impl != HS_IMPL_FLOAT_POB && impl != HS_IMPL_FLOAT_STALL) {
        why = "impl must be 0 (fixed), 1 (float_pob) or 2 (float_stall)";
        return HS_ERR_BAD_ARG;
    }
    if (max_k < 1 || max_k > kMaxK) {
        why = "max_k must be 1 ... 64 (wider batches: several calls with accumulate = 1)";
        return HS_ERR_BAD_ARG;
    }
    if (num_rows == 0 || num_cols == 0) {
        why = "empty matrix";
        return HS_ERR_BAD_ARG;
    }
    if (!indptr) {
        why = "null indptr";
        return HS_ERR_BAD_ARG;
    }
    if (indptr[0] != 0) {
        why = "indptr does not start at 0";
        return HS_ERR_BAD_MATRIX;
    }
    for (uint32_t r = 0; r < num_rows; ++r) {
        if (indptr[r + 1] < indptr[r]) {
            why = "indptr decreases at row " + std::to_string(r);
            return HS_ERR_BAD_MATRIX;
        }
    }
    const uint64_t nnz = indptr[num_rows];
    if (nnz && !indices) {
        why = "null indices";
        return HS_ERR_BAD_ARG;
    }
    for (uint64_t e = 0; e < nnz; ++e) {
        if (indices[e] >= num_cols) {
            why = "column index " + std::to_string(indices[e]) + " of entry " + std::to_string(e) + " is not below num_cols";
            return HS_ERR_BAD_MATRIX;
        }
    }
    return HS_OK;
}

// hsp_sddmm_device's arguments
inline int check_product(uint32_t num_rows, uint32_t num_cols, uint32_t max_k, const void* u, uint64_t ldu, const void* v, uint64_t ldv, uint32_t k,
                         const void* out, std::string& why) {
    if (!u || !v || !out) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (k < 1 || k > max_k) {
        why = "k must be 1 ... max_k (" + std::to_string(max_k) + ")";
        return HS_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(u) % 16 || reinterpret_cast<uintptr_t>(v) % 16 || reinterpret_cast<uintptr_t>(out) % 16) {
        why = "u, v and out must be 16-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    if (ldu % 4 || ldv % 4 || ldu < num_rows || ldv < num_cols) {
        why = "ldu and ldv must be multiples of 4 words with ldu >= num_rows and ldv >= num_cols";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

}  // namespace hsp
}  // namespace hisparse

#endif  // HISPARSE_HSP_COMMON_H_
