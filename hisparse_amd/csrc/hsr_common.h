// hsr_common.h — what the two implementations of include/hisparse_rows.h share (hsr_api.cpp on the HIP runtime, hsr_cpu.cpp on host
// threads): the indptr check and the argument checks, so that both refuse the same calls with the same codes.  Host code only.
#ifndef HISPARSE_HSR_COMMON_H_
#define HISPARSE_HSR_COMMON_H_

#include <cmath>
#include <cstdint>
#include <string>

#include "hisparse_hip.h"
#include "hisparse_rows.h"

namespace hisparse {
namespace hsr {

// hsr_create's arguments and indptr itself; HS_OK or the code, with `why` set
inline int check_rows(uint32_t num_rows, const uint32_t* indptr, std::string& why) {
    if (num_rows == 0) {
        why = "no rows";
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
    return HS_OK;
}

// the ranges [a, a + bytes) and [b, b + bytes) share a byte
inline bool overlap(const void* a, const void* b, uint64_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

inline bool misaligned(const void* a) { return reinterpret_cast<uintptr_t>(a) % 4 != 0; }

// hsr_softmax_device's arguments (`device` = the alignment rule applies; the host forms copy)
inline int check_forward(uint64_t nnz, const float* s, float scale, const float* p, bool device, std::string& why) {
    if (!s || !p) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (device && (misaligned(s) || misaligned(p))) {
        why = "s and p must be 4-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    if (!std::isfinite(scale)) {
        why = "scale must be finite";
        return HS_ERR_BAD_ARG;
    }
    if (p != s && overlap(s, p, nnz * 4)) {
        why = "p overlaps s without being s (in place means the same pointer)";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsr_softmax_backward_device's arguments
inline int check_backward(uint64_t nnz, const float* p, const float* gp, float scale, const float* gs, bool device, std::string& why) {
    if (!p || !gp || !gs) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (device && (misaligned(p) || misaligned(gp) || misaligned(gs))) {
        why = "p, gp and gs must be 4-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    if (!std::isfinite(scale)) {
        why = "scale must be finite";
        return HS_ERR_BAD_ARG;
    }
    if (overlap(p, gs, nnz * 4)) {
        why = "gs overlaps p";
        return HS_ERR_BAD_ARG;
    }
    if (gs != gp && overlap(gp, gs, nnz * 4)) {
        why = "gs overlaps gp without being gp (in place means the same pointer)";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

}  // namespace hsr
}  // namespace hisparse

#endif  // HISPARSE_HSR_COMMON_H_
