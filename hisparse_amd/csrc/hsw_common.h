// hsw_common.h — what the two implementations of include/hisparse_wide.h share (hsw_api.cpp on the HIP runtime, hsw_cpu.cpp on the host):
// the limits, the argument checks, so that both refuse the same calls with the same codes, and the counting sort that builds the
// transposed pattern.  The pattern check itself is hsp_common.h's, the one hsp_create applies.  Host code only.
#ifndef HISPARSE_HSW_COMMON_H_
#define HISPARSE_HSW_COMMON_H_

#include <cstdint>
#include <string>
#include <vector>

#include "hisparse_hip.h"
#include "hisparse_wide.h"
#include "hsp_common.h"

namespace hisparse {
namespace hsw {

constexpr uint32_t kMaxD = 256;      // features per row

// hsw_create's arguments and the pattern itself; HS_OK or the code, with `why` set
inline int check_create(uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t flags, std::string& why) {
    if (flags & ~uint32_t(HSW_TRANSPOSED)) {
        why = "unknown flag bits (HSW_TRANSPOSED = 1 is the only one)";
        return HS_ERR_BAD_ARG;
    }
    return hsp::check_pattern(HS_IMPL_FLOAT_POB, num_rows, num_cols, indptr, indices, 1, why);
}

// The transposed pattern, stable: cptr[c] ... cptr[c + 1] are column c's entries in ascending CSR index; row[k] is the row of the k-th
// of them and perm[k] its CSR index.
inline void build_transposed(uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, std::vector<uint32_t>& cptr, std::vector<uint32_t>& row,
                             std::vector<uint32_t>& perm) {
    const uint64_t nnz = indptr[num_rows];
    cptr.assign(size_t(num_cols) + 1, 0);
    row.resize(nnz);
    perm.resize(nnz);
    for (uint64_t e = 0; e < nnz; ++e) ++cptr[indices[e] + 1];
    for (uint32_t c = 0; c < num_cols; ++c) cptr[c + 1] += cptr[c];
    std::vector<uint32_t> next(cptr.begin(), cptr.end() - 1);
    for (uint32_t r = 0; r < num_rows; ++r) {
        for (uint64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            const uint32_t k = next[indices[e]]++;
            row[k] = r;
            perm[k] = uint32_t(e);
        }
    }
}

// the ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

inline int check_d(uint32_t d, std::string& why) {
    if (d < 1 || d > kMaxD) {
        why = "d must be 1 ... 256";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// a dense operand of the _device forms: n rows of ld words, d of them used
inline int check_features(const char* name, const void* p, uint64_t ld, uint32_t d, std::string& why) {
    if (!p) {
        why = std::string("null ") + name;
        return HS_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(p) % 16) {
        why = std::string(name) + " must be 16-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    if (ld % 4 || ld < d) {
        why = std::string("the leading dimension of ") + name + " must be a multiple of 4 words and at least d";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// an array of nnz words in CSR order
inline int check_entries(const char* name, const void* p, std::string& why) {
    if (!p) {
        why = std::string("null ") + name;
        return HS_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(p) % 4) {
        why = std::string(name) + " must be 4-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsw_sddmm_device's arguments
inline int check_sddmm(uint32_t num_rows, uint32_t num_cols, uint64_t nnz, const float* u, uint64_t ldu, const float* v, uint64_t ldv, uint32_t d, const float* out,
                       std::string& why) {
    if (int rc = check_d(d, why)) return rc;
    if (int rc = check_features("u", u, ldu, d, why)) return rc;
    if (int rc = check_features("v", v, ldv, d, why)) return rc;
    if (int rc = check_entries("out", out, why)) return rc;
    if (overlap(out, nnz * 4, u, uint64_t(num_rows) * ldu * 4) || overlap(out, nnz * 4, v, uint64_t(num_cols) * ldv * 4)) {
        why = "out overlaps an input";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsw_spmm_device's arguments (x_rows x ldx gathered, y_rows x ldy written); hsw_spmm_t_device's with the two counts exchanged
inline int check_spmm(uint32_t y_rows, uint32_t x_rows, uint64_t nnz, const float* w, const float* x, uint64_t ldx, uint32_t d, const float* y, uint64_t ldy, std::string& why) {
    if (int rc = check_d(d, why)) return rc;
    if (int rc = check_entries("w", w, why)) return rc;
    if (int rc = check_features("x", x, ldx, d, why)) return rc;
    if (int rc = check_features("y", y, ldy, d, why)) return rc;
    const uint64_t y_bytes = uint64_t(y_rows) * ldy * 4;
    if (overlap(y, y_bytes, w, nnz * 4) || overlap(y, y_bytes, x, uint64_t(x_rows) * ldx * 4)) {
        why = "y overlaps an input";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// the host forms: ld = d, no alignment rule (both implementations copy or walk the arrays as they are)
// a and b are the inputs of a_words and b_words, out the result of out_words
inline int check_host(uint32_t d, const void* a, uint64_t a_words, const void* b, uint64_t b_words, const void* out, uint64_t out_words, std::string& why) {
    if (int rc = check_d(d, why)) return rc;
    if (!a || !b || !out) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (overlap(out, out_words * 4, a, a_words * 4) || overlap(out, out_words * 4, b, b_words * 4)) {
        why = "the result overlaps an input";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

}  // namespace hsw
}  // namespace hisparse

#endif  // HISPARSE_HSW_COMMON_H_
