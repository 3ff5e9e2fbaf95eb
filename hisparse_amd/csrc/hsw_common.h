// hsw_common.h — what the two implementations of include/hisparse_wide.h share (hsw_api.cpp on the HIP runtime, hsw_cpu.cpp on the host):
// the limits, the argument checks, so that both refuse the same calls with the same codes, and the counting sort that builds the
// transposed pattern; and the argument checks of include/hisparse_aggregate.h, whose four calls work on the same object.  The pattern
// check itself is hsp_common.h's, the one hsp_create applies.  Host code only.
#ifndef HISPARSE_HSW_COMMON_H_
#define HISPARSE_HSW_COMMON_H_

#include <cstdint>
#include <string>
#include <vector>

#include "hisparse_aggregate.h"
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

// ---- the calls of include/hisparse_aggregate.h: sum / mean / max / min of the neighbours' rows on the same object ------------------------
// the aggregators of a call
inline int check_ops(uint32_t ops, std::string& why) {
    if (ops == 0) {
        why = "ops names no aggregator";
        return HS_ERR_BAD_ARG;
    }
    if (ops & ~uint32_t(HSAGG_SUM | HSAGG_MEAN | HSAGG_MAX | HSAGG_MIN)) {
        why = "unknown bits in ops (HSAGG_SUM = 1, HSAGG_MEAN = 2, HSAGG_MAX = 4, HSAGG_MIN = 8)";
        return HS_ERR_BAD_ARG;
    }
    if ((ops & HSAGG_SUM) && (ops & HSAGG_MEAN)) {
        why = "HSAGG_SUM and HSAGG_MEAN share an output: ask for one of them";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// One operand of an aggregation call: p is null for an operand the call does not use.
struct AggRange {
    const char* name;
    const void* p;
    uint64_t bytes;
};

// no result (the first `results` of r) shares a byte with another operand of the call
inline int check_apart(const AggRange* r, size_t count, size_t results, std::string& why) {
    for (size_t i = 0; i < results; ++i) {
        for (size_t k = 0; k < count; ++k) {
            if (k == i || !r[i].p || !r[k].p || (k < results && k < i)) continue;
            if (overlap(r[i].p, r[i].bytes, r[k].p, r[k].bytes)) {
                why = std::string(r[i].name) + " overlaps " + r[k].name;
                return HS_ERR_BAD_ARG;
            }
        }
    }
    return HS_OK;
}

// hsagg_forward_device's arguments.  Outputs whose bit is not set are not looked at; the arg arrays may be null.
inline int check_agg_forward(uint32_t num_rows, uint32_t num_cols, uint32_t ops, const float* x, uint64_t ldx, uint32_t d, const float* ysum, const float* ymax,
                             const uint32_t* amax, const float* ymin, const uint32_t* amin, uint64_t ldy, std::string& why) {
    if (int rc = check_ops(ops, why)) return rc;
    if (int rc = check_d(d, why)) return rc;
    if (int rc = check_features("x", x, ldx, d, why)) return rc;
    const bool sum = ops & (HSAGG_SUM | HSAGG_MEAN), max = ops & HSAGG_MAX, min = ops & HSAGG_MIN;
    if (sum)
        if (int rc = check_features("ysum", ysum, ldy, d, why)) return rc;
    if (max)
        if (int rc = check_features("ymax", ymax, ldy, d, why)) return rc;
    if (max && amax)
        if (int rc = check_features("amax", amax, ldy, d, why)) return rc;
    if (min)
        if (int rc = check_features("ymin", ymin, ldy, d, why)) return rc;
    if (min && amin)
        if (int rc = check_features("amin", amin, ldy, d, why)) return rc;
    const uint64_t y_bytes = uint64_t(num_rows) * ldy * 4;
    const AggRange r[] = {{"ysum", sum ? ysum : nullptr, y_bytes}, {"ymax", max ? ymax : nullptr, y_bytes}, {"amax", max ? amax : nullptr, y_bytes},
                          {"ymin", min ? ymin : nullptr, y_bytes}, {"amin", min ? amin : nullptr, y_bytes}, {"x", x, uint64_t(num_cols) * ldx * 4}};
    return check_apart(r, 6, 5, why);
}

// hsagg_backward_device's arguments: a set HSAGG_MAX / HSAGG_MIN bit needs both the gradient and the arg array
inline int check_agg_backward(uint32_t num_rows, uint32_t num_cols, uint32_t ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin,
                              const uint32_t* amin, uint64_t ldg, uint32_t d, const float* gx, uint64_t ldgx, std::string& why) {
    if (int rc = check_ops(ops, why)) return rc;
    if (int rc = check_d(d, why)) return rc;
    const bool sum = ops & (HSAGG_SUM | HSAGG_MEAN), max = ops & HSAGG_MAX, min = ops & HSAGG_MIN;
    if (sum)
        if (int rc = check_features("gsum", gsum, ldg, d, why)) return rc;
    if (max) {
        if (int rc = check_features("gmax", gmax, ldg, d, why)) return rc;
        if (int rc = check_features("amax", amax, ldg, d, why)) return rc;
    }
    if (min) {
        if (int rc = check_features("gmin", gmin, ldg, d, why)) return rc;
        if (int rc = check_features("amin", amin, ldg, d, why)) return rc;
    }
    if (int rc = check_features("gx", gx, ldgx, d, why)) return rc;
    const uint64_t g_bytes = uint64_t(num_rows) * ldg * 4;
    const AggRange r[] = {{"gx", gx, uint64_t(num_cols) * ldgx * 4}, {"gsum", sum ? gsum : nullptr, g_bytes}, {"gmax", max ? gmax : nullptr, g_bytes},
                          {"amax", max ? amax : nullptr, g_bytes}, {"gmin", min ? gmin : nullptr, g_bytes}, {"amin", min ? amin : nullptr, g_bytes}};
    return check_apart(r, 6, 1, why);
}

// the host forms: every ld = d, no alignment rule
inline int check_agg_forward_host(uint32_t num_rows, uint32_t num_cols, uint32_t ops, const float* x, uint32_t d, const float* ysum, const float* ymax, const uint32_t* amax,
                                  const float* ymin, const uint32_t* amin, std::string& why) {
    if (int rc = check_ops(ops, why)) return rc;
    if (int rc = check_d(d, why)) return rc;
    const bool sum = ops & (HSAGG_SUM | HSAGG_MEAN), max = ops & HSAGG_MAX, min = ops & HSAGG_MIN;
    if (!x || (sum && !ysum) || (max && !ymax) || (min && !ymin)) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    const uint64_t y_bytes = uint64_t(num_rows) * d * 4;
    const AggRange r[] = {{"ysum", sum ? ysum : nullptr, y_bytes}, {"ymax", max ? ymax : nullptr, y_bytes}, {"amax", max ? amax : nullptr, y_bytes},
                          {"ymin", min ? ymin : nullptr, y_bytes}, {"amin", min ? amin : nullptr, y_bytes}, {"x", x, uint64_t(num_cols) * d * 4}};
    return check_apart(r, 6, 5, why);
}

inline int check_agg_backward_host(uint32_t num_rows, uint32_t num_cols, uint32_t ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin,
                                   const uint32_t* amin, uint32_t d, const float* gx, std::string& why) {
    if (int rc = check_ops(ops, why)) return rc;
    if (int rc = check_d(d, why)) return rc;
    const bool sum = ops & (HSAGG_SUM | HSAGG_MEAN), max = ops & HSAGG_MAX, min = ops & HSAGG_MIN;
    if (!gx || (sum && !gsum) || (max && (!gmax || !amax)) || (min && (!gmin || !amin))) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    const uint64_t g_bytes = uint64_t(num_rows) * d * 4;
    const AggRange r[] = {{"gx", gx, uint64_t(num_cols) * d * 4}, {"gsum", sum ? gsum : nullptr, g_bytes}, {"gmax", max ? gmax : nullptr, g_bytes},
                          {"amax", max ? amax : nullptr, g_bytes}, {"gmin", min ? gmin : nullptr, g_bytes}, {"amin", min ? amin : nullptr, g_bytes}};
    return check_apart(r, 6, 1, why);
}

}  // namespace hsw
}  // namespace hisparse

#endif  // HISPARSE_HSW_COMMON_H_
