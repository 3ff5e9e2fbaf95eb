// hsmh_common.h — what the two implementations of include/hisparse_heads.h share (hsmh_api.cpp on the HIP runtime, hsmh_cpu.cpp on the
// host): the argument checks, so that both refuse the same calls with the same codes.  Built from hsat_common.h's checks (the pattern,
// scale, the reach of an operand), hsab_common.h's overlap check of the backward and hsw_common.h's checks of one operand, all taken at
// the width heads * d.  The calls with a bias of include/hisparse_heads_bias.h add the checks of their two per-entry arrays, and the
// calls with dropout of include/hisparse_heads_dropout.h those of drop_p and of a bias that may be null, at the end, with hsmhd_keep_mask
// itself, which both libraries export, and with the same over bf16 features for include/hisparse_heads_dropout_bf16.h; the calls of include/hisparse_gat.h (additive scores from one word per node and head) their
// slope and the checks of the five head arrays, after that; the calls of include/hisparse_gatv2.h the checks of a, ga and the caller's
// workspace, last.  Host code only.
#ifndef HISPARSE_HSMH_COMMON_H_
#define HISPARSE_HSMH_COMMON_H_

#include <cmath>
#include <cstdint>
#include <string>

#include "hisparse_heads.h"
#include "hisparse_heads_dropout_bf16.h"
#include "hsab_common.h"
#include "philox.h"

namespace hisparse {
namespace hsmh {

constexpr uint32_t kMaxHeads = 64;
constexpr uint32_t kMaxWidth = 256;      // heads * d

// hsmh_create's arguments and the pattern itself: hsat_create's check, max_heads and the flags
inline int check_create(uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags, std::string& why) {
    if (flags & ~uint32_t(HSMH_BACKWARD)) {
        why = "unknown flag bits (HSMH_BACKWARD = 1 is the only one)";
        return HS_ERR_BAD_ARG;
    }
    if (max_heads < 1 || max_heads > kMaxHeads) {
        why = "max_heads must be 1 ... 64";
        return HS_ERR_BAD_ARG;
    }
    return hsat::check_create(num_rows, num_cols, indptr, indices, why);
}

// the SHAPES ACCEPTED paragraph of the header
inline int check_shape(uint32_t heads, uint32_t d, uint32_t max_heads, std::string& why) {
    const char* other = "; the per-head calls of hsat_forward_device / hsab_backward_device cover every other shape";
    if (d < 4 || d > kMaxWidth || (d & (d - 1))) {
        why = std::string("d must be one of 4, 8, 16, 32, 64, 128, 256") + other;
        return HS_ERR_BAD_ARG;
    }
    if (heads < 1 || heads > max_heads) {
        why = std::string("heads must be 1 ... max_heads, the count given to hsmh_create") + other;
        return HS_ERR_BAD_ARG;
    }
    if (uint64_t(heads) * d > kMaxWidth) {
        why = std::string("heads * d must be at most 256") + other;
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// lse: num_rows rows of ldl words, `heads` of them used
inline int check_lse(const float* lse, uint64_t ldl, uint32_t heads, std::string& why) {
    if (int rc = hsw::check_entries("lse", lse, why)) return rc;
    if (ldl < heads) {
        why = "the leading dimension of lse must be at least heads";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}
inline uint64_t lse_reach(uint64_t n, uint64_t ldl, uint32_t heads) { return n ? ((n - 1) * ldl + heads) * 4 : 0; }

// hsmh_forward_device's arguments
inline int check_forward(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv,
                         uint32_t heads, uint32_t d, float scale, const float* y, uint64_t ldy, const float* lse, uint64_t ldl, std::string& why) {
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = hsw::check_features("q", q, ldq, w, why)) return rc;
    if (int rc = hsw::check_features("k", k, ldk, w, why)) return rc;
    if (int rc = hsw::check_features("v", v, ldv, w, why)) return rc;
    if (int rc = hsw::check_features("y", y, ldy, w, why)) return rc;
    if (lse)
        if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = hsat::check_scale(scale, why)) return rc;
    return hsat::check_overlaps(q, hsat::reach(num_rows, ldq, w), k, hsat::reach(num_cols, ldk, w), v, hsat::reach(num_cols, ldv, w), y, hsat::reach(num_rows, ldy, w), lse,
                                lse_reach(num_rows, ldl, heads), why);
}

// hsmh_forward's: ld = heads * d, ldl = heads, no alignment rule (both implementations copy or walk the arrays as they are)
inline int check_forward_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const float* q, const float* k, const float* v, uint32_t heads, uint32_t d, float scale,
                              const float* y, const float* lse, std::string& why) {
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    if (!q || !k || !v || !y) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4;
    return hsat::check_overlaps(q, rb, k, cb, v, cb, y, rb, lse, uint64_t(num_rows) * heads * 4, why);
}

inline int check_backward_flag(bool backward, std::string& why) {
    if (!backward) {
        why = "the object was created without HSMH_BACKWARD";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsmh_backward_device's arguments
inline int check_backward(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v,
                          uint64_t ldv, const float* gy, uint64_t ldgy, const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float scale, const float* gq, uint64_t ldgq,
                          const float* gk, uint64_t ldgk, const float* gv, uint64_t ldgv, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = hsw::check_features("q", q, ldq, w, why)) return rc;
    if (int rc = hsw::check_features("k", k, ldk, w, why)) return rc;
    if (int rc = hsw::check_features("v", v, ldv, w, why)) return rc;
    if (int rc = hsw::check_features("gy", gy, ldgy, w, why)) return rc;
    if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = hsw::check_features("gq", gq, ldgq, w, why)) return rc;
    if (int rc = hsw::check_features("gk", gk, ldgk, w, why)) return rc;
    if (int rc = hsw::check_features("gv", gv, ldgv, w, why)) return rc;
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const hsab::Range in[5] = {{"q", q, hsat::reach(num_rows, ldq, w)}, {"k", k, hsat::reach(num_cols, ldk, w)}, {"v", v, hsat::reach(num_cols, ldv, w)},
                               {"gy", gy, hsat::reach(num_rows, ldgy, w)}, {"lse", lse, lse_reach(num_rows, ldl, heads)}};
    const hsab::Range out[3] = {{"gq", gq, hsat::reach(num_rows, ldgq, w)}, {"gk", gk, hsat::reach(num_cols, ldgk, w)}, {"gv", gv, hsat::reach(num_cols, ldgv, w)}};
    return hsab::check_overlaps(in, out, why);
}

// hsmh_backward's: ld = heads * d, ldl = heads, no alignment rule
inline int check_backward_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const float* q, const float* k, const float* v, const float* gy,
                               const float* lse, uint32_t heads, uint32_t d, float scale, const float* gq, const float* gk, const float* gv, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    if (!q || !k || !v || !gy || !lse || !gq || !gk || !gv) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4;
    const hsab::Range in[5] = {{"q", q, rb}, {"k", k, cb}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * heads * 4}};
    const hsab::Range out[3] = {{"gq", gq, rb}, {"gk", gk, cb}, {"gv", gv, cb}};
    return hsab::check_overlaps(in, out, why);
}

// ---- the bf16 calls of include/hisparse_heads_bf16.h: the same rules over 2-byte elements, every reach in bytes ----------------------

constexpr uint32_t kMaxWidth16 = 512;      // heads * d in elements: 1 KiB, the 64 chunks of the widest group as kMaxWidth words are

// the SHAPES ACCEPTED paragraph of hisparse_heads_bf16.h
inline int check_shape16(uint32_t heads, uint32_t d, uint32_t max_heads, std::string& why) {
    const char* other = "; the fp32 calls hsmh_forward_device / hsmh_backward_device take operands widened to fp32, at d = 4 too";
    if (d < 8 || d > 256 || (d & (d - 1))) {
        why = std::string("d must be one of 8, 16, 32, 64, 128, 256 with bf16 operands (a head is whole 16-byte chunks of 8 elements)") + other;
        return HS_ERR_BAD_ARG;
    }
    if (heads < 1 || heads > max_heads) {
        why = std::string("heads must be 1 ... max_heads, the count given to hsmh_create") + other;
        return HS_ERR_BAD_ARG;
    }
    if (uint64_t(heads) * d > kMaxWidth16) {
        why = std::string("heads * d must be at most 512 with bf16 operands (a row of at most 1 KiB)") + other;
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// one bf16 feature operand of w = heads * d elements per row
inline int check_features16(const char* name, const void* p, uint64_t ld, uint32_t w, std::string& why) {
    if (!p) {
        why = std::string("null ") + name;
        return HS_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(p) % 16) {
        why = std::string(name) + " must be 16-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    if (ld % 8 || ld < w) {
        why = std::string("the leading dimension of ") + name + " must be a multiple of 8 elements and at least heads * d";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// the bytes of a bf16 operand of n rows: to the end of the 16-byte chunk that holds element w - 1 of row n - 1 (w is a multiple of 8)
inline uint64_t reach16(uint64_t n, uint64_t ld, uint32_t w) { return n ? ((n - 1) * ld + w) * 2 : 0; }

// hsmh16_forward_device's arguments
inline int check_forward16(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv,
                           uint32_t heads, uint32_t d, float scale, const uint16_t* y, uint64_t ldy, const float* lse, uint64_t ldl, std::string& why) {
    if (int rc = check_shape16(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = check_features16("q", q, ldq, w, why)) return rc;
    if (int rc = check_features16("k", k, ldk, w, why)) return rc;
    if (int rc = check_features16("v", v, ldv, w, why)) return rc;
    if (int rc = check_features16("y", y, ldy, w, why)) return rc;
    if (lse)
        if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = hsat::check_scale(scale, why)) return rc;
    return hsat::check_overlaps(q, reach16(num_rows, ldq, w), k, reach16(num_cols, ldk, w), v, reach16(num_cols, ldv, w), y, reach16(num_rows, ldy, w), lse,
                                lse_reach(num_rows, ldl, heads), why);
}

// hsmh16_forward's: ld = heads * d, ldl = heads, no alignment rule
inline int check_forward16_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint32_t heads, uint32_t d,
                                float scale, const uint16_t* y, const float* lse, std::string& why) {
    if (int rc = check_shape16(heads, d, max_heads, why)) return rc;
    if (!q || !k || !v || !y) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 2, cb = uint64_t(num_cols) * heads * d * 2;
    return hsat::check_overlaps(q, rb, k, cb, v, cb, y, rb, lse, uint64_t(num_rows) * heads * 4, why);
}

// hsmh16_backward_device's arguments
inline int check_backward16(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk,
                            const uint16_t* v, uint64_t ldv, const uint16_t* gy, uint64_t ldgy, const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float scale,
                            const uint16_t* gq, uint64_t ldgq, const uint16_t* gk, uint64_t ldgk, const uint16_t* gv, uint64_t ldgv, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape16(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = check_features16("q", q, ldq, w, why)) return rc;
    if (int rc = check_features16("k", k, ldk, w, why)) return rc;
    if (int rc = check_features16("v", v, ldv, w, why)) return rc;
    if (int rc = check_features16("gy", gy, ldgy, w, why)) return rc;
    if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = check_features16("gq", gq, ldgq, w, why)) return rc;
    if (int rc = check_features16("gk", gk, ldgk, w, why)) return rc;
    if (int rc = check_features16("gv", gv, ldgv, w, why)) return rc;
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const hsab::Range in[5] = {{"q", q, reach16(num_rows, ldq, w)}, {"k", k, reach16(num_cols, ldk, w)}, {"v", v, reach16(num_cols, ldv, w)},
                               {"gy", gy, reach16(num_rows, ldgy, w)}, {"lse", lse, lse_reach(num_rows, ldl, heads)}};
    const hsab::Range out[3] = {{"gq", gq, reach16(num_rows, ldgq, w)}, {"gk", gk, reach16(num_cols, ldgk, w)}, {"gv", gv, reach16(num_cols, ldgv, w)}};
    return hsab::check_overlaps(in, out, why);
}

// hsmh16_backward's: ld = heads * d, ldl = heads, no alignment rule
inline int check_backward16_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy,
                                 const float* lse, uint32_t heads, uint32_t d, float scale, const uint16_t* gq, const uint16_t* gk, const uint16_t* gv, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape16(heads, d, max_heads, why)) return rc;
    if (!q || !k || !v || !gy || !lse || !gq || !gk || !gv) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 2, cb = uint64_t(num_cols) * heads * d * 2;
    const hsab::Range in[5] = {{"q", q, rb}, {"k", k, cb}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * heads * 4}};
    const hsab::Range out[3] = {{"gq", gq, rb}, {"gk", gk, cb}, {"gv", gv, cb}};
    return hsab::check_overlaps(in, out, why);
}

// ---- the calls with a bias of include/hisparse_heads_bias.h: the fp32 rules, and those of the two per-entry arrays --------------------

// bias or gbias: nnz entries of ld words, `heads` of them used
inline int check_bias(const char* name, const float* b, uint64_t ld, uint32_t heads, std::string& why) {
    if (int rc = hsw::check_entries(name, b, why)) return rc;
    if (ld < heads) {
        why = std::string("the leading dimension of ") + name + " must be at least heads";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}
inline uint64_t bias_reach(uint64_t nnz, uint64_t ld, uint32_t heads) { return nnz ? ((nnz - 1) * ld + heads) * 4 : 0; }

// an output of a call against one more input
inline int check_apart(const char* out_name, const void* out, uint64_t out_bytes, const char* in_name, const void* in, uint64_t in_bytes, std::string& why) {
    if (out && in && hsw::overlap(out, out_bytes, in, in_bytes)) {
        why = std::string(out_name) + " overlaps " + in_name;
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

inline int check_map(bool map, std::string& why, const char* with = "a bias") {
    if (!map) {
        why = std::string("the object holds no entry map: the backward with ") + with + " needs an object from hsmhb_create with HSMH_BACKWARD";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsmhb_forward_device's arguments: hsmh_forward_device's, and bias as one more input
inline int check_forward_bias(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, uint64_t nnz, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v,
                              uint64_t ldv, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, const float* y, uint64_t ldy, const float* lse, uint64_t ldl,
                              std::string& why) {
    if (int rc = check_forward(num_rows, num_cols, max_heads, q, ldq, k, ldk, v, ldv, heads, d, scale, y, ldy, lse, ldl, why)) return rc;
    if (int rc = check_bias("bias", bias, ldb, heads, why)) return rc;
    const uint64_t bb = bias_reach(nnz, ldb, heads);
    if (int rc = check_apart("y", y, hsat::reach(num_rows, ldy, heads * d), "bias", bias, bb, why)) return rc;
    return check_apart("lse", lse, lse_reach(num_rows, ldl, heads), "bias", bias, bb, why);
}

// hsmhb_forward's: ld = heads * d, ldl = ldb = heads, no alignment rule
inline int check_forward_bias_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, uint64_t nnz, const float* q, const float* k, const float* v, const float* bias,
                                   uint32_t heads, uint32_t d, float scale, const float* y, const float* lse, std::string& why) {
    if (int rc = check_forward_host(num_rows, num_cols, max_heads, q, k, v, heads, d, scale, y, lse, why)) return rc;
    if (!bias) {
        why = "null bias";
        return HS_ERR_BAD_ARG;
    }
    const uint64_t bb = nnz * heads * 4;
    if (int rc = check_apart("y", y, uint64_t(num_rows) * heads * d * 4, "bias", bias, bb, why)) return rc;
    return check_apart("lse", lse, uint64_t(num_rows) * heads * 4, "bias", bias, bb, why);
}

// what the two backward forms share once the plain call's checks have passed: bias against gQ, gK and gV, gbias against everything
inline int check_bias_overlaps(const hsab::Range (&in)[6], const hsab::Range (&out)[3], const float* gbias, uint64_t gbias_bytes, std::string& why) {
    for (const hsab::Range& o : out)
        if (int rc = check_apart(o.name, o.p, o.bytes, in[5].name, in[5].p, in[5].bytes, why)) return rc;
    if (!gbias) return HS_OK;
    for (const hsab::Range& i : in)
        if (int rc = check_apart("gbias", gbias, gbias_bytes, i.name, i.p, i.bytes, why)) return rc;
    for (const hsab::Range& o : out)
        if (int rc = check_apart("gbias", gbias, gbias_bytes, o.name, o.p, o.bytes, why)) return rc;
    return HS_OK;
}

// hsmhb_backward_device's arguments: the map, hsmh_backward_device's, bias as one more input and gbias (may be null) as one more output
inline int check_backward_bias(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool map, uint64_t nnz, const float* q, uint64_t ldq, const float* k, uint64_t ldk,
                               const float* v, uint64_t ldv, const float* gy, uint64_t ldgy, const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d,
                               float scale, const float* gq, uint64_t ldgq, const float* gk, uint64_t ldgk, const float* gv, uint64_t ldgv, const float* gbias, uint64_t ldgb,
                               std::string& why) {
    if (int rc = check_map(map, why)) return rc;
    if (int rc = check_backward(num_rows, num_cols, max_heads, true, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, heads, d, scale, gq, ldgq, gk, ldgk, gv, ldgv, why)) return rc;
    if (int rc = check_bias("bias", bias, ldb, heads, why)) return rc;
    if (gbias)
        if (int rc = check_bias("gbias", gbias, ldgb, heads, why)) return rc;
    const uint32_t w = heads * d;
    const hsab::Range in[6] = {{"q", q, hsat::reach(num_rows, ldq, w)}, {"k", k, hsat::reach(num_cols, ldk, w)}, {"v", v, hsat::reach(num_cols, ldv, w)},
                               {"gy", gy, hsat::reach(num_rows, ldgy, w)}, {"lse", lse, lse_reach(num_rows, ldl, heads)}, {"bias", bias, bias_reach(nnz, ldb, heads)}};
    const hsab::Range out[3] = {{"gq", gq, hsat::reach(num_rows, ldgq, w)}, {"gk", gk, hsat::reach(num_cols, ldgk, w)}, {"gv", gv, hsat::reach(num_cols, ldgv, w)}};
    return check_bias_overlaps(in, out, gbias, bias_reach(nnz, ldgb, heads), why);
}

// hsmhb_backward's: ld = heads * d, ldl = ldb = ldgb = heads, no alignment rule
inline int check_backward_bias_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool map, uint64_t nnz, const float* q, const float* k, const float* v, const float* gy,
                                    const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale, const float* gq, const float* gk, const float* gv,
                                    const float* gbias, std::string& why) {
    if (int rc = check_map(map, why)) return rc;
    if (int rc = check_backward_host(num_rows, num_cols, max_heads, true, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return rc;
    if (!bias) {
        why = "null bias";
        return HS_ERR_BAD_ARG;
    }
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4, eb = nnz * heads * 4;
    const hsab::Range in[6] = {{"q", q, rb}, {"k", k, cb}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * heads * 4}, {"bias", bias, eb}};
    const hsab::Range out[3] = {{"gq", gq, rb}, {"gk", gk, cb}, {"gv", gv, cb}};
    return check_bias_overlaps(in, out, gbias, eb, why);
}

// ---- the calls with dropout of include/hisparse_heads_dropout.h: the rules above with a bias that may be null, and drop_p ------------

inline int check_drop(float drop_p, std::string& why) {
    if (!std::isfinite(drop_p) || drop_p < 0.0f || drop_p >= 1.0f) {
        why = "drop_p must be finite and in [0, 1)";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsmhd_forward_device's arguments: hsmhb_forward_device's with a bias, hsmh_forward_device's without, and drop_p
inline int check_forward_dropout(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, uint64_t nnz, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v,
                                 uint64_t ldv, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, const float* y, uint64_t ldy, const float* lse,
                                 uint64_t ldl, std::string& why) {
    if (int rc = bias ? check_forward_bias(num_rows, num_cols, max_heads, nnz, q, ldq, k, ldk, v, ldv, bias, ldb, heads, d, scale, y, ldy, lse, ldl, why)
                      : check_forward(num_rows, num_cols, max_heads, q, ldq, k, ldk, v, ldv, heads, d, scale, y, ldy, lse, ldl, why))
        return rc;
    return check_drop(drop_p, why);
}

// hsmhd_forward's: ld = heads * d, ldl = ldb = heads, no alignment rule
inline int check_forward_dropout_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, uint64_t nnz, const float* q, const float* k, const float* v, const float* bias,
                                      uint32_t heads, uint32_t d, float scale, float drop_p, const float* y, const float* lse, std::string& why) {
    if (int rc = bias ? check_forward_bias_host(num_rows, num_cols, max_heads, nnz, q, k, v, bias, heads, d, scale, y, lse, why)
                      : check_forward_host(num_rows, num_cols, max_heads, q, k, v, heads, d, scale, y, lse, why))
        return rc;
    return check_drop(drop_p, why);
}

// hsmhd_backward_device's arguments: the map (it keys the column side's draws, with or without a bias), hsmhb_backward_device's with a
// bias; without one hsmh_backward_device's and gbias (may be null) as one more output
inline int check_backward_dropout(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool map, uint64_t nnz, const float* q, uint64_t ldq, const float* k, uint64_t ldk,
                                  const float* v, uint64_t ldv, const float* gy, uint64_t ldgy, const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads,
                                  uint32_t d, float scale, float drop_p, const float* gq, uint64_t ldgq, const float* gk, uint64_t ldgk, const float* gv, uint64_t ldgv,
                                  const float* gbias, uint64_t ldgb, std::string& why) {
    if (int rc = check_map(map, why, "dropout")) return rc;
    if (bias) {
        if (int rc = check_backward_bias(num_rows, num_cols, max_heads, map, nnz, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, bias, ldb, heads, d, scale, gq, ldgq, gk, ldgk, gv, ldgv,
                                         gbias, ldgb, why))
            return rc;
        return check_drop(drop_p, why);
    }
    if (int rc = check_backward(num_rows, num_cols, max_heads, true, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, heads, d, scale, gq, ldgq, gk, ldgk, gv, ldgv, why)) return rc;
    if (gbias)
        if (int rc = check_bias("gbias", gbias, ldgb, heads, why)) return rc;
    const uint32_t w = heads * d;
    const hsab::Range in[6] = {{"q", q, hsat::reach(num_rows, ldq, w)}, {"k", k, hsat::reach(num_cols, ldk, w)}, {"v", v, hsat::reach(num_cols, ldv, w)},
                               {"gy", gy, hsat::reach(num_rows, ldgy, w)}, {"lse", lse, lse_reach(num_rows, ldl, heads)}, {"bias", nullptr, 0}};
    const hsab::Range out[3] = {{"gq", gq, hsat::reach(num_rows, ldgq, w)}, {"gk", gk, hsat::reach(num_cols, ldgk, w)}, {"gv", gv, hsat::reach(num_cols, ldgv, w)}};
    if (int rc = check_bias_overlaps(in, out, gbias, bias_reach(nnz, ldgb, heads), why)) return rc;
    return check_drop(drop_p, why);
}

// hsmhd_backward's: ld = heads * d, ldl = ldb = ldgb = heads, no alignment rule
inline int check_backward_dropout_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool map, uint64_t nnz, const float* q, const float* k, const float* v,
                                       const float* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, const float* gq, const float* gk,
                                       const float* gv, const float* gbias, std::string& why) {
    if (int rc = check_map(map, why, "dropout")) return rc;
    if (bias) {
        if (int rc = check_backward_bias_host(num_rows, num_cols, max_heads, map, nnz, q, k, v, gy, lse, bias, heads, d, scale, gq, gk, gv, gbias, why)) return rc;
        return check_drop(drop_p, why);
    }
    if (int rc = check_backward_host(num_rows, num_cols, max_heads, true, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4, eb = nnz * heads * 4;
    const hsab::Range in[6] = {{"q", q, rb}, {"k", k, cb}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * heads * 4}, {"bias", nullptr, 0}};
    const hsab::Range out[3] = {{"gq", gq, rb}, {"gk", gk, cb}, {"gv", gv, cb}};
    if (int rc = check_bias_overlaps(in, out, gbias, eb, why)) return rc;
    return check_drop(drop_p, why);
}

// ---- the bf16 calls with dropout of include/hisparse_heads_dropout_bf16.h: the bf16 rules for the features, the rules above for the rest --

// hsmhd16_forward_device's arguments: hsmh16_forward_device's, bias (may be null) as one more input, and drop_p
inline int check_forward_dropout16(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, uint64_t nnz, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk,
                                   const uint16_t* v, uint64_t ldv, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, const uint16_t* y,
                                   uint64_t ldy, const float* lse, uint64_t ldl, std::string& why) {
    if (int rc = check_forward16(num_rows, num_cols, max_heads, q, ldq, k, ldk, v, ldv, heads, d, scale, y, ldy, lse, ldl, why)) return rc;
    if (bias) {
        if (int rc = check_bias("bias", bias, ldb, heads, why)) return rc;
        const uint64_t bb = bias_reach(nnz, ldb, heads);
        if (int rc = check_apart("y", y, reach16(num_rows, ldy, heads * d), "bias", bias, bb, why)) return rc;
        if (int rc = check_apart("lse", lse, lse_reach(num_rows, ldl, heads), "bias", bias, bb, why)) return rc;
    }
    return check_drop(drop_p, why);
}

// hsmhd16_forward's: ld = heads * d, ldl = ldb = heads, no alignment rule
inline int check_forward_dropout16_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, uint64_t nnz, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                        const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, const uint16_t* y, const float* lse, std::string& why) {
    if (int rc = check_forward16_host(num_rows, num_cols, max_heads, q, k, v, heads, d, scale, y, lse, why)) return rc;
    const uint64_t bb = nnz * heads * 4;
    if (int rc = check_apart("y", y, uint64_t(num_rows) * heads * d * 2, "bias", bias, bb, why)) return rc;
    if (int rc = check_apart("lse", lse, uint64_t(num_rows) * heads * 4, "bias", bias, bb, why)) return rc;
    return check_drop(drop_p, why);
}

// hsmhd16_backward_device's arguments: the map (it keys the column side's draws, with or without a bias), hsmh16_backward_device's, bias
// (may be null) as one more input and gbias (may be null) as one more output
inline int check_backward_dropout16(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool map, uint64_t nnz, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk,
                                    const uint16_t* v, uint64_t ldv, const uint16_t* gy, uint64_t ldgy, const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads,
                                    uint32_t d, float scale, float drop_p, const uint16_t* gq, uint64_t ldgq, const uint16_t* gk, uint64_t ldgk, const uint16_t* gv, uint64_t ldgv,
                                    const float* gbias, uint64_t ldgb, std::string& why) {
    if (int rc = check_map(map, why, "dropout")) return rc;
    if (int rc = check_backward16(num_rows, num_cols, max_heads, true, q, ldq, k, ldk, v, ldv, gy, ldgy, lse, ldl, heads, d, scale, gq, ldgq, gk, ldgk, gv, ldgv, why)) return rc;
    if (bias)
        if (int rc = check_bias("bias", bias, ldb, heads, why)) return rc;
    if (gbias)
        if (int rc = check_bias("gbias", gbias, ldgb, heads, why)) return rc;
    const uint32_t w = heads * d;
    const hsab::Range in[6] = {{"q", q, reach16(num_rows, ldq, w)}, {"k", k, reach16(num_cols, ldk, w)}, {"v", v, reach16(num_cols, ldv, w)},
                               {"gy", gy, reach16(num_rows, ldgy, w)}, {"lse", lse, lse_reach(num_rows, ldl, heads)}, {"bias", bias, bias ? bias_reach(nnz, ldb, heads) : 0}};
    const hsab::Range out[3] = {{"gq", gq, reach16(num_rows, ldgq, w)}, {"gk", gk, reach16(num_cols, ldgk, w)}, {"gv", gv, reach16(num_cols, ldgv, w)}};
    if (int rc = check_bias_overlaps(in, out, gbias, gbias ? bias_reach(nnz, ldgb, heads) : 0, why)) return rc;
    return check_drop(drop_p, why);
}

// hsmhd16_backward's: ld = heads * d, ldl = ldb = ldgb = heads, no alignment rule
inline int check_backward_dropout16_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool map, uint64_t nnz, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                         const uint16_t* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, const uint16_t* gq,
                                         const uint16_t* gk, const uint16_t* gv, const float* gbias, std::string& why) {
    if (int rc = check_map(map, why, "dropout")) return rc;
    if (int rc = check_backward16_host(num_rows, num_cols, max_heads, true, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 2, cb = uint64_t(num_cols) * heads * d * 2, eb = nnz * heads * 4;
    const hsab::Range in[6] = {{"q", q, rb}, {"k", k, cb}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * heads * 4}, {"bias", bias, bias ? eb : 0}};
    const hsab::Range out[3] = {{"gq", gq, rb}, {"gk", gk, cb}, {"gv", gv, cb}};
    if (int rc = check_bias_overlaps(in, out, gbias, eb, why)) return rc;
    return check_drop(drop_p, why);
}

// hsmhd_keep_mask, whole: keep[e * heads + h] = 1 where (entry e, head h) is kept.  An entry's index is a 32-bit word of the counter.
inline int keep_mask(uint64_t nnz, uint32_t heads, float drop_p, uint64_t seed, uint64_t offset, uint8_t* keep) {
    std::string why;
    if (check_drop(drop_p, why) || heads < 1 || heads > kMaxHeads || nnz > (uint64_t(1) << 32) || (nnz && !keep)) return HS_ERR_BAD_ARG;
    const philox::Dropout dr = philox::dropout_of(drop_p, seed, offset);
    for (uint64_t e = 0; e < nnz; ++e) {
        for (uint32_t quad = 0; 4 * quad < heads; ++quad) {      // one draw serves four heads
            const philox::Words x = philox::philox4x32_10(uint32_t(e), quad, dr.off0, dr.off1, dr.key0, dr.key1);
            const uint32_t word[4] = {x.a, x.b, x.c, x.d};
            for (uint32_t h = 4 * quad; h < heads && h < 4 * quad + 4; ++h) keep[e * heads + h] = word[h & 3u] >= dr.thr ? 1 : 0;
        }
    }
    return HS_OK;
}

// ---- the calls of include/hisparse_gat.h: additive scores from one word per node and head, no Q, no K, no scale ----------------------

inline int check_slope(float slope, std::string& why) {
    if (!std::isfinite(slope) || slope < 0.0f) {      // -0.0f is not below zero: it counts as 0
        why = "slope must be finite and at least 0";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// el, er, gel or ger: one row per node of ld words, `heads` of them used; the rules and the reach of lse
inline int check_head_words(const char* name, const float* p, uint64_t ld, uint32_t heads, std::string& why) { return check_bias(name, p, ld, heads, why); }

// hsgat_forward_device's arguments
inline int check_gat_forward(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv,
                             uint32_t heads, uint32_t d, float slope, const float* y, uint64_t ldy, const float* lse, uint64_t ldl, std::string& why) {
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = check_head_words("el", el, ldel, heads, why)) return rc;
    if (int rc = check_head_words("er", er, lder, heads, why)) return rc;
    if (int rc = hsw::check_features("v", v, ldv, w, why)) return rc;
    if (int rc = hsw::check_features("y", y, ldy, w, why)) return rc;
    if (lse)
        if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = check_slope(slope, why)) return rc;
    return hsat::check_overlaps(el, lse_reach(num_rows, ldel, heads), er, lse_reach(num_cols, lder, heads), v, hsat::reach(num_cols, ldv, w), y, hsat::reach(num_rows, ldy, w), lse,
                                lse_reach(num_rows, ldl, heads), why);
}

// hsgat_forward's: ld = heads * d for V and Y, ld = heads for el, er and lse, no alignment rule
inline int check_gat_forward_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const float* el, const float* er, const float* v, uint32_t heads, uint32_t d, float slope,
                                  const float* y, const float* lse, std::string& why) {
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    if (!el || !er || !v || !y) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = check_slope(slope, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4;
    return hsat::check_overlaps(el, uint64_t(num_rows) * heads * 4, er, uint64_t(num_cols) * heads * 4, v, cb, y, rb, lse, uint64_t(num_rows) * heads * 4, why);
}

// hsgat_backward_device's arguments
inline int check_gat_backward(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v,
                              uint64_t ldv, const float* gy, uint64_t ldgy, const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float slope, const float* gel, uint64_t ldgel,
                              const float* ger, uint64_t ldger, const float* gv, uint64_t ldgv, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = check_head_words("el", el, ldel, heads, why)) return rc;
    if (int rc = check_head_words("er", er, lder, heads, why)) return rc;
    if (int rc = hsw::check_features("v", v, ldv, w, why)) return rc;
    if (int rc = hsw::check_features("gy", gy, ldgy, w, why)) return rc;
    if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = check_head_words("gel", gel, ldgel, heads, why)) return rc;
    if (int rc = check_head_words("ger", ger, ldger, heads, why)) return rc;
    if (int rc = hsw::check_features("gv", gv, ldgv, w, why)) return rc;
    if (int rc = check_slope(slope, why)) return rc;
    const hsab::Range in[5] = {{"el", el, lse_reach(num_rows, ldel, heads)}, {"er", er, lse_reach(num_cols, lder, heads)}, {"v", v, hsat::reach(num_cols, ldv, w)},
                               {"gy", gy, hsat::reach(num_rows, ldgy, w)}, {"lse", lse, lse_reach(num_rows, ldl, heads)}};
    const hsab::Range out[3] = {{"gel", gel, lse_reach(num_rows, ldgel, heads)}, {"ger", ger, lse_reach(num_cols, ldger, heads)}, {"gv", gv, hsat::reach(num_cols, ldgv, w)}};
    return hsab::check_overlaps(in, out, why);
}

// hsgat_backward's: ld = heads * d for V, gY and gV, ld = heads for the five head arrays, no alignment rule
inline int check_gat_backward_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const float* el, const float* er, const float* v, const float* gy,
                                   const float* lse, uint32_t heads, uint32_t d, float slope, const float* gel, const float* ger, const float* gv, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    if (!el || !er || !v || !gy || !lse || !gel || !ger || !gv) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = check_slope(slope, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4, rh = uint64_t(num_rows) * heads * 4, ch = uint64_t(num_cols) * heads * 4;
    const hsab::Range in[5] = {{"el", el, rh}, {"er", er, ch}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, rh}};
    const hsab::Range out[3] = {{"gel", gel, rh}, {"ger", ger, ch}, {"gv", gv, cb}};
    return hsab::check_overlaps(in, out, why);
}

// ---- the calls of include/hisparse_gatv2.h: the score a[h] . LeakyReLU(XD[row] + XS[col]); a and ga are heads * d contiguous words ------

// a or ga: heads * d contiguous fp32 words, 16-byte aligned, no ld
inline int check_head_vector(const char* name, const float* p, std::string& why) {
    if (!p) {
        why = std::string("null ") + name;
        return HS_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(p) % 16) {
        why = std::string(name) + " must be 16-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// the workspace of hsgat2_backward_device: at least `need` bytes (what hsgat2_work_bytes says), 16-byte aligned
inline int check_work(const void* work, uint64_t work_bytes, uint64_t need, std::string& why) {
    if (!work) {
        why = "null workspace";
        return HS_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(work) % 16) {
        why = "the workspace must be 16-byte aligned";
        return HS_ERR_BAD_ARG;
    }
    if (work_bytes < need) {
        why = "the workspace is smaller than hsgat2_work_bytes says for this object, heads and d";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsgat2_forward_device's arguments
inline int check_gat2_forward(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, uint32_t heads,
                              uint32_t d, float slope, const float* y, uint64_t ldy, const float* lse, uint64_t ldl, std::string& why) {
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = hsw::check_features("xd", xd, ldxd, w, why)) return rc;
    if (int rc = hsw::check_features("xs", xs, ldxs, w, why)) return rc;
    if (int rc = check_head_vector("a", a, why)) return rc;
    if (int rc = hsw::check_features("y", y, ldy, w, why)) return rc;
    if (lse)
        if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = check_slope(slope, why)) return rc;
    return hsat::check_overlaps(xd, hsat::reach(num_rows, ldxd, w), xs, hsat::reach(num_cols, ldxs, w), a, uint64_t(w) * 4, y, hsat::reach(num_rows, ldy, w), lse,
                                lse_reach(num_rows, ldl, heads), why);
}

// hsgat2_forward's: ld = heads * d, ldl = heads, no alignment rule
inline int check_gat2_forward_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, const float* xd, const float* xs, const float* a, uint32_t heads, uint32_t d, float slope,
                                   const float* y, const float* lse, std::string& why) {
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    if (!xd || !xs || !a || !y) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = check_slope(slope, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4;
    return hsat::check_overlaps(xd, rb, xs, cb, a, uint64_t(heads) * d * 4, y, rb, lse, uint64_t(num_rows) * heads * 4, why);
}

// what the two backward forms share: the three outputs against the five inputs and each other, and the workspace (null in the host
// form) against all eight
inline int check_gat2_overlaps(const hsab::Range (&in)[5], const hsab::Range (&out)[3], const void* work, uint64_t work_bytes, std::string& why) {
    if (int rc = hsab::check_overlaps(in, out, why)) return rc;
    for (const hsab::Range& i : in)
        if (int rc = check_apart("the workspace", work, work_bytes, i.name, i.p, i.bytes, why)) return rc;
    for (const hsab::Range& o : out)
        if (int rc = check_apart("the workspace", work, work_bytes, o.name, o.p, o.bytes, why)) return rc;
    return HS_OK;
}

// hsgat2_backward_device's arguments; `need` is what hsgat2_work_bytes says
inline int check_gat2_backward(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a,
                               const float* gy, uint64_t ldgy, const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float slope, const float* gxd, uint64_t ldgxd, const float* gxs,
                               uint64_t ldgxs, const float* ga, const void* work, uint64_t work_bytes, uint64_t need, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    const uint32_t w = heads * d;
    if (int rc = hsw::check_features("xd", xd, ldxd, w, why)) return rc;
    if (int rc = hsw::check_features("xs", xs, ldxs, w, why)) return rc;
    if (int rc = check_head_vector("a", a, why)) return rc;
    if (int rc = hsw::check_features("gy", gy, ldgy, w, why)) return rc;
    if (int rc = check_lse(lse, ldl, heads, why)) return rc;
    if (int rc = hsw::check_features("gxd", gxd, ldgxd, w, why)) return rc;
    if (int rc = hsw::check_features("gxs", gxs, ldgxs, w, why)) return rc;
    if (int rc = check_head_vector("ga", ga, why)) return rc;
    if (int rc = check_slope(slope, why)) return rc;
    if (int rc = check_work(work, work_bytes, need, why)) return rc;
    const hsab::Range in[5] = {{"xd", xd, hsat::reach(num_rows, ldxd, w)}, {"xs", xs, hsat::reach(num_cols, ldxs, w)}, {"a", a, uint64_t(w) * 4}, {"gy", gy, hsat::reach(num_rows, ldgy, w)},
                               {"lse", lse, lse_reach(num_rows, ldl, heads)}};
    const hsab::Range out[3] = {{"gxd", gxd, hsat::reach(num_rows, ldgxd, w)}, {"gxs", gxs, hsat::reach(num_cols, ldgxs, w)}, {"ga", ga, uint64_t(w) * 4}};
    return check_gat2_overlaps(in, out, work, work_bytes, why);
}

// hsgat2_backward's: ld = heads * d, ldl = heads, no alignment rule, no workspace
inline int check_gat2_backward_host(uint32_t num_rows, uint32_t num_cols, uint32_t max_heads, bool backward, const float* xd, const float* xs, const float* a, const float* gy,
                                    const float* lse, uint32_t heads, uint32_t d, float slope, const float* gxd, const float* gxs, const float* ga, std::string& why) {
    if (int rc = check_backward_flag(backward, why)) return rc;
    if (int rc = check_shape(heads, d, max_heads, why)) return rc;
    if (!xd || !xs || !a || !gy || !lse || !gxd || !gxs || !ga) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = check_slope(slope, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * heads * d * 4, cb = uint64_t(num_cols) * heads * d * 4, ab = uint64_t(heads) * d * 4;
    const hsab::Range in[5] = {{"xd", xd, rb}, {"xs", xs, cb}, {"a", a, ab}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * heads * 4}};
    const hsab::Range out[3] = {{"gxd", gxd, rb}, {"gxs", gxs, cb}, {"ga", ga, ab}};
    return hsab::check_overlaps(in, out, why);
}

}  // namespace hsmh
}  // namespace hisparse

#endif  // HISPARSE_HSMH_COMMON_H_
