// hsat_common.h — what the two implementations of include/hisparse_attention.h share (hsat_api.cpp on the HIP runtime, hsat_cpu.cpp on
// the host): the argument checks, so that both refuse the same calls with the same codes.  Built from hsw_common.h's checks of one
// operand (check_d, check_features, check_entries, overlap) and hsp_common.h's pattern check.  Host code only.
#ifndef HISPARSE_HSAT_COMMON_H_
#define HISPARSE_HSAT_COMMON_H_

#include <cmath>
#include <cstdint>
#include <string>

#include "hisparse_attention.h"
#include "hsw_common.h"

namespace hisparse {
namespace hsat {

// hsat_create's arguments and the pattern itself: hsw_create's check without flags
inline int check_create(uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, std::string& why) {
    return hsw::check_create(num_rows, num_cols, indptr, indices, 0, why);
}

// the bytes of a dense operand of n rows: from its pointer to the end of the 16-byte chunk that holds word d - 1 of row n - 1 (with heads
// by ld, a pointer is offset into its row, so n * ld words from it would pass the end of the caller's array)
inline uint64_t reach(uint64_t n, uint64_t ld, uint32_t d) { return n ? ((n - 1) * ld + hsp::round_up4(d)) * 4 : 0; }

inline int check_scale(float scale, std::string& why) {
    if (!std::isfinite(scale)) {
        why = "scale must be finite";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// y (and lse, when there is one) against the three inputs and each other; every range in bytes
inline int check_overlaps(const void* q, uint64_t q_bytes, const void* k, uint64_t k_bytes, const void* v, uint64_t v_bytes, const void* y, uint64_t y_bytes, const void* lse,
                          uint64_t lse_bytes, std::string& why) {
    if (hsw::overlap(y, y_bytes, q, q_bytes) || hsw::overlap(y, y_bytes, k, k_bytes) || hsw::overlap(y, y_bytes, v, v_bytes)) {
        why = "y overlaps an input";
        return HS_ERR_BAD_ARG;
    }
    if (!lse) return HS_OK;
    if (hsw::overlap(lse, lse_bytes, q, q_bytes) || hsw::overlap(lse, lse_bytes, k, k_bytes) || hsw::overlap(lse, lse_bytes, v, v_bytes)) {
        why = "lse overlaps an input";
        return HS_ERR_BAD_ARG;
    }
    if (hsw::overlap(lse, lse_bytes, y, y_bytes)) {
        why = "lse overlaps y";
        return HS_ERR_BAD_ARG;
    }
    return HS_OK;
}

// hsat_forward_device's arguments
inline int check_forward(uint32_t num_rows, uint32_t num_cols, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, uint32_t d, float scale,
                         const float* y, uint64_t ldy, const float* lse, std::string& why) {
    if (int rc = hsw::check_d(d, why)) return rc;
    if (int rc = hsw::check_features("q", q, ldq, d, why)) return rc;
    if (int rc = hsw::check_features("k", k, ldk, d, why)) return rc;
    if (int rc = hsw::check_features("v", v, ldv, d, why)) return rc;
    if (int rc = hsw::check_features("y", y, ldy, d, why)) return rc;
    if (lse)
        if (int rc = hsw::check_entries("lse", lse, why)) return rc;
    if (int rc = check_scale(scale, why)) return rc;
    return check_overlaps(q, reach(num_rows, ldq, d), k, reach(num_cols, ldk, d), v, reach(num_cols, ldv, d), y, reach(num_rows, ldy, d), lse, uint64_t(num_rows) * 4, why);
}

// hsat_forward's: ld = d, no alignment rule (both implementations copy or walk the arrays as they are)
inline int check_forward_host(uint32_t num_rows, uint32_t num_cols, const float* q, const float* k, const float* v, uint32_t d, float scale, const float* y, const float* lse,
                              std::string& why) {
    if (int rc = hsw::check_d(d, why)) return rc;
    if (!q || !k || !v || !y) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = check_scale(scale, why)) return rc;
    return check_overlaps(q, uint64_t(num_rows) * d * 4, k, uint64_t(num_cols) * d * 4, v, uint64_t(num_cols) * d * 4, y, uint64_t(num_rows) * d * 4, lse, uint64_t(num_rows) * 4, why);
}

}  // namespace hsat
}  // namespace hisparse

#endif  // HISPARSE_HSAT_COMMON_H_
