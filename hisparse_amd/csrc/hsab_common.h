// hsab_common.h — what the two implementations of include/hisparse_attention_backward.h share (hsab_api.cpp on the HIP runtime,
// hsab_cpu.cpp on the host): the argument checks, so that both refuse the same calls with the same codes.  Built from hsat_common.h's
// checks (the pattern, scale, the reach of an operand) and hsw_common.h's checks of one operand.  Host code only.
#ifndef HISPARSE_HSAB_COMMON_H_
#define HISPARSE_HSAB_COMMON_H_

#include <cstdint>
#include <string>

#include "hisparse_attention_backward.h"
#include "hsat_common.h"

namespace hisparse {
namespace hsab {

// hsab_create's arguments and the pattern itself: hsat_create's check
inline int check_create(uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, std::string& why) {
    return hsat::check_create(num_rows, num_cols, indptr, indices, why);
}

struct Range {
    const char* name;
    const void* p;
    uint64_t bytes;
};

// each of the three outputs against the five inputs and against the other outputs
inline int check_overlaps(const Range (&in)[5], const Range (&out)[3], std::string& why) {
    for (const Range& o : out) {
        for (const Range& i : in) {
            if (hsw::overlap(o.p, o.bytes, i.p, i.bytes)) {
                why = std::string(o.name) + " overlaps " + i.name;
                return HS_ERR_BAD_ARG;
            }
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = a + 1; b < 3; ++b) {
            if (hsw::overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) {
                why = std::string(out[a].name) + " overlaps " + out[b].name;
                return HS_ERR_BAD_ARG;
            }
        }
    }
    return HS_OK;
}

// hsab_backward_device's arguments
inline int check_backward(uint32_t num_rows, uint32_t num_cols, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                          const float* lse, uint32_t d, float scale, const float* gq, uint64_t ldgq, const float* gk, uint64_t ldgk, const float* gv, uint64_t ldgv, std::string& why) {
    if (int rc = hsw::check_d(d, why)) return rc;
    if (int rc = hsw::check_features("q", q, ldq, d, why)) return rc;
    if (int rc = hsw::check_features("k", k, ldk, d, why)) return rc;
    if (int rc = hsw::check_features("v", v, ldv, d, why)) return rc;
    if (int rc = hsw::check_features("gy", gy, ldgy, d, why)) return rc;
    if (int rc = hsw::check_entries("lse", lse, why)) return rc;
    if (int rc = hsw::check_features("gq", gq, ldgq, d, why)) return rc;
    if (int rc = hsw::check_features("gk", gk, ldgk, d, why)) return rc;
    if (int rc = hsw::check_features("gv", gv, ldgv, d, why)) return rc;
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const Range in[5] = {{"q", q, hsat::reach(num_rows, ldq, d)}, {"k", k, hsat::reach(num_cols, ldk, d)}, {"v", v, hsat::reach(num_cols, ldv, d)},
                         {"gy", gy, hsat::reach(num_rows, ldgy, d)}, {"lse", lse, uint64_t(num_rows) * 4}};
    const Range out[3] = {{"gq", gq, hsat::reach(num_rows, ldgq, d)}, {"gk", gk, hsat::reach(num_cols, ldgk, d)}, {"gv", gv, hsat::reach(num_cols, ldgv, d)}};
    return check_overlaps(in, out, why);
}

// hsab_backward's: ld = d, no alignment rule (both implementations copy or walk the arrays as they are)
inline int check_backward_host(uint32_t num_rows, uint32_t num_cols, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t d, float scale,
                               const float* gq, const float* gk, const float* gv, std::string& why) {
    if (int rc = hsw::check_d(d, why)) return rc;
    if (!q || !k || !v || !gy || !lse || !gq || !gk || !gv) {
        why = "null argument";
        return HS_ERR_BAD_ARG;
    }
    if (int rc = hsat::check_scale(scale, why)) return rc;
    const uint64_t rb = uint64_t(num_rows) * d * 4, cb = uint64_t(num_cols) * d * 4;
    const Range in[5] = {{"q", q, rb}, {"k", k, cb}, {"v", v, cb}, {"gy", gy, rb}, {"lse", lse, uint64_t(num_rows) * 4}};
    const Range out[3] = {{"gq", gq, rb}, {"gk", gk, cb}, {"gv", gv, cb}};
    return check_overlaps(in, out, why);
}

}  // namespace hsab
}  // namespace hisparse

#endif  // HISPARSE_HSAB_COMMON_H_
