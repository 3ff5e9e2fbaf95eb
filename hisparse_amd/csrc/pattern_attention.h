// pattern_attention.h — the launcher of the fused attention kernel (pattern_attention.hip), called by hsat_api.cpp.  The schedule is the one
// of wide_products.h, unchanged: its classes, its teams, its grid cap and its entries per trip.
#ifndef HISPARSE_PATTERN_ATTENTION_H_
#define HISPARSE_PATTERN_ATTENTION_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// Y[r] = sum_{e in row r} P[e] V[idx[e]], P = the row softmax of scale * (Q[r] . K[idx[e]]); lse[r] = the row's log-sum-exp (lse may be
// nullptr).  Rows without entries are written as zeros and -inf: a pattern without entries is launched too.  s.perm is not used.
hipError_t launch_pattern_attention(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, uint32_t d, float scale, float* y,
                                    uint64_t ldy, float* lse, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_PATTERN_ATTENTION_H_
