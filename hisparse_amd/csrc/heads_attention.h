// heads_attention.h — the launchers of the three kernels of the multi-head attention step (heads_attention.hip), called by hsmh_api.cpp.
// The schedule is the one of wide_products.h, unchanged and taken at the width heads * d: its classes, its teams, its grid cap and its
// entries per trip.  d is a power of two from 4 to 256 and heads * d <= 256 (hsmh_common.h checks both before a launch).
#ifndef HISPARSE_HEADS_ATTENTION_KERNELS_H_
#define HISPARSE_HEADS_ATTENTION_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// Forward, over the pattern itself.  Per head h, on words h d ... h d + d - 1: Y[r] = the softmax of scale * (Q[r] . K[idx[e]]) over the
// row's entries times V[idx[e]], lse[r * ldl + h] = the row's log-sum-exp (lse may be nullptr).  Rows without entries: zeros and -inf.
hipError_t launch_heads_forward(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, uint32_t heads, uint32_t d, float scale,
                                float* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream);

// Backward, row side, over the pattern itself: gQ and the D words, dsum[r * ldd + h], per head as attention_backward.h's row side.
hipError_t launch_heads_backward_rows(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                      const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float scale, float* gq, uint64_t ldgq, double* dsum, uint64_t ldd,
                                      hipStream_t stream);

// Backward, column side, over the transposed pattern (s.ptr = column pointers, s.idx = the row of every entry in column order, s.list =
// the columns by length class): gK and gV per head as attention_backward.h's column side; dsum is what the row side wrote.
hipError_t launch_heads_backward_cols(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                      const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float scale, float* gk, uint64_t ldgk, float* gv,
                                      uint64_t ldgv, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_HEADS_ATTENTION_KERNELS_H_
