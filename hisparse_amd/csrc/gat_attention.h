// gat_attention.h — the launchers of the three kernels of the graph attention (GAT) step over a CSR pattern (gat_attention.hip), called by
// hsmh_api.cpp.  The schedule is the one of wide_products.h, unchanged and taken at the width heads * d, exactly as heads_attention.h
// takes it.  el, gel and lse are fp32 [row][head], er and ger fp32 [column][head], rows of their own ld words; d is a power of two from 4
// to 256 and heads * d <= 256 (hsmh_common.h checks all of it before a launch).
#ifndef HISPARSE_GAT_ATTENTION_KERNELS_H_
#define HISPARSE_GAT_ATTENTION_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// Forward, over the pattern itself: x = el[r][h] + er[c][h], t = x > 0 ? x : slope * x (two fp32 operations), Y and lse (may be nullptr).
hipError_t launch_gat_forward(const WideSide& s, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, uint32_t heads, uint32_t d, float slope,
                              float* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream);

// Backward, row side, over the pattern itself: gel and the D words, dsum[r * ldd + h].
hipError_t launch_gat_backward_rows(const WideSide& s, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                    const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gel, uint64_t ldgel, double* dsum, uint64_t ldd,
                                    hipStream_t stream);

// Backward, column side, over the transposed pattern: ger and gV, from the D words of the row side.
hipError_t launch_gat_backward_cols(const WideSide& s, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                    const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float slope, float* ger, uint64_t ldger, float* gv,
                                    uint64_t ldgv, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_GAT_ATTENTION_KERNELS_H_
