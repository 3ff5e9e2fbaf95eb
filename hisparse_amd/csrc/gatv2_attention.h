// gatv2_attention.h — the launchers of the four kernels of the GATv2 step over a CSR pattern (gatv2_attention.hip), called by
// hsmh_api.cpp.  The schedule is the one of wide_products.h, unchanged and taken at the width heads * d, exactly as heads_attention.h
// takes it.  XD, gY, Y and gXD are fp32 [row][head][feature], XS and gXS fp32 [column][head][feature], a and ga heads * d contiguous fp32
// words, lse fp32 [row][head]; d is a power of two from 4 to 256 and heads * d <= 256 (hsmh_common.h checks all of it before a launch).
#ifndef HISPARSE_GATV2_ATTENTION_KERNELS_H_
#define HISPARSE_GATV2_ATTENTION_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// Forward, over the pattern itself: z = XD[r] + XS[c], w = z > 0 ? z : slope * z, t = a[h] . w, Y and lse (may be nullptr).
hipError_t launch_gatv2_forward(const WideSide& s, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, uint32_t heads, uint32_t d, float slope, float* y,
                                uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream);

// The physical workgroups of the row side's launch at this width: the vectors of heads * d doubles it leaves in the workspace.
uint32_t gatv2_row_vectors(const WideSide& s, uint32_t heads, uint32_t d);

// Backward, row side, over the pattern itself: gXD, the D words dsum[r * ldd + h], and per physical workgroup one vector of heads * d
// doubles, work[block * heads * d + k], the workgroup's share of ga.
hipError_t launch_gatv2_backward_rows(const WideSide& s, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, const float* gy, uint64_t ldgy, const float* lse,
                                      uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gxd, uint64_t ldgxd, double* dsum, uint64_t ldd, double* work, hipStream_t stream);

// Backward, column side, over the transposed pattern: gXS, from the D words of the row side.
hipError_t launch_gatv2_backward_cols(const WideSide& s, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, const float* gy, uint64_t ldgy, const float* lse,
                                      uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float slope, float* gxs, uint64_t ldgxs, hipStream_t stream);

// ga[k] = the `vectors` workgroup vectors of the row side added in index order, rounded once.
hipError_t launch_gatv2_reduce(const double* work, uint32_t vectors, uint32_t width, float* ga, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_GATV2_ATTENTION_KERNELS_H_
