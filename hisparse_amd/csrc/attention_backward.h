// attention_backward.h — the launchers of the two kernels of the fused attention backward step (attention_backward.hip), called by
// hsab_api.cpp.  The schedule is the one of wide_products.h, unchanged: its classes, its teams, its grid cap and its entries per trip.
#ifndef HISPARSE_ATTENTION_BACKWARD_KERNELS_H_
#define HISPARSE_ATTENTION_BACKWARD_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// Row side, over the pattern itself (s.idx = the column of every entry).  With P[e] = exp(scale * (Q[r] . K[idx[e]]) - lse[r]) and
// GP[e] = gY[r] . V[idx[e]]:  dsum[r] = sum_{e in row r} P[e] GP[e]  and  gQ[r] = scale * sum_{e in row r} P[e] (GP[e] - dsum[r]) K[idx[e]].
// Rows without entries are written as zeros (gQ and dsum).  s.perm is not used.
hipError_t launch_attention_backward_rows(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                          const float* lse, uint32_t d, float scale, float* gq, uint64_t ldgq, double* dsum, hipStream_t stream);

// Column side, over the transposed pattern (s.ptr = column pointers, s.idx = the row of every entry in column order, s.list = the columns
// by length class).  dsum is what the row side wrote.  gK[c] = sum_{col(e) = c} scale P[e] (GP[e] - dsum[row(e)]) Q[row(e)] and
// gV[c] = sum_{col(e) = c} P[e] gY[row(e)].  Columns without entries are written as zeros.  s.perm is not used.
hipError_t launch_attention_backward_cols(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                                          const float* lse, const double* dsum, uint32_t d, float scale, float* gk, uint64_t ldgk, float* gv, uint64_t ldgv, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_ATTENTION_BACKWARD_KERNELS_H_
