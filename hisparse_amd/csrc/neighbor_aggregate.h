// neighbor_aggregate.h — launchers of the neighbour aggregation's kernels (neighbor_aggregate.hip), called by hsw_api.cpp for
// include/hisparse_aggregate.h.  The schedule, its constants and the sides are wide_products.h's, unchanged.
#ifndef HISPARSE_NEIGHBOR_AGGREGATE_H_
#define HISPARSE_NEIGHBOR_AGGREGATE_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// the aggregators of one launch: sum (mean: the sum over the row's length), max, min; at least one of them
struct AggregateOps {
    bool sum = false, mean = false, max = false, min = false;
};

// ysum[r][j] = sum (mean) of X[idx[e]][j] over the entries of row r of s, ymax / ymin their extremes and amax / amin (may be nullptr) the
// winners' entry indices; a row without entries is +0.0f and ~0u.  Outputs whose aggregator is not asked for are not touched.
hipError_t launch_neighbor_forward(const WideSide& s, AggregateOps ops, const float* x, uint64_t ldx, uint32_t d, float* ysum, float* ymax, uint32_t* amax, float* ymin,
                                   uint32_t* amin, uint64_t ldy, hipStream_t stream);
// s is the transposed side (s.perm: the CSR index of every entry): gx[c][j] = the sum over the entries k of column c, r = idx[k], of
// gsum[r][j] (mean: / the length of row r, from row_ptr) + gmax[r][j] where amax[r][j] == perm[k] + gmin[r][j] where amin[r][j] == perm[k]
hipError_t launch_neighbor_backward(const WideSide& s, const uint32_t* row_ptr, AggregateOps ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin,
                                    const uint32_t* amin, uint64_t ldg, uint32_t d, float* gx, uint64_t ldgx, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_NEIGHBOR_AGGREGATE_H_
