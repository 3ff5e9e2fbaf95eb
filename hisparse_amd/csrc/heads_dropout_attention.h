// heads_dropout_attention.h — the launchers of the three kernels of the multi-head attention step with dropout on the attention weights
// (heads_dropout_attention.hip), called by hsmh_api.cpp.  The schedule is the one of wide_products.h, unchanged and taken at the width
// heads * d, exactly as heads_bias_attention.h takes it.  bias (may be nullptr: the score is then the plain calls') and gbias (may be
// nullptr) are fp32 [entry][head] in the CSR order of the pattern, rows of ldb and ldgb words; d is a power of two from 4 to 256 and
// heads * d <= 256; dr holds the key, the offset words, the threshold and c of philox.h (hsmh_common.h checks all of it before a launch).
#ifndef HISPARSE_HEADS_DROPOUT_ATTENTION_KERNELS_H_
#define HISPARSE_HEADS_DROPOUT_ATTENTION_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "philox.h"
#include "wide_products.h"

namespace hisparse {
namespace dev {

// Forward, over the pattern itself: heads_bias_attention.h's forward with Y = c * (sum over the KEPT entries) / l; l and lse over all entries.
hipError_t launch_dropout_forward(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* bias, uint64_t ldb,
                                  uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr, float* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream);

// Backward, row side, over the pattern itself: gQ and the D words, dsum[r * ldd + h], with GP -> w GP, w = keep ? c : 0 keyed by the entry's index.
hipError_t launch_dropout_rows(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                               const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr, float* gq,
                               uint64_t ldgq, double* dsum, uint64_t ldd, hipStream_t stream);

// Backward, column side, over the transposed pattern: gK, gV (weighed with w P) and, where gbias is not nullptr, gbias[perm[e'] * ldgb + h]
// = P (w GP - D).  s.perm[e'] is the CSR index of the transposed pattern's entry e' (the entry map; required here: it keys the draw).
hipError_t launch_dropout_cols(const WideSide& s, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                               const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale,
                               const philox::Dropout& dr, float* gk, uint64_t ldgk, float* gv, uint64_t ldgv, float* gbias, uint64_t ldgb, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_HEADS_DROPOUT_ATTENTION_KERNELS_H_
