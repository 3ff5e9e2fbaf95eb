// heads16_dropout_attention.h — the launchers of the three kernels of the multi-head attention step with bf16 operands, an optional
// per-entry bias and dropout on the attention weights (heads16_dropout_attention.hip), called by hsmh_api.cpp.  The schedule is the one of
// wide_products.h, unchanged and taken at the row's size in 16-byte chunks exactly as heads16_attention.h takes it: a row of heads * d
// bf16 elements is scheduled as a row of heads * d / 2 words.  d is a power of two from 8 to 256 and heads * d <= 512.  Feature operands
// are bf16 bit patterns in uint16_t, every feature ld is in ELEMENTS; lse, bias (may be nullptr) and gbias (may be nullptr) are fp32 and
// the D words double, as in heads_dropout_attention.h, so the two precisions share them; dr is philox.h's (hsmh_common.h checks all of it
// before a launch).
#ifndef HISPARSE_HEADS16_DROPOUT_ATTENTION_KERNELS_H_
#define HISPARSE_HEADS16_DROPOUT_ATTENTION_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "philox.h"
#include "wide_products.h"

namespace hisparse {
namespace dev {

// Forward, over the pattern itself: heads16_attention.h's forward with t = fl32(fl32(scale * s) + bias) and Y = c * (sum over the KEPT
// entries) / l, rounded to fp32 and then to bf16; l and lse over all entries.
hipError_t launch_bf16_drop_forward(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const float* bias,
                                    uint64_t ldb, uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr, uint16_t* y, uint64_t ldy, float* lse, uint64_t ldl,
                                    hipStream_t stream);

// Backward, row side, over the pattern itself: gQ and the D words, dsum[r * ldd + h], with GP -> w GP, w = keep ? c : 0 keyed by the entry's index.
hipError_t launch_bf16_drop_rows(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                 uint64_t ldgy, const float* lse, uint64_t ldl, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d, float scale, const philox::Dropout& dr,
                                 uint16_t* gq, uint64_t ldgq, double* dsum, uint64_t ldd, hipStream_t stream);

// Backward, column side, over the transposed pattern: gK, gV (weighed with w P) and, where gbias is not nullptr, gbias[perm[e'] * ldgb + h]
// = P (w GP - D) in fp32.  s.perm[e'] is the CSR index of the transposed pattern's entry e' (the entry map; required here: it keys the draw).
hipError_t launch_bf16_drop_cols(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                 uint64_t ldgy, const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, const float* bias, uint64_t ldb, uint32_t heads, uint32_t d,
                                 float scale, const philox::Dropout& dr, uint16_t* gk, uint64_t ldgk, uint16_t* gv, uint64_t ldgv, float* gbias, uint64_t ldgb, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_HEADS16_DROPOUT_ATTENTION_KERNELS_H_
