// heads16_attention.h — the launchers of the three kernels of the multi-head attention step with bf16 operands (heads16_attention.hip),
// called by hsmh_api.cpp.  The schedule is the one of wide_products.h, unchanged and taken at the row's size in 16-byte chunks: a chunk
// holds eight bf16 elements, so a row of heads * d elements is scheduled as a row of heads * d / 2 words.  d is a power of two from 8 to
// 256 and heads * d <= 512 (hsmh_common.h checks both before a launch).  Feature operands are bf16 bit patterns in uint16_t, every ld is
// in ELEMENTS; lse is fp32 and the D words are double, exactly as in heads_attention.h, so the two precisions share both.
#ifndef HISPARSE_HEADS16_ATTENTION_KERNELS_H_
#define HISPARSE_HEADS16_ATTENTION_KERNELS_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// Forward, over the pattern itself.  Per head h, on elements h d ... h d + d - 1: Y[r] = the softmax of scale * (Q[r] . K[idx[e]]) over the
// row's entries times V[idx[e]], rounded to fp32 and then to bf16; lse[r * ldl + h] = the row's log-sum-exp in fp32 (lse may be nullptr).
// Rows without entries: 0x0000 and -inf.
hipError_t launch_heads16_forward(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, uint32_t heads, uint32_t d,
                                  float scale, uint16_t* y, uint64_t ldy, float* lse, uint64_t ldl, hipStream_t stream);

// Backward, row side, over the pattern itself: gQ and the D words, dsum[r * ldd + h], per head as heads_attention.h's row side.
hipError_t launch_heads16_backward_rows(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                        uint64_t ldgy, const float* lse, uint64_t ldl, uint32_t heads, uint32_t d, float scale, uint16_t* gq, uint64_t ldgq, double* dsum, uint64_t ldd,
                                        hipStream_t stream);

// Backward, column side, over the transposed pattern: gK and gV per head as heads_attention.h's column side; dsum is what the row side wrote.
hipError_t launch_heads16_backward_cols(const WideSide& s, const uint16_t* q, uint64_t ldq, const uint16_t* k, uint64_t ldk, const uint16_t* v, uint64_t ldv, const uint16_t* gy,
                                        uint64_t ldgy, const float* lse, uint64_t ldl, const double* dsum, uint64_t ldd, uint32_t heads, uint32_t d, float scale, uint16_t* gk,
                                        uint64_t ldgk, uint16_t* gv, uint64_t ldgv, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_HEADS16_ATTENTION_KERNELS_H_
