/* hisparse_heads_bf16.h — bf16 OPERANDS for the multi-head attention object of hisparse_heads.h (EXTENSION; no reference counterpart).
 *
 * Four more calls on the EXISTING object hsmh_pattern: the same pattern, the same transposed pattern, the same D words and the same
 * stream.  Nothing of an object is held twice for a caller who mixes precisions; hsmh_create, hsmh_destroy, hsmh_last_error, hsmh_info,
 * hsmh_set_stream and hsmh_sync are hisparse_heads.h's.  The formulas are that header's, per head:
 *     hsmh16_forward_device    Y: num_rows x ldy (bf16) and lse: num_rows x ldl (fp32)   from   Q: num_rows rows, K, V: num_cols rows (bf16)
 *     hsmh16_backward_device   gQ: num_rows x ldgq, gK: num_cols x ldgk, gV: num_cols x ldgv (bf16)   from   Q, gY, K, V (bf16) and lse (fp32)
 * Under autocast Q, K, V and g_Y are bf16 tensors; these calls take them as they are where the fp32 calls need four operands widened and
 * four results narrowed per layer and step.
 *
 * ELEMENT TYPES: Q, K, V, gY, Y, gQ, gK and gV are bf16, passed as bit patterns in uint16_t (the upper half of the fp32 of the same
 *   value).  lse stays fp32 [row][head] and D stays double inside the object, exactly as in hisparse_heads.h, so A FORWARD IN ONE
 *   PRECISION MAY BE FOLLOWED BY A BACKWARD IN THE OTHER: the lse words are the same kind.  ONE BACKWARD CALL MAY BE IN FLIGHT PER OBJECT,
 *   whichever precision it is (the D words are shared).  Same library (libhisparse_hip.so; libhisparse_cpu.so exports the same four
 *   symbols on the host: plain loops, two passes per row, the same two roundings -- a second implementation, never a fallback).
 *
 * SHAPES ACCEPTED: d in {8, 16, 32, 64, 128, 256} (a head is a power-of-two number of 16-byte chunks of 8 elements), 1 <= heads <=
 *   max_heads and heads * d <= 512: a row is at most 1 KiB and at most 64 chunks, the same widest group as fp32.  Anything else is
 *   HS_ERR_BAD_ARG; the message names the rule and points to the fp32 calls, which take d = 4.  heads, d, scale and the precision may
 *   change from call to call.
 *
 * LAYOUT of the _device calls.  Element j of head h of row i of a feature operand sits at i * ld + h * d + j; ld is in ELEMENTS.  The
 *   feature pointers are 16-byte aligned, every ld is a multiple of 8 and at least heads * d.  Elements heads * d ... ld - 1 of an input
 *   row may be loaded but reach no result: a NaN there (0x7FC0) changes nothing.  Elements heads * d ... ld - 1 of an output row are not
 *   written.  lse of (row r, head h) sits at r * ldl + h, ldl >= heads, 4-byte aligned, may be NULL in the forward and is REQUIRED in
 *   the backward.  A feature operand of n rows reaches from its pointer to the end of the 16-byte chunk that holds its last element,
 *   ((n - 1) * ld + heads * d) * 2 bytes; lse reaches ((num_rows - 1) * ldl + heads) * 4 bytes.  An output (lse of the forward among
 *   them) may not share a byte with an input or with another output; ranges that touch are fine.  scale must be finite.  The backward
 *   needs an object created with HSMH_BACKWARD.  Every breach is HS_ERR_BAD_ARG, hsmh_last_error(p) says why, and the object stays usable
 *   for both precisions.  hsmh16_forward_device is ONE kernel launch and hsmh16_backward_device exactly TWO on the object's stream; neither
 *   allocates or synchronises, and both can be captured into a graph (one linear branch).
 * hsmh16_forward / hsmh16_backward: the host-pointer forms, ld = heads * d exactly for every feature array and ldl = heads, no alignment
 *   rule beyond the element's; they copy in, run, copy out; synchronous; their transient device buffers are the only allocations.
 *
 * ARITHMETIC: the ARITHMETIC block of hisparse_heads.h applied to the operands widened to fp32, which is exact.  One fp32 multiply per
 *   product (the product of two bf16 numbers is exact in fp32), the d products of a head and entry added in double in any order, s
 *   rounded once to fp32, t = scale * s one fp32 multiply, everything after that in double with the library's exp and log.  EACH OUTPUT
 *   WORD IS ROUNDED TO fp32 AND THEN FROM fp32 TO bf16, ROUND TO NEAREST EVEN; both roundings are part of the contract.  NaN stays NaN,
 *   +-inf and the sign of zero survive the rounding.  Where the fp32 call bounds an output word x by b, this call bounds it by
 *       b + 2^-8 (|x| + b) + 2^-134
 *   (half a bf16 ulp is 2^-8 relative, half the bf16 subnormal spacing is 2^-134).  lse keeps its fp32 bound unchanged.
 *
 * SPECIAL ROWS AND VALUES: the tables of hisparse_heads.h, per head; HEADS DO NOT LEAK.  A row without entries is the word 0x0000 in all
 *   heads * d elements of Y and of gQ and -inf in all heads words of lse; a column without entries is 0x0000 in gK and gV.  Every output
 *   word has exactly one writer and there are no atomics: two calls with the same inputs give the same words.
 *
 * HOW THE WORK IS SCHEDULED: the three kernels of hisparse_heads.h with a lane owning one 16-byte chunk of EIGHT elements: the schedule
 *   of hisparse_wide.h taken at the row's size in 16-byte chunks, so the lane group of a row is half as wide as in fp32 and a wavefront
 *   holds twice the entries in flight per trip.  The d / 8 lanes of a head add the head's dots among themselves; where a head has at
 *   least four lanes (d >= 32) a trip's four weights are dealt one per lane.  Sums stay in double.  No matrix engine.
 *
 * COST (MI355X; tools/heads16_times.py, profiles/heads16_times.txt; DESIGN.md section 6b has the table and the bar): the bf16 call
 *   against the fp32 call of the SAME object in the same run, forward / backward.  ogbl-ppa (576 K rows, 42.5 M entries), 4 heads of
 *   d = 16: 2956 / 6533 us against 3405 / 7929 us (0.87 / 0.82); 8 heads of d = 16: 0.74 / 0.70; 4 heads of d = 64 and 2 of d = 128:
 *   0.62 / 0.61 and 0.62 / 0.62.  transformer-50: 0.62 to 0.75 forward, 0.59 to 0.74 backward.  No shape came out slower.  8 heads of
 *   d = 64, which fp32 cannot take: 18127 / 39906 us on ogbl-ppa.  The call still costs what its gathers of whole rows cost, now of
 *   heads * d * 2 bytes; halving a row that was two cache lines gains least.  The kernels run two wavefronts per SIMD (216 / 187 / 227
 *   VGPRs) where the fp32 kernels run three, three and two. */
#ifndef HISPARSE_HEADS_BF16_H_
#define HISPARSE_HEADS_BF16_H_

#include "hisparse_heads.h"

#ifdef __cplusplus
extern "C" {
#endif

int hsmh16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                          float scale, uint16_t* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsmh16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint32_t heads, uint32_t d, float scale, uint16_t* y,
                   float* lse /* may be NULL */); /* host pointers, ld = heads * d, ldl = heads, synchronous */
int hsmh16_backward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const uint16_t* gy_dev,
                           uint64_t ldgy, const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float scale, uint16_t* gq_dev, uint64_t ldgq, uint16_t* gk_dev, uint64_t ldgk,
                           uint16_t* gv_dev, uint64_t ldgv);
int hsmh16_backward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy, const float* lse, uint32_t heads, uint32_t d, float scale,
                    uint16_t* gq, uint16_t* gk, uint16_t* gv); /* host pointers, ld = heads * d, ldl = heads, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_HEADS_BF16_H_ */
