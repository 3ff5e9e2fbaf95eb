/* hisparse_heads_dropout_bf16.h — bf16 OPERANDS for the calls with a bias and dropout of the multi-head attention object of
 * hisparse_heads.h (EXTENSION; no reference counterpart).
 *
 * Four more calls on the EXISTING object hsmh_pattern; there is no new create, flag, object field, allocation or atomic.  They are
 * the calls of hisparse_heads_dropout.h -- an optional per-entry, per-head additive bias on the score, dropout on the attention weights
 * after the softmax, the mask recomputed and never stored -- over the bf16 feature operands of hisparse_heads_bf16.h:
 *     hsmhd16_forward_device    Y (bf16), lse (fp32)   from   Q, K, V (bf16), bias (fp32, may be NULL), drop_p, seed, offset
 *     hsmhd16_backward_device   gQ, gK, gV (bf16), gbias (fp32, may be NULL)   from   Q, K, V, gY (bf16), lse (fp32), bias (may be NULL),
 *                               drop_p, seed, offset
 * One family with the bias optional covers bf16 + bias (drop_p = 0), bf16 + dropout (bias NULL) and bf16 + both.  A graph transformer
 * that trains under autocast with an edge-encoding bias and attention dropout stays in bf16: no operand is widened and no result
 * narrowed, the gathered rows are half as wide, and heads * d reaches 512.  Same library (libhisparse_hip.so; libhisparse_cpu.so
 * exports the same four symbols on the host: plain loops, the same roundings -- a second implementation, never a fallback).
 *
 * FORMULAS: those of hisparse_heads_dropout.h applied to the operands widened to fp32, which is exact.  Per row r, head h and entry e,
 *     t = fl32(fl32(scale * s) + bias[e][h])   (fl32(scale * s) when bias is NULL),   P = softmax_row(t),
 *     P' = w P,   w = keep(e, h) ? c : 0,   c = 1 / (1 - drop_p) formed in double and applied once,
 *     Y[r][h] = sum_e P' V[col(e)][h];   lse is the log-sum-exp of ALL the row's entries: the words of the call without dropout.
 *     GP = w (gY[r] . V[c]),   D = sum_e P GP,   GS = scale P (GP - D),   gQ = sum GS K,   gK = sum GS Q,   gV[c] = sum_e w P gY[r],
 *     gbias = P (GP - D)      (a dropped entry's gbias word is -P D, not zero)
 *   All sums are in double.  THE KEEP DECISION is hisparse_heads_dropout.h's, word for word: Philox4x32-10 keyed by seed, offset, the
 *   entry's index in the caller's CSR order and the head; hsmhd_keep_mask of that header gives the mask of a call of this one.  The
 *   backward must be given the drop_p, seed and offset of the forward whose lse it is given.
 *
 * ELEMENT TYPES: Q, K, V, gY, Y, gQ, gK and gV are bf16, bit patterns in uint16_t.  bias and gbias stay fp32 [entry][head]: they are the
 *   small stream (heads * 4 bytes per entry against 4 * heads * d bytes of gathered K and V rows), gbias feeds an fp32 table, and fp32
 *   keeps t the fp32 family's own expression.  lse is fp32 [row][head] and D double inside the object.  CROSS-PRECISION: lse of
 *   hsmhd16_forward* may feed hsmhd_backward* (on the operands widened) and lse of hsmhd_forward* may feed hsmhd16_backward*; the draws are
 *   the same in both, because they depend only on (seed, offset, e, h).  ONE BACKWARD CALL MAY BE IN FLIGHT PER OBJECT, whichever family.
 *
 * SHAPES, LAYOUT, ALIGNMENT, OVERLAP: hisparse_heads_bf16.h's for the features -- d in {8, 16, 32, 64, 128, 256}, 1 <= heads <=
 *   max_heads, heads * d <= 512, every feature ld in ELEMENTS, a multiple of 8 and at least heads * d, feature pointers 16-byte aligned,
 *   a feature operand of n rows reaching ((n - 1) * ld + heads * d) * 2 bytes -- and hisparse_heads_bias.h's for lse, bias and gbias (ldb
 *   and ldgb are not read where the pointer is NULL).  An output may not share a byte with an input or another output.  scale must be
 *   finite; drop_p a float, finite and in [0, 1), as hsmhd_* checks it.  WHICH OBJECT: the forward runs on ANY hsmh_pattern; the backward
 *   needs THE ENTRY MAP, with or without a bias: on an object without it (from the plain create, or from hsmhb_create without HSMH_BACKWARD)
 *   it is HS_ERR_BAD_ARG and the message names hsmhb_create.  Every breach is HS_ERR_BAD_ARG, the object's last-error string says why, and the object
 *   stays usable.  hsmhd16_forward_device is ONE kernel launch and hsmhd16_backward_device exactly TWO on the object's stream; neither
 *   allocates or synchronises.  The object's info is unchanged by the calls.
 * hsmhd16_forward / hsmhd16_backward: the host-pointer forms, ld = heads * d for the features, ld = heads for lse, bias and gbias, no
 *   alignment rule beyond the element's; synchronous; their transient device buffers are the only allocations.
 *
 * DEGENERACIES, BIT FOR BIT: with drop_p = 0 and bias NULL every output word equals that of hsmh16_forward_device /
 *   hsmh16_backward_device; with drop_p = 0 and a bias of all +0.0 the same holds (thr = 0 keeps every entry, c = 1.0 and x * 1.0 = x,
 *   t + 0.0 has t's value; the schedule and the order of every sum are those of hisparse_heads_bf16.h's kernels).
 *
 * SPECIAL ROWS AND VALUES: the tables of hisparse_heads_bias.h and hisparse_heads_dropout.h; the outputs are bf16 words.  A row without
 *   entries, and a head of a row whose kept set is empty (FULLY DROPPED), give the word 0x0000 in Y, with lse -inf and as without dropout
 *   respectively; a column without entries is 0x0000 in gK and gV.  NaN stays NaN.  A bias of -inf masks the entry and renormalises the
 *   row as in hisparse_heads_dropout.h.
 * ARITHMETIC: each bf16 output word is rounded to fp32 and then from fp32 to bf16, round to nearest even, as in hisparse_heads_bf16.h;
 *   lse and gbias words are rounded once to fp32.  ERROR BOUND: where hsmhd_* (on the widened operands) bounds a bf16-typed output word x
 *   by b, this call bounds it by
 *       b + 2^-8 (|x| + b) + 2^-134
 *   and lse and gbias keep their fp32 bounds.  No new constant is introduced.
 *
 * HOW THE WORK IS SCHEDULED: the three kernels of hisparse_heads_bf16.h (a lane owning one 16-byte chunk of EIGHT elements, the schedule
 *   of hisparse_wide.h taken at the row's size in 16-byte chunks) with the bias, the draws and the entry map of hisparse_heads_dropout.h's
 *   kernels (heads16_dropout_attention.hip).  A head is d / 8 lanes.  Where a head has at least four lanes (d >= 32) lane i of each four
 *   loads the bias word and draws for the trip's entry i alone, and one ballot of the wavefront hands the bits out.  Below that width a
 *   lane loads the bias words of its four entries itself but still draws once per trip: one generator call yields the words of four
 *   heads, so lane i of four neighbouring lanes (chunks of one such four heads) draws entry i and four ballots hand the bits out.  The
 *   column side reads an entry's CSR index from the entry map it streams anyway.
 * COST (MI355X; tools/heads16_dropout_times.py, profiles/heads16_dropout_times.txt; DESIGN.md section 6c-bf16 has the table): this call
 *   against (a) hsmhd_* with fp32 operands and (b) hsmh16_* without bias and dropout, on the SAME object in the same run, drop_p = 0.1,
 *   bias and gbias given, forward / backward.  ogbl-ppa (576 K rows, 42.5 M entries), 4 heads of d = 16: 3306 / 9892 us against (a)
 *   3660 / 11739 us (0.90 / 0.84) and (b) 2935 / 6459 us (1.13 / 1.53); 8 heads of d = 16: (a) 0.73 / 0.78; 4 heads of d = 64: 9547 /
 *   26141 us, (a) 0.62 / 0.61, (b) 1.04 / 1.29; 2 heads of d = 128: (a) 0.60 / 0.61; 8 heads of d = 64, which fp32 cannot take: 18865 /
 *   50190 us, (b) 1.04 / 1.25.  transformer-50: (a) 0.58 to 0.71 forward, 0.59 to 0.77 backward.  No shape came out slower than fp32.
 *   Ratio (b) is above the fp32 family's 1.07 to 1.10 forward and 1.01 to 1.03 backward because it is taken against calls WITHOUT a
 *   bias: it also holds the bias stream and, on the column side, the gathered bias words and the scattered gbias words.  The kernels run
 *   two wavefronts per SIMD as the bf16 kernels do (226 / 209 / 253 VGPRs against 216 / 187 / 227), without scratch and with no more
 *   LDS than theirs. */
#ifndef HISPARSE_HEADS_DROPOUT_BF16_H_
#define HISPARSE_HEADS_DROPOUT_BF16_H_

#include "hisparse_heads.h"

#ifdef __cplusplus
extern "C" {
#endif

int hsmhd16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv,
                           const float* bias_dev /* may be NULL */, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset,
                           uint16_t* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsmhd16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const float* bias /* may be NULL */, uint32_t heads, uint32_t d, float scale,
                    float drop_p, uint64_t seed, uint64_t offset, uint16_t* y, float* lse /* may be NULL */); /* host pointers, ld = heads * d, ldl = ldb = heads, synchronous */
int hsmhd16_backward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const uint16_t* gy_dev,
                            uint64_t ldgy, const float* lse_dev, uint64_t ldl, const float* bias_dev /* may be NULL */, uint64_t ldb, uint32_t heads, uint32_t d, float scale,
                            float drop_p, uint64_t seed, uint64_t offset, uint16_t* gq_dev, uint64_t ldgq, uint16_t* gk_dev, uint64_t ldgk, uint16_t* gv_dev, uint64_t ldgv,
                            float* gbias_dev /* may be NULL */, uint64_t ldgb);
int hsmhd16_backward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy, const float* lse, const float* bias /* may be NULL */,
                     uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, uint16_t* gq, uint16_t* gk, uint16_t* gv,
                     float* gbias /* may be NULL */); /* host pointers, ld = heads * d, ldl = ldb = ldgb = heads, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_HEADS_DROPOUT_BF16_H_ */
