/* hisparse_heads_dropout.h — DROPOUT ON THE ATTENTION WEIGHTS for the multi-head attention object of hisparse_heads.h (EXTENSION; no
 * reference counterpart).
 *
 * Five more calls on the EXISTING object hsmh_pattern; there is no new create.  The formulas are those of hisparse_heads_bias.h (with
 * a bias) or hisparse_heads.h (bias NULL) with ONE change, after the softmax:
 *     P'[e][h] = w[e][h] * P[e][h],      w[e][h] = keep(e, h) ? c : 0,      c = 1 / (1 - drop_p), formed in double
 * which is what a model that trains with attention dropout needs and cannot build from outside: a bias of -inf renormalises the row,
 * and the fused calls never hold P.  NO MASK IS STORED: forward and backward recompute keep(e, h) from a counter-based generator, so
 * forward is still ONE launch, backward TWO, neither allocates or synchronises, and the library still builds no per-entry array.
 *     hsmhd_forward_device    Y and lse   from   Q, K, V, bias (may be NULL), drop_p, seed, offset
 *     hsmhd_backward_device   gQ, gK, gV and gbias (may be NULL)   from   Q, K, V, gY, lse, bias (may be NULL), drop_p, seed, offset
 *     hsmhd_keep_mask         the mask itself, on the host: how a caller or a test reproduces it
 * Same library (libhisparse_hip.so; libhisparse_cpu.so exports the same five symbols on the host: plain loops, the same roundings -- a
 * second implementation, never a fallback).
 *
 * FORWARD, per row r and head h, with t = fl32(fl32(scale * s) + bias) (or fl32(scale * s) when bias is NULL) and P = softmax_row(t):
 *     Y[r][h] = sum_e w P V[col(e)][h]
 *   lse is the log-sum-exp of ALL the row's entries: the same words as without dropout, so the backward and the merge of slabs by lse
 *    work as they did.
 * BACKWARD:
 *     GP = w (gY[r] . V[c]),   D[r][h] = sum_e P GP,   GS = scale P (GP - D),   gQ = sum GS K,   gK = sum GS Q,
 *     gV[c] = sum_e w P gY[r],   gbias = P (GP - D)      (a dropped entry's gbias word is -P D, not zero)
 *   The backward must be given the drop_p, seed and offset of the forward whose lse it is given.
 *
 * THE KEEP DECISION is fixed here so that every implementation agrees.  e is THE ENTRY'S INDEX IN THE CALLER'S CSR ORDER (the order of
 *   `indices` given to create; a pair held twice is two entries and two independent draws), h the head:
 *     x(e, h)    = word (h & 3) of Philox4x32-10( counter = (e, h >> 2, offset & 0xffffffff, offset >> 32),
 *                                                 key     = (seed & 0xffffffff, seed >> 32) )
 *     thr        = (uint32_t) floor((double) drop_p * 4294967296.0)
 *     keep(e, h) = x(e, h) >= thr
 *   Philox4x32-10 with the standard constants: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten
 *   rounds.  Known answers, counter ; key -> output:
 *     0 0 0 0 ; 0 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff ffffffff ffffffff ffffffff ; ffffffff ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344 ; a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   One generator call serves four heads of an entry.  A (seed, offset, e, h) used twice is the same decision twice: a caller advances
 *   offset per step and per layer.
 * drop_p is a float, finite and in [0, 1); anything else, 1.0 and NaN included, is HS_ERR_BAD_ARG with a message, and the object stays
 *   usable.
 *   CONSEQUENCE: with drop_p = 0, thr = 0 and c = 1.0, so every output word is BIT FOR BIT that of hsmhb_forward_device and
 *   hsmhb_backward_device with the same bias, and with bias NULL that of hsmh_forward_device and hsmh_backward_device (x * 1.0 = x; the
 *   schedule and the order of every sum are the same).
 *
 * WHICH OBJECT.  hsmhd_forward and hsmhd_forward_device run on ANY hsmh_pattern.  hsmhd_backward and hsmhd_backward_device need THE
 *   ENTRY MAP, with or without a bias (through it the column side names an entry as the forward did): on an object without it (from
 *   hsmh_create, or from hsmhb_create without HSMH_BACKWARD) they are HS_ERR_BAD_ARG and the message names hsmhb_create.  hsmh_info is
 *   unchanged; nothing is allocated.
 *
 * EVERYTHING ELSE is hisparse_heads_bias.h's: the layouts of the features, lse, bias and gbias (ldb and ldgb are not read where the
 *   pointer is NULL), the shapes accepted, the overlap rule, the stream rules, ONE BACKWARD IN FLIGHT PER OBJECT, one writer per output
 *   word and no atomics (two calls with the same inputs give the same words).  hsmhd_forward / hsmhd_backward are the host-pointer
 *   forms: ld = heads * d for the features, ld = heads for lse, bias and gbias; synchronous.
 * SPECIAL ROWS AND VALUES: the tables of hisparse_heads_bias.h decide P, and a dropped entry's weight is exactly 0, as a masked
 *   entry's is.  FULLY DROPPED ROW: a row with entries and a finite lse whose kept set is empty in a head gives +0.0 in that head's d
 *   words of Y, not NaN, and lse as without dropout.  A bias of -inf on an entry together with dropout computes what the pattern
 *   without that entry computes under the same draws for the remaining entries' indices OF THE ORIGINAL PATTERN.
 * ARITHMETIC: t as in hisparse_heads_bias.h (hisparse_heads.h when bias is NULL); the softmax sums l over all entries; c multiplies an
 *   entry's weight or an output word once, in double; one rounding per output word.  Against the bounds of hisparse_heads_bias.h: the
 *   forward's centred term rho / (1 - rho) sum P |V - Y| becomes 2 rho / (1 - rho) sum w P |V| (the kept weights no longer sum to one)
 *   and its summation term takes sum w P |V|; in the backward GP becomes w GP, gam becomes w gam + 2^-52 |w GP|, and gV takes w P for P.
 *
 * hsmhd_keep_mask(nnz, heads, drop_p, seed, offset, keep): a pure host function that needs no object and no device.  keep is uint8_t
 *   [entry][head], nnz * heads bytes, 1 = kept.  HS_ERR_BAD_ARG for a drop_p outside [0, 1), heads outside 1 ... 64, nnz above 2^32 or
 *   a NULL keep with nnz > 0.
 *
 * HOW THE WORK IS SCHEDULED: the three kernels of hisparse_heads_bias.h restated (heads_dropout_attention.hip) on the unchanged
 *   schedule of hisparse_wide.h.  Forward and row side know an entry's index; the column side reads it from the entry map, which it
 *   streams anyway.  Where a head has at least four lanes (d >= 16) lane i of each four draws for the trip's entry i alone, one generator
 *   call per lane and trip, and one ballot of the wavefront hands the bits out; below that width a lane draws for its four entries.
 * COST (MI355X; tools/heads_dropout_times.py, profiles/heads_dropout_times.txt; DESIGN.md section 6c has the table and the bar): the call
 *   against what a caller with attention dropout had to do before it -- the per-head chain of hisparse_heads_bias.h's COST paragraph with
 *   element-wise multiplies by a precomputed weight array, one per head forward and two backward, the array's generation not charged --
 *   measured in the same run on the same buffers, drop_p = 0.1, bias and gbias given.  ogbl-ppa (576 K rows, 42.5 M entries), 4 heads of
 *   d = 16: 3708 us forward and 11691 us backward against 8790 and 28539 us (0.42, 0.41); 8 heads of d = 16: 0.41 and 0.35; 4 heads of
 *   d = 64: 0.98 and 0.89.  Against hsmhb_forward_device and hsmhb_backward_device of the same object, the price of the generator: 1.07
 *   to 1.10 forward, 1.01 to 1.03 backward.  The kernels run three, three and two wavefronts per SIMD as the bias kernels do (163 / 167 /
 *   193 VGPRs), without scratch and with their LDS. */
#ifndef HISPARSE_HEADS_DROPOUT_H_
#define HISPARSE_HEADS_DROPOUT_H_

#include "hisparse_heads.h"

#ifdef __cplusplus
extern "C" {
#endif

int hsmhd_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv,
                         const float* bias_dev /* may be NULL */, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, float* y_dev,
                         uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsmhd_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias /* may be NULL */, uint32_t heads, uint32_t d, float scale, float drop_p,
                  uint64_t seed, uint64_t offset, float* y, float* lse /* may be NULL */); /* host pointers, ld = heads * d, ldl = ldb = heads, synchronous */
int hsmhd_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, const float* bias_dev /* may be NULL */, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p,
                          uint64_t seed, uint64_t offset, float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv,
                          float* gbias_dev /* may be NULL */, uint64_t ldgb);
int hsmhd_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, const float* bias /* may be NULL */, uint32_t heads,
                   uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, float* gq, float* gk, float* gv,
                   float* gbias /* may be NULL */); /* host pointers, ld = heads * d, ldl = ldb = ldgb = heads, synchronous */
int hsmhd_keep_mask(uint64_t nnz, uint32_t heads, float drop_p, uint64_t seed, uint64_t offset, uint8_t* keep /* [entry][head], 1 = kept */);

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_HEADS_DROPOUT_H_ */
