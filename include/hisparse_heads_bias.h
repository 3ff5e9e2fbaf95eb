/* hisparse_heads_bias.h — A PER-ENTRY, PER-HEAD ADDITIVE BIAS for the multi-head attention object of hisparse_heads.h (EXTENSION; no
 * reference counterpart).
 *
 * Five more calls on the EXISTING object hsmh_pattern.  The formulas are those of hisparse_heads.h with ONE change, the score before
 * the softmax:
 *     t[e][h] = scale * s[e][h] + bias[e][h]
 * which is what edge encodings, relative-position and distance biases, soft masks and hard masks (a bias of -inf) need.  The backward
 * adds one output, the gradient of the bias,
 *     gB[e][h] = P[e][h] * (GP[e][h] - D[row(e)][h])
 * which carries no factor scale and is defined for scale = 0 too.  The bias is the one per-entry array that belongs to the caller; the
 * library still builds none of its own: forward is ONE launch, backward is TWO, neither allocates or synchronises.
 *     hsmhb_forward_device    Y and lse as hsmh_forward_device   from   Q, K, V and bias: nnz x ldb
 *     hsmhb_backward_device   gQ, gK, gV as hsmh_backward_device and gbias: nnz x ldgb (may be NULL)   from   Q, K, V, gY, lse and bias
 * Same library (libhisparse_hip.so; libhisparse_cpu.so exports the same five symbols on the host: plain loops, the same two roundings
 * of t -- a second implementation, never a fallback).
 *
 * hsmhb_create is hsmh_create: the same arguments, checks, error codes and messages, and the object it returns works with every hsmh_*
 *   and hsmh16_* call, with their results unchanged.  With HSMH_BACKWARD it also keeps THE ENTRY MAP, the CSR index of every entry of the
 *   transposed pattern, which the column side of the backward needs to find an entry's bias words and to store its gbias words:
 *       device_bytes += 4 max(nnz, 1)
 *   on top of hsmh_create's formula; hsmh_info reports exactly that.  Every allocation still happens at create.
 *   hsmhb_forward and hsmhb_forward_device need no map and accept ANY hsmh_pattern, one from plain hsmh_create included.
 *   hsmhb_backward and hsmhb_backward_device on an object without the map (from hsmh_create, or from hsmhb_create without
 *   HSMH_BACKWARD) are HS_ERR_BAD_ARG and the message names hsmhb_create.
 *
 * LAYOUT.  bias and gbias are fp32 [entry][head]: the word of (entry e, head h) sits at e * ld + h, with e THE INDEX IN THE CALLER'S CSR
 *   ORDER (the order of `indices` given to create; a pair held twice is two entries, two bias words and two gbias words per head).
 *   ldb >= heads and ldgb >= heads, 4-byte alignment, as for lse.  Words h >= heads of an entry are never read (bias) or written (gbias).
 *   bias reaches ((nnz - 1) * ldb + heads) * 4 bytes and gbias ((nnz - 1) * ldgb + heads) * 4; with nnz = 0 neither pointer is
 *   dereferenced.  bias is REQUIRED (a caller without one has hsmh_forward_device); gbias MAY BE NULL, for a bias that is a constant such
 *   as a mask.  bias is an input and gbias an output under the overlap rule of hisparse_heads.h: gbias may share no byte with Q, K, V, gY,
 *   lse, bias, gQ, gK or gV, and Y, lse (forward), gQ, gK and gV none with bias.  Everything else -- the feature operands, lse, the
 *   shapes accepted (d in {4, ..., 256}, heads * d <= 256, fp32), scale finite, the stream rules, ONE BACKWARD IN FLIGHT PER OBJECT
 *   (whichever of the hsmh_*, hsmh16_* and hsmhb_* calls it is) -- is hisparse_heads.h's.  Every breach is HS_ERR_BAD_ARG,
 *   hsmh_last_error(p) says why, and the object stays usable.
 * hsmhb_forward / hsmhb_backward: the host-pointer forms, ld = heads * d for the features and ld = heads for lse, bias and gbias.
 *
 * ARITHMETIC: t = fl32(fl32(scale * fl32(s)) + bias): s rounded once to fp32 as in hisparse_heads.h, ONE fp32 multiply, then ONE fp32
 *   add, no contraction into a fused multiply-add.  Everything after t is as documented there.  gB is formed in double and rounded once.
 *   Against the bounds of hisparse_heads.h the per-entry score error eta_e becomes (1 + u) eta_e + u |t_e| (u = 2^-24, the rounding of
 *   the one extra add) and everything downstream of eta_e is unchanged; gB is held to the bound of GS with the factor |scale| left out,
 *   plus its own rounding.
 *   CONSEQUENCE: with every bias word +0.0 the three feature outputs and lse are BIT FOR BIT those of hsmh_forward_device and
 *   hsmh_backward_device on the same object (x + 0 = x; the schedule and the order of every sum are the same).
 *
 * SPECIAL ROWS AND VALUES: the tables of hisparse_heads.h, applied to t.  A bias of -inf under a finite row maximum weighs exactly 0:
 *   the entry adds nothing to Y, gQ, gK or gV and its gB word is zero, so a masked pattern computes what the pattern without the masked
 *   entries computes.  A row whose entries are all -inf in one head is that table's "only -inf" row in that head: Y NaN, lse -inf.  A
 *   NaN or +inf bias word behaves as a NaN or +inf score.  HEADS DO NOT LEAK: a bias word of head h reaches head h's d words only.
 *   Every output word, gbias included, has exactly one writer and there are no atomics: two calls with the same inputs give the same
 *   words.
 *
 * HOW THE WORK IS SCHEDULED: the three kernels of hisparse_heads.h restated (heads_bias_attention.hip) on the unchanged schedule of
 *   hisparse_wide.h.  Forward and row side: the lanes of a head stream their entry's bias word (one address per head, a non-temporal
 *   load issued with the column index).  Column side: per transposed entry the map word is streamed beside the row index, the bias word
 *   is gathered through it, and one lane of each head of the group that owns the entry stores the gB word, one piece of 4 * heads bytes
 *   per entry.  gB comes from the column side because D of a row is complete only after the row's last entry.  Where a head has at least
 *   four lanes (d >= 16) lane i of each four loads the bias word (and the map word) of the trip's entry i alone and forms that entry's
 *   score alone, as the weights of a trip are dealt in hisparse_heads.h: one load per lane and trip instead of four.
 *
 * COST (MI355X; tools/heads_bias_times.py, profiles/heads_bias_times.txt; DESIGN.md section 6b has the table and the bar): the call against
 *   what a caller with a bias had to do before it -- per head the chain of hsw_sddmm_device, an element-wise add, hsr_softmax_device and
 *   hsw_spmm_device forward and the seven-call chain backward, with one more element-wise operation for the bias's gradient -- measured
 *   in the same run on the same buffers.  ogbl-ppa (576 K rows, 42.5 M entries), 4 heads of d = 16: 3447 us forward and 11673 us backward
 *   (gbias given) against 8510 and 27909 us (0.41, 0.42); 8 heads of d = 16: 0.39 and 0.36; 4 heads of d = 64: 0.97 and 0.90.  Against
 *   hsmh_forward_device and hsmh_backward_device of the same object, without a bias: 0.98 to 1.01 forward, 1.27 to 1.47 backward (the
 *   column side gathers the bias and scatters gbias in pieces of 4 * heads bytes).  The kernels run three, three and two wavefronts per
 *   SIMD as the plain ones (158 / 159 / 187 VGPRs).  The object holds 556 MB on ogbl-ppa with max_heads = 8, 170 MB of it the map. */
#ifndef HISPARSE_HEADS_BIAS_H_
#define HISPARSE_HEADS_BIAS_H_

#include "hisparse_heads.h"

#ifdef __cplusplus
extern "C" {
#endif

int hsmhb_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads,
                 uint32_t flags); /* hsmh_create, and with HSMH_BACKWARD the entry map as well */
int hsmhb_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* bias_dev, uint64_t ldb,
                         uint32_t heads, uint32_t d, float scale, float* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsmhb_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias, uint32_t heads, uint32_t d, float scale, float* y,
                  float* lse /* may be NULL */); /* host pointers, ld = heads * d, ldl = ldb = heads, synchronous */
int hsmhb_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float* gq_dev, uint64_t ldgq,
                          float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv, float* gbias_dev /* may be NULL */, uint64_t ldgb);
int hsmhb_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale,
                   float* gq, float* gk, float* gv, float* gbias /* may be NULL */); /* host pointers, ld = heads * d, ldl = ldb = ldgb = heads, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_HEADS_BIAS_H_ */
