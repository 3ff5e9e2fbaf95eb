/* hisparse_gat.h — GRAPH ATTENTION (GAT) OVER A CSR PATTERN: additive scores from one word per node and head, on the multi-head
 * attention object of hisparse_heads.h (EXTENSION; no reference counterpart).
 *
 * Four more calls on the EXISTING object hsmh_pattern.  Rows are destinations, columns are sources.  Per head h:
 *     x[e][h]  = fl32(el[row(e)][h] + er[col(e)][h])              one fp32 add
 *     t[e][h]  = x > 0 ? x : fl32(slope * x)                      LeakyReLU: one fp32 multiply, IEEE; x == 0 takes the slope branch
 *     P[e][h]  = row softmax of t[.][h]      lse[r][h] = the row's log-sum-exp of t[.][h]
 *     Y[r][h d + j] = sum_{e in r} P[e][h] V[col(e)][h d + j]
 *   backward, from the lse words AS GIVEN:  P = exp(t - lse[row(e)][h])
 *     GP[e][h] = sum_{j<d} gY[row(e)][h d + j] * V[col(e)][h d + j]     D[r][h] = sum_{e in r} P GP
 *     dx[e][h] = x > 0 ? 1 : slope                                 (the derivative torch's leaky_relu has, at x == 0 too)
 *     GX[e][h] = P (GP - D[row(e)][h]) dx
 *     gel[r][h] = sum_{e in r} GX      ger[c][h] = sum_{col(e)=c} GX      gV[c][h d + j] = sum_{col(e)=c} P gY[row(e)][h d + j]
 * el and er are ONE WORD PER NODE AND HEAD.  A model forms them before the call, el[i][h] = a_l[h] . Wh[i][h] and er[j][h] = a_r[h] . Wh[j][h]
 * (one small dense product per side), and V = Wh.  There is no Q, no K, no scale and no per-entry array: per entry the library gathers one
 * row of V and `heads` words of er.
 *     hsgat_forward_device    Y: num_rows x ldy and lse: num_rows x ldl (may be NULL)   from   el: num_rows x ldel, er: num_cols x lder, V
 *     hsgat_backward_device   gel: num_rows x ldgel, ger: num_cols x ldger, gV: num_cols x ldgv   from   el, er, V, gY and lse
 * Same library (libhisparse_hip.so; libhisparse_cpu.so exports the same four symbols on the host: plain loops, two passes per row, the
 * same roundings -- a second implementation, never a fallback).
 *
 * THE OBJECT is hisparse_heads.h's, whole: create, destroy, info, stream, sync and last_error are hsmh_*'s (an object from hsmhb_create
 * works as well).  The forward runs on ANY hsmh_pattern.  The backward needs HSMH_BACKWARD, for the transposed pattern and the D words
 * (HS_ERR_BAD_ARG otherwise, and the message names the flag); NO ENTRY MAP is needed.  Nothing is allocated outside create, and hsmh_info
 * is unchanged by these calls.  The forward is ONE launch and the backward TWO, asynchronous on the object's stream; both can be captured
 * into a graph.  ONE BACKWARD IN FLIGHT PER OBJECT, whichever of the hsmh_*, hsmh16_*, hsmhb_*, hsmhd_* and hsgat_* calls it is: the D
 * words are shared.
 *
 * ARGUMENTS.  slope is a float, finite and >= 0 (-0.0f counts as 0); anything else is HS_ERR_BAD_ARG.  slope = 1 makes t = x, slope = 0 a
 *   ReLU.  SHAPES ACCEPTED are hisparse_heads.h's: d in {4, 8, ..., 256}, heads <= max_heads and heads * d <= 256 (the backward's dot of
 *   gY and V over a head's lanes uses the same shuffle tree).  FOR ANY OTHER d: the scores do not read V, so pad every head of V and gY
 *   with zero columns up to the next accepted d.  This is exact, and the pad columns of Y and gV come out +0.
 * LAYOUT.  V, gY, Y and gV follow hisparse_heads.h: fp32 [index][head][feature], 16-byte aligned, ld a multiple of 4 and at least
 *   heads * d; pad words are not read into any result and are not written.  el, gel and lse are fp32 [row][head], er and ger fp32
 *   [column][head]: 4-byte aligned, ld >= heads, words h >= heads of a row are neither read into a result nor written, and the reach of
 *   each of the five is ((n - 1) * ld + heads) * 4 bytes.  An output may share no byte with an input or with another output; ranges that
 *   touch are fine.  Every breach is HS_ERR_BAD_ARG, hsmh_last_error(p) says why, and the object stays usable.
 * hsgat_forward / hsgat_backward: the host-pointer forms, ld = heads * d for the features and ld = heads for the five head arrays, no
 *   alignment rule; they copy in, run, copy out and are synchronous.
 *
 * ARITHMETIC: x and t are exactly the two fp32 operations above: there is no freedom of order, so a score carries NO error term.  Every
 *   product gY * V is one fp32 multiply (the library is built with -ffp-contract=off).  Everything else is in double with the library's
 *   exp and log.  The row side forms gel = A - D B with A = sum P GP dx and B = sum P dx, as the row side of hisparse_attention_backward.h
 *   does.  One rounding to fp32 per output word.  Every output word has one writer, there are no atomics: two calls give the same words.
 *   BOUNDS: those of hisparse_attention.h and hisparse_attention_backward.h with scale = 1, eta_e = 0 and the feature word that multiplies
 *   GS_e replaced by dx_e.  With u = 2^-24, rho = expm1(32 * 2^-52), n_r the entries of the row and m_c those of the column:
 *     |y - Y|     <= u|Y| + rho/(1-rho) sum P|V - Y| + (n_r + 16) 2^-52 sum P|V| + 2^-149
 *     |lse - LSE| <= u|LSE| + (n_r + 16) 2^-52 (1 + |LSE|) + 2^-149
 *     gam_e  = u|GP_e| + d 2^-52 A'_e + 2^-149  (A'_e = sum_j |gY V|)     epsD_r = sum_r P(rho|GP| + (1+rho) gam) + (n_r+16) 2^-52 sum_r P|GP|
 *     eps_e  = rho P|GP - D| + (1+rho) P (gam_e + epsD_r)                  mag_e = P(|GP| + |D|)
 *     |gel - GEL| <= u|GEL| + sum_{e in r} eps_e dx_e + (n_r + 16) 2^-52 sum_{e in r} mag_e dx_e + 2^-149
 *     |ger - GER| <= the same over the column's entries with m_c
 *     |gv - GV|   <= u|GV| + sum_{col=c} rho P|gY| + (m_c + 16) 2^-52 sum_{col=c} P|gY| + 2^-149
 *
 * SPECIAL ROWS AND VALUES, per head; HEADS DO NOT LEAK: a word of el, er or lse of head h reaches head h's words only.
 *   A row without entries reads +0.0 in Y and gel and -inf in lse; a column without entries +0.0 in ger and gV.  A NaN or +inf x makes
 *   the row's head NaN in Y and lse.  x = -inf with slope > 0 weighs exactly 0: an er word of -inf is how a caller masks a source for a
 *   head (and an el word of -inf a whole destination: Y NaN, lse -inf).  WITH slope = 0, 0 * -inf IS NaN BY IEEE AND THE ROW'S HEAD IS BAD:
 *   mask with a slope above 0.  In the backward a lse word that is not finite gives NaN in that head's gel[r], and in that head's ger[c]
 *   and d words of gV[c] for every column c the row touches.  No other word is touched.
 *
 * HOW THE WORK IS SCHEDULED: three kernels (gat_attention.hip) on the unchanged schedule of hisparse_wide.h at the width heads * d:
 *   groups of lanes over 16-byte chunks, teams by length class, rows and columns above 512 entries on a workgroup of their own and
 *   started first, a row or column of any length on ONE workgroup, groups merged by shuffles and the four wavefronts through LDS.
 *   Forward: a lane owns one chunk, reads its head's el word once and per trip of four entries issues the four gathers of V and the four
 *   one-word loads of er before the first use; the lanes of a head load the same word, so each forms x and t itself and the forward has
 *   no dot and no shuffle inside a head; per lane the online softmax of hisparse_heads.h (m, l and four sums).  Row side: gY's chunk and
 *   the el and lse words in registers, the d / 4 lanes of a head add the partial dots by shuffles, three sums per lane (D, A, B).  Column
 *   side, over the transposed pattern: V's chunk and the er word in registers, per entry the gathers of gY[r]'s chunk and of el, lse
 *   and D of (r, h), five sums per lane.
 *
 * COST (MI355X; tools/gat_times.py, profiles/gat_times.txt; DESIGN.md section 6d has the table): the call against what a caller had before
 *   it -- hsmhb_forward_device / hsmhb_backward_device of the SAME object with Q and K zeroed and a precomputed LeakyReLU(el + er) bias
 *   (making it is not charged), plus, in the backward, the two reductions of gbias into g_el (torch.segment_reduce by row) and g_er
 *   (Tensor.index_add_ by column; no hsr_* or hsw_* call fits a per-entry operand of `heads` words) -- in one run on the same buffers,
 *   slope 0.2, medians of three.  ogbl-ppa (576 K rows, 42.5 M entries), forward / backward in us, gat against baseline:
 *       4 x 16:   2888.6 /  3408.0 (0.85)     6106.2 / 14385.2 (0.42)        8 x 8:    2900.8 /  3447.9 (0.84)     6155.6 / 16236.0 (0.38)
 *       8 x 16:   5147.1 /  6687.9 (0.77)    10809.6 / 24315.0 (0.44)        4 x 64:  10138.1 / 13732.7 (0.74)    23110.5 / 44551.4 (0.52)
 *   transformer-50 (8.5 M entries): 0.98, 0.90, 0.90, 0.75 forward and 0.14, 0.09, 0.17, 0.29 backward, where the column reduction's
 *   atomics weigh most.  No shape is slower than the baseline.  Y and gV are the baseline's words bit for bit (a zero dot adds +0.0), gel
 *   and ger differ from its reduced gbias by at most 9.4e-06 of the largest magnitude (fp32 sums there, double here).  There is no
 *   pass/fail ratio.  The kernels take 130 (forward), 122 (row side) and 152 (column side) VGPRs: three, four and three wavefronts per
 *   SIMD, where the fp32 kernels of hisparse_heads.h run three, three and two; no scratch; 11, 6 and 10 KiB of LDS. */
#ifndef HISPARSE_GAT_H_
#define HISPARSE_GAT_H_

#include "hisparse_heads.h"

#ifdef __cplusplus
extern "C" {
#endif

int hsgat_forward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                         float slope, float* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsgat_forward(hsmh_pattern* p, const float* el, const float* er, const float* v, uint32_t heads, uint32_t d, float slope, float* y,
                  float* lse /* may be NULL */); /* host pointers, ld = heads * d, ld = heads for el, er and lse, synchronous */
int hsgat_backward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gel_dev, uint64_t ldgel, float* ger_dev, uint64_t ldger, float* gv_dev,
                          uint64_t ldgv);
int hsgat_backward(hsmh_pattern* p, const float* el, const float* er, const float* v, const float* gy, const float* lse, uint32_t heads, uint32_t d, float slope, float* gel,
                   float* ger, float* gv); /* host pointers, ld = heads * d, ld = heads for el, er, lse, gel and ger, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_GAT_H_ */
