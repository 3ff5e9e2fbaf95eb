/* hisparse_gatv2.h — GATv2 ATTENTION OVER A CSR PATTERN: the score a . LeakyReLU(XD[row] + XS[col]), on the multi-head attention object
 * of hisparse_heads.h (EXTENSION; no reference counterpart).
 *
 * Six more calls on the EXISTING object hsmh_pattern.  Rows are destinations, columns are sources.  Per head h and j < d:
 *     z[e][h][j] = fl32(XD[row(e)][h d + j] + XS[col(e)][h d + j])        one fp32 add
 *     w[e][h][j] = z > 0 ? z : fl32(slope * z)                            LeakyReLU: one fp32 multiply, IEEE; z == 0 and NaN take the slope branch
 *     t[e][h]    = fl32(sum_j fl32(a[h][j] * w[e][h][j]))                 hisparse_heads.h's dot: fp32 products, added in double in any order, one rounding
 *     P[e][h]    = row softmax of t[.][h]      lse[r][h] = the row's log-sum-exp of t[.][h]
 *     Y[r][h d + j] = sum_{e in r} P[e][h] XS[col(e)][h d + j]
 *   backward, from the lse words AS GIVEN:  P = exp(t - lse[row(e)][h])
 *     GP[e][h] = sum_{j<d} fl32(gY[row(e)][h d + j] * XS[col(e)][h d + j])     D[r][h] = sum_{e in r} P GP
 *     GT[e][h] = P (GP - D[row(e)][h])
 *     dz[e][h][j] = z > 0 ? 1 : slope                              (the derivative torch's leaky_relu has, at z == 0 too)
 *     gXD[r][h d + j] = sum_{e in r}     GT a[h][j] dz[e][h][j]
 *     gXS[c][h d + j] = sum_{col(e)=c}   (P gY[row(e)][h d + j] + GT a[h][j] dz[e][h][j])
 *     ga[h][j]        = sum over ALL e   GT[e][h] w[e][h][j]
 * This is the layer of PyG's and DGL's GATv2Conv: XD = W_dst x and XS = W_src x are one dense product per side, made before the call, and
 * the score and the value read the SAME gathered row XS[col(e)].  (share_weights is XD = XS when rows are columns; it needs no call of
 * its own.)  There is no per-entry array: per entry the library gathers one row of XS, as hsgat_forward_device does, where the route
 * through hsmhb_* needs nnz x heads * d words formed outside the library and read four times.
 *     hsgat2_forward_device    Y: num_rows x ldy and lse: num_rows x ldl (may be NULL)   from   XD: num_rows x ldxd, XS: num_cols x ldxs, a
 *     hsgat2_backward_device   gXD: num_rows x ldgxd, gXS: num_cols x ldgxs, ga   from   XD, XS, a, gY and lse, in a workspace of the caller's
 *     hsgat2_work_bytes        the size of that workspace for this object, heads and d
 * Same library (libhisparse_hip.so; libhisparse_cpu.so exports the same six symbols on the host: plain loops, two passes per row, the
 * same roundings -- a second implementation, never a fallback).
 *
 * THE OBJECT is hisparse_heads.h's, whole: create, destroy, info, stream, sync and last_error are hsmh_*'s (an object from hsmhb_create
 * works as well).  The forward runs on ANY hsmh_pattern.  The backward needs HSMH_BACKWARD, for the transposed pattern and the D words
 * (HS_ERR_BAD_ARG otherwise, and the message names the flag); NO ENTRY MAP is needed and there is no new create flag.  Nothing is
 * allocated outside create, and hsmh_info is unchanged by these calls.  The forward is ONE launch and the backward THREE (row side,
 * column side, the sum of ga), one linear branch, asynchronous on the object's stream; both can be captured into a graph.  ONE BACKWARD
 * IN FLIGHT PER OBJECT, whichever of the hsmh_*, hsmh16_*, hsmhb_*, hsmhd_*, hsgat_* and hsgat2_* calls it is: the D words are shared.
 *
 * THE GRADIENT OF a is a sum over the WHOLE pattern, the one output of this family that is not owned by a row or a column.  Every output
 * word still has one writer, there are no atomics and two calls give the same words: each physical workgroup of the row side (at most
 * 8 per compute unit, 2048 on an MI355X) keeps its rows' shares of ga in double, adds its lanes in a fixed order and stores ONE vector
 * of heads * d doubles; the third launch adds the vectors in index order and rounds once.  The vectors live in a WORKSPACE THE CALLER
 * OWNS: hsgat2_work_bytes(p, heads, d, &bytes) says how large (at most 2048 * 256 * 8 bytes = 4 MiB; heads * d * 8 in
 * libhisparse_cpu.so), the _device backward takes `void* work_dev, uint64_t work_bytes`, device memory, 16-byte aligned, at least that
 * large, and its contents before and after the call mean nothing.  A workspace may serve any number of objects and calls that do not
 * run at the same time.  With nnz = 0 every word of ga is +0.0; the words are always written.
 *
 * ARGUMENTS.  slope is a float, finite and >= 0 (-0.0f counts as 0); anything else is HS_ERR_BAD_ARG.  slope = 1 makes w = z, slope = 0 a
 *   ReLU.  SHAPES ACCEPTED are hisparse_heads.h's: d in {4, 8, ..., 256}, heads <= max_heads and heads * d <= 256.  FOR ANY OTHER d:
 *   pad every head of XD, XS, a and gY with zero columns up to the next accepted d.  This is exact: a pad word has z = w = +0, adds
 *   a * w = +0 to the score and +0 to GP, and the pad columns of Y, gXD, gXS and ga come out +0.
 * LAYOUT.  XD, XS, gY, Y, gXD and gXS follow hisparse_heads.h: fp32 [index][head][feature], 16-byte aligned, ld a multiple of 4 and at
 *   least heads * d; pad words are not read into any result and are not written.  a and ga are fp32 [head][feature], heads * d
 *   CONTIGUOUS words, 16-byte aligned, with no ld.  lse is fp32 [row][head] as in hisparse_gat.h: 4-byte aligned, ldl >= heads, words
 *   h >= heads of a row neither read nor written, reach ((num_rows - 1) * ldl + heads) * 4 bytes.  An output may share no byte with an
 *   input, with another output or with the workspace, and the workspace none with an input; ranges that touch are fine.  Every breach
 *   -- a null, misaligned or too small workspace among them -- is HS_ERR_BAD_ARG, hsmh_last_error(p) says why, and the object stays
 *   usable.
 * hsgat2_forward / hsgat2_backward: the host-pointer forms, ld = heads * d, ldl = heads, no alignment rule; they copy in, run, copy out
 *   and are synchronous, and allocate their transients, the workspace among them, themselves.
 *
 * ARITHMETIC: z and w are exactly the two fp32 operations above: there is no freedom of order, so they carry NO error term.  Every
 *   product a * w and gY * XS is one fp32 multiply (the library is built with -ffp-contract=off).  The score is a d-term dot of exactly
 *   known fp32 words, added in double and rounded once: its error term is hisparse_attention.h's eta at scale = 1 with the operands a
 *   and w.  Everything else is in double with the library's exp and log.  The row side forms, per word j, A_j = sum P GP dz_j and
 *   B_j = sum P dz_j and gXD_j = a_j (A_j - D B_j), as the row side of hisparse_gat.h forms gel = A - D B; beside them
 *   A'_j = sum P GP w_j and B'_j = sum P w_j, and A'_j - D B'_j is the row's share of ga_j.  The column side keeps sum P gY_j and
 *   sum GT dz_j apart and adds a_j times the second to the first.  One rounding to fp32 per output word.
 *   BOUNDS: those of hisparse_attention.h and hisparse_attention_backward.h with scale = 1, the operands a and w in the place of Q and K
 *   and the feature word that multiplies GS_e replaced by a_j dz_ej (gXD, gXS) or w_ej (ga).  With u = 2^-24, n_r the entries of the row,
 *   m_c those of the column, S_e the exact sum of the products fl32(a_j w_ej) and A_e the sum of their magnitudes:
 *     delta_e = u|S_e| + d 2^-52 A_e + 2^-149      eta_e = (1 + u) delta_e + u|S_e| + 2^-149      eta_r = max_{e in r} eta_e
 *     |y - Y|     <= u|Y| + expm1(eta_r)/(1 - expm1(eta_r)) sum P|XS - Y| + (n_r + 16) 2^-52 sum P|XS| + 2^-149
 *     |lse - LSE| <= u|LSE| + eta_r + (n_r + 16) 2^-52 (1 + |LSE|) + 2^-149
 *     rho_e  = expm1(eta_e + 32 * 2^-52)            gam_e = u|GP_e| + d 2^-52 A'_e + 2^-149  (A'_e = sum_j |gY XS|)
 *     epsD_r = sum_r P(rho_e|GP| + (1+rho_e) gam) + (n_r+16) 2^-52 sum_r P|GP|
 *     eps_e  = rho_e P|GP - D| + (1+rho_e) P (gam_e + epsD_r)                  mag_e = P(|GP| + |D|)
 *     |gxd - GXD| <= u|GXD| + sum_{e in r} eps_e |a_j| dz_ej + (n_r + 16) 2^-52 sum_{e in r} mag_e |a_j| dz_ej + 2^-149
 *     |gxs - GXS| <= u|GXS| + sum_{col=c} (rho_e P|gY_j| + eps_e |a_j| dz_ej) + (m_c + 16) 2^-52 sum_{col=c} (P|gY_j| + mag_e |a_j| dz_ej) + 2^-149
 *     |ga - GA|   <= u|GA| + sum_{ALL e} eps_e |w_ej| + sum_r (n_r + 16) 2^-52 sum_{e in r} mag_e |w_ej|
 *                    + ((R + 16) + (G + 16)) 2^-52 sum_{ALL e} mag_e |w_ej| + 2^-149
 *   ga's first three terms are a row's share held to gel's bound of hisparse_gat.h and summed over the rows.  The shares are then
 *   added in double in an order of which the bound only uses that it is fixed: the R rows with entries inside the workgroups (adding a
 *   lane that holds +0.0 is exact), and the G workgroup vectors in the third launch (G <= 2048; G = 1 in libhisparse_cpu.so), each
 *   at most that many additions deep.  No tolerance is introduced.
 *
 * SPECIAL ROWS AND VALUES, per head; HEADS DO NOT LEAK: a word of XD, XS, a, gY or lse of head h reaches head h's words only.
 *   A row without entries reads +0.0 in Y and gXD and -inf in lse; a column without entries +0.0 in gXS; both whatever a holds.  A NaN
 *   or +inf t makes the row's head NaN in Y and lse: a NaN word of XD[r] or of a[h] does (slope * NaN and a * NaN are NaN), and so does
 *   a NaN word of XS[c] in every row that holds c, whose Y it reaches as a value as well.  t = -inf weighs exactly 0 (a word of -inf
 *   in XS[c] under a positive a_j and slope > 0 scores -inf, but as a VALUE 0 * -inf is NaN by IEEE: mask through the pattern, not
 *   through XS).  In the backward a lse word that is not finite gives NaN in that head's words of gXD[r], and of gXS[c] for every
 *   column c the row touches, and in ALL d words of ga[h]: ga is a sum over every row.  A NaN in a[h] makes every t of head h NaN:
 *   head h's words of gXD, gXS and ga are NaN and nothing else is.  No other word is touched.
 *
 * HOW THE WORK IS SCHEDULED: four kernels (gatv2_attention.hip) on the unchanged schedule of hisparse_wide.h at the width heads * d:
 *   groups of lanes over 16-byte chunks, teams by length class, rows and columns above 512 entries on a workgroup of their own and
 *   started first, a row or column of any length on ONE workgroup, groups merged by shuffles and the four wavefronts through LDS.
 *   Forward: a lane owns one chunk, keeps a's chunk for the whole kernel and XD[r]'s for the row, and per trip of four entries issues
 *   the four gathers of XS before the first use; it forms z and w of its chunk itself and the d / 4 lanes of a head add the partial
 *   dots a . w by the shuffle tree of the dot-product kernels; per lane the online softmax of hisparse_heads.h.  Row side: the same
 *   single gather, two dots per entry (a . w and gY . XS), seventeen sums per lane (D and four each of A, B, A', B'), and four more
 *   that persist over the rows a workgroup walks: the chunk a lane owns does not depend on the row.  Column side, over the transposed
 *   pattern: XS[c]'s and a's chunks in registers, per entry the gathers of gY[r]'s and XD[r]'s chunks and of lse and D of (r, h),
 *   eight sums per lane.  The fourth kernel is one workgroup that adds the vectors.
 *
 * COST (MI355X; tools/gatv2_times.py, profiles/gatv2_times.txt; DESIGN.md section 6e has the table and the method): the call against
 *   what a caller had before it, charged in full -- the torch expression that forms t per entry from gathered rows,
 *   hsmhb_forward_device / hsmhb_backward_device of the SAME object with Q and K zeroed, the per-entry product that turns gbias into
 *   the gradients of the gathered rows with its two reductions, and the reduction for ga -- in one run on the same buffers, slope 0.2,
 *   medians of three.  ogbl-ppa (576 K rows, 42.5 M entries), forward / backward in us, v2 against baseline:
 *       4 x 16:   2787.5 /  45928.6 (0.061)     9708.8 /  54082.0 (0.180)        8 x 8:    2993.5 /  46407.6 (0.065)     9456.7 /  56261.1 (0.168)
 *       8 x 16:   4982.8 /  77573.9 (0.064)    18799.7 / 106274.0 (0.177)        4 x 64:  10816.8 / 141468.8 (0.076)    39134.2 / 212384.0 (0.184)
 *   transformer-50 (8.5 M entries): 0.053, 0.058, 0.062, 0.071 forward and 0.094, 0.086, 0.113, 0.134 backward.  No shape is slower than
 *   the baseline, nearly all of which is the per-entry array.  The forward costs what hsgat_forward_device costs, the backward 1.6 times
 *   hsgat_backward_device.  The two paths differ by at most 3.2e-06 of the largest magnitude (fp32 sums there, double here).  There is no
 *   pass/fail ratio.  The kernels take 160 (forward), 231 (row side), 204 (column side) and 28 (sum of ga) VGPRs: three, two, two
 *   wavefronts per SIMD; no scratch; 11, 34 and 16 KiB of LDS. */
#ifndef HISPARSE_GATV2_H_
#define HISPARSE_GATV2_H_

#include "hisparse_heads.h"

#ifdef __cplusplus
extern "C" {
#endif

int hsgat2_forward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev /* heads * d words */, uint32_t heads, uint32_t d,
                          float slope, float* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsgat2_forward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, uint32_t heads, uint32_t d, float slope, float* y,
                   float* lse /* may be NULL */); /* host pointers, ld = heads * d, ldl = heads, synchronous */
int hsgat2_work_bytes(const hsmh_pattern* p, uint32_t heads, uint32_t d, uint64_t* bytes); /* HS_ERR_BAD_ARG for a shape the calls refuse */
int hsgat2_backward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev, const float* gy_dev, uint64_t ldgy,
                           const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gxd_dev, uint64_t ldgxd, float* gxs_dev, uint64_t ldgxs,
                           float* ga_dev /* heads * d words */, void* work_dev, uint64_t work_bytes);
int hsgat2_backward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, const float* gy, const float* lse, uint32_t heads, uint32_t d, float slope, float* gxd,
                    float* gxs, float* ga); /* host pointers, ld = heads * d, ldl = heads, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_GATV2_H_ */
