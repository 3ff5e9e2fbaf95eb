/* hisparse_attention_backward.h — the BACKWARD of the attention step over a matrix's CSR pattern in ONE call: from (Q, K, V, gY, lse) to
 * (gQ, gK, gV), with ROW-MAJOR dense operands and no per-entry array (EXTENSION; no reference counterpart).
 *
 * hisparse_attention.h does the forward step in one launch and writes lse, one word per row.  Without this object the backward step
 * recomputes S and P with hsw_sddmm_device + hsr_softmax_device and runs the five calls of hisparse_wide.h's chain: seven launches and
 * three to four arrays of nnz words.  This object holds the pattern and its transpose and does
 *     hsab_backward_device   gQ: num_rows x ldgq, gK: num_cols x ldgk, gV: num_cols x ldgv   from   Q, gY: num_rows rows, K, V: num_cols
 *                                                                                                  rows, lse: num_rows words
 * in TWO kernels on one stream.  With row(e), col(e) and the order of the entries as in hisparse_wide.h the call computes a function of
 * its inputs alone:
 *     S_e  = sum_{j < d} Q[row(e)][j] * K[col(e)][j]       T_e = scale * S_e       P_e = exp(T_e - lse[row(e)])
 *     GP_e = sum_{j < d} gY[row(e)][j] * V[col(e)][j]      D_r = sum_{e in r} P_e * GP_e
 *     GS_e = scale * P_e * (GP_e - D_r)
 *     gQ[r][j] = sum_{e in r} GS_e * K[col(e)][j]
 *     gK[c][j] = sum_{col(e) = c} GS_e * Q[row(e)][j]
 *     gV[c][j] = sum_{col(e) = c} P_e * gY[row(e)][j]
 * D comes from P . GP inside the call: Y is not an input.  With lse as hsat_forward_device wrote it for the same Q, K and scale, P is the
 * forward's row softmax and the three results are the gradients of sum_{r, j} gY[r][j] * Y[r][j].
 *
 * ALL FEATURES ARE fp32, 1 <= d <= 256, and there is no impl argument, as in hisparse_wide.h.  Same library (libhisparse_hip.so;
 * libhisparse_cpu.so exports the same eight symbols on the host: plain loops on the calling thread, two passes per row, "device"
 * pointers are host pointers, hsab_set_stream accepts and ignores and hsab_sync is a no-op -- a second implementation, never a fallback:
 * without a usable gfx950 device this library's hsab_create fails with HS_ERR_NO_DEVICE / HS_ERR_HIP as hs_create does).  Error codes
 * are those of hisparse_hip.h.
 *
 * hsab_create: indptr[num_rows + 1] and indices[nnz] are HOST arrays and the validation is hsat_create's: an indptr that decreases or
 *   does not start at 0, or a column index >= num_cols, is HS_ERR_BAD_MATRIX; num_rows == 0, num_cols == 0 or a null pointer (indices
 *   may be NULL when nnz = 0) is HS_ERR_BAD_ARG; *out is then NULL and hsab_last_error(NULL) says why.  A pair held twice is two
 *   entries, the columns of a row may come in any order, nnz = 0 is a valid object.  EVERY allocation happens here: the object keeps on
 *   the device indptr, indices and the list of the rows sorted into the length classes of hisparse_wide.h; the transposed pattern, built
 *   on the host by hisparse_wide.h's stable counting sort -- column pointers and the row of every entry in column order, WITHOUT the
 *   CSR-index map (there is no per-entry array to index) -- with the list of the columns sorted into the same classes; and one double
 *   per row, the row's D, which the first kernel writes and the second reads:
 *       device_bytes = 4 (num_rows + 1) + 4 max(nnz, 1) + 4 num_rows + 4 (num_cols + 1) + 4 max(nnz, 1) + 4 num_cols + 8 num_rows
 *   which hsab_info reports beside nnz (either pointer may be NULL).  hsab_backward_device allocates nothing, synchronises nothing and is
 *   exactly TWO kernel launches on the object's stream; it can be captured into a graph (one linear branch).
 *   ONE BACKWARD CALL MAY BE IN FLIGHT PER OBJECT, because of the D words: calls on one object must be ordered by their stream (the same
 *   stream, or an event between two streams).  Two heads, or two layers over the same pattern, that are to overlap need two objects.
 *
 * LAYOUT of hsab_backward_device: hisparse_attention.h's.  Row i of a dense operand starts at word i * ld.  The seven feature pointers
 *   are 16-byte aligned, every ld is a multiple of 4 and at least d.  Words d ... ld - 1 of an input row may be loaded but reach no
 *   result: a NaN there changes nothing.  Words d ... ld - 1 of an output row are not written.  lse_dev is a 4-byte aligned array of
 *   num_rows words and is REQUIRED.  An operand of n rows reaches from its pointer to the end of the 16-byte chunk that holds word d - 1
 *   of row n - 1 (that much must be the caller's memory); the three outputs may not share a byte with an input (lse among them) or with
 *   each other.  scale must be finite.  Every breach is HS_ERR_BAD_ARG, hsab_last_error(p) says why, and the object stays usable.  d
 *   and scale may change from call to call.
 * HEADS.  H heads stored [index][head][feature] are H calls with ld = H * d and the seven feature pointers offset by h * d words (lse: one
 *   array of num_rows words per head), one after the other on the object's stream.  d must then be a multiple of 4, so that the offset
 *   pointers keep the 16-byte alignment; the words of the other heads lie in the pad of each row: those of the inputs reach no result
 *   and those of the outputs are not written.
 * hsab_backward: the host-pointer form, ld = d exactly for all seven feature arrays, no alignment rule beyond a float's, lse required;
 *   it copies in, runs, copies out; synchronous; its transient device buffers are the only allocations outside hsab_create.
 *
 * SPECIAL VALUES.
 *     a row without entries              d words of +0.0f in gQ[r]
 *     a column without entries           d words of +0.0f in gK[c] and in gV[c]
 *     lse[r] not finite (a dead or bad   NaN in all d words of gQ[r], and in all d words of gK[c] and gV[c] of every column c that holds
 *     row of the forward), n_r > 0       one of the row's entries; no other word is touched
 *   A -inf score under a finite lse has P exactly 0.  A zero weight times a non-finite word follows IEEE, as in hsw_spmm_device.  A NaN
 *   or +inf score under a finite lse cannot come from hsat_forward; the words it reaches (its row of gQ, the columns of the row's
 *   entries) are unspecified, and no other word is.  Every output word has exactly one writer and there are no atomics: two calls with
 *   the same inputs give the same words.
 *
 * HOW THE WORK IS SCHEDULED: both kernels exactly as in hisparse_wide.h (groups of lanes that cover a feature row in 16-byte chunks,
 *   teams of groups by the length class, more than 512 entries on a workgroup of their own and started first; A ROW, AND A COLUMN, OF ANY
 *   LENGTH RUNS ON ONE WORKGROUP).  Row side: the row's chunks of Q and gY stay in registers; per trip a group takes four entries and
 *   issues their four gathers of K and four of V before the first use, adds both dots over its lanes by shuffles and forms p.  The row
 *   is ONE pass with nine double sums per lane, a_j += p gp K_j, b_j += p K_j, D += p gp, then gQ_j = scale (a_j - D b_j): lse is known,
 *   so there is no running maximum and no rescale.  It stores gQ and the row's D.  Column side, over the transposed pattern: the
 *   column's chunks of K and V stay in registers; per entry it gathers Q[r] and gY[r] in 16-byte loads, reads lse[r] and D[r], forms the
 *   two dots, p and gs, and adds gK_j += gs Q_j, gV_j += p gY_j.  Groups merge by lane shuffles, the four wavefronts of a long row or
 *   column through LDS.  No matrix engine.
 *
 * STREAM ORDER: hisparse_wide.h's.  hsab_set_stream(NULL) restores the object's own stream; hsab_sync waits for the current one; a
 *   caller-owned stream must be synchronised by its owner before hsab_destroy.  A training step on one stream is three launches:
 *   hsat_forward_device, then (after the caller's own work on Y) hsab_backward_device.
 *
 * COST (MI355X; tools/attention_backward_times.py, profiles/attention_backward_times.txt; DESIGN.md section 6b has the table and the
 *   bar).  ogbl-ppa (576 K rows, 42.5 M entries), d = 16 and 64: 4078 and 8641 us against 6165 and 11292 us for the chain's seven calls
 *   in the same run (0.66, 0.77); transformer-50 (every row and column a long one): 364 and 1329 us against 616 and 1751.  The call
 *   costs what its four gathers cost; the object holds 354 MB on ogbl-ppa against four arrays of 170 MB plus hsw's 519 MB for the chain.
 *   hsab_create takes 485 ms there (the host's counting sort of the transposed pattern, as hsw_create with HSW_TRANSPOSED).
 *
 * ARITHMETIC.
 *   Every product Q[r][j] * K[c][j] and gY[r][j] * V[c][j] is ONE fp32 multiply (no FMA contraction: -ffp-contract=off); the d products
 *   of an entry are added in double, in any order.  s[e] is rounded once to fp32 and t[e] = scale * s[e] is one fp32 multiply, exactly
 *   as hsat_forward_device forms them; gp[e] may be rounded once to fp32 or kept double.  From there on everything is double: the
 *   weight exp((double)t[e] - (double)lse[r]) with the library's exp (never a fast intrinsic), D, gs, the products with the feature
 *   words and the sums in any order -- also in the form scale (sum p gp K_j - D sum p K_j) of the row side.  There is one rounding to
 *   fp32 per output word.
 *   With u = 2^-24, delta_e and eta_e as in hisparse_attention.h (S_e = the exact sum of the fp32 products of Q and K, A_e = the sum of
 *   their magnitudes, delta_e = u |S_e| + d 2^-52 A_e + 2^-149, T_e = scale * S_e, eta_e = (1 + u) |scale| delta_e + u |T_e| + 2^-149),
 *   GP_e = the exact sum of the fp32 products of gY and V, A'_e = the sum of their magnitudes, P, D and GS exact from T_e, GP_e and the
 *   lse WORDS AS GIVEN, n_r = the row's length and m_c = the column's length:
 *       gam_e  = u |GP_e| + d 2^-52 A'_e + 2^-149
 *       rho_e  = expm1(eta_e + 32 2^-52)
 *       epsD_r = sum_{e in r} P_e (rho_e |GP_e| + (1 + rho_e) gam_e) + (n_r + 16) 2^-52 sum_{e in r} P_e |GP_e|
 *       eps_e  = |scale| (rho_e P_e |GP_e - D_r| + (1 + rho_e) P_e (gam_e + epsD_r))
 *       mag_e  = |scale| P_e (|GP_e| + |D_r|)
 *       |gq[r][j] - gQ| <= u |gQ| + sum_{e in r} eps_e |K_ej| + (n_r + 16) 2^-52 sum_{e in r} mag_e |K_ej| + 2^-149
 *       |gk[c][j] - gK| <= u |gK| + sum_{col = c} eps_e |Q_ej| + (m_c + 16) 2^-52 sum_{col = c} mag_e |Q_ej| + 2^-149
 *       |gv[c][j] - gV| <= u |gV| + sum_{col = c} rho_e P_e |gY_ej| + (m_c + 16) 2^-52 sum_{col = c} P_e |gY_ej| + 2^-149
 *   (every score is off by at most eta_e and the library's exp by a few ulp of a double, so every weight is off by at most rho_e
 *   relative; gam_e is gp's error; epsD_r is what both do to D; the 2^-52 terms are the double sums, with mag_e covering both sums of the
 *   row side's one-pass form.)  Dropping D from gs lands about 10^6 times outside these bounds. */
#ifndef HISPARSE_ATTENTION_BACKWARD_H_
#define HISPARSE_ATTENTION_BACKWARD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsab_pattern hsab_pattern;

int hsab_create(hsab_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr,
                const uint32_t* indices); /* indptr, indices: HOST arrays */
int hsab_destroy(hsab_pattern* p);
const char* hsab_last_error(const hsab_pattern* p); /* p == NULL: the last failed hsab_create of this thread */
int hsab_info(const hsab_pattern* p, uint64_t* nnz, uint64_t* device_bytes);
int hsab_set_stream(hsab_pattern* p, void* hip_stream); /* NULL restores the object's own stream */
int hsab_sync(hsab_pattern* p);
int hsab_backward_device(hsab_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv,
                         const float* gy_dev, uint64_t ldgy, const float* lse_dev, uint32_t d, float scale, float* gq_dev, uint64_t ldgq,
                         float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv);
int hsab_backward(hsab_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t d, float scale,
                  float* gq, float* gk, float* gv); /* host pointers, ld = d, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_ATTENTION_BACKWARD_H_ */
