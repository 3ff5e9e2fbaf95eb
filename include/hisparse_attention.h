/* hisparse_attention.h — the attention step over a matrix's CSR pattern in ONE call: scores, row softmax and the weighted sum of the
 * value rows, with ROW-MAJOR dense operands and no per-entry array (EXTENSION; no reference counterpart).
 *
 * hisparse_wide.h and hisparse_rows.h do the forward step as three launches over two arrays of nnz words:
 *     hsw_sddmm_device (Q, K) = S  ->  hsr_softmax_device (S) = P  ->  hsw_spmm_device (P, V) = Y
 * Every score crosses device memory four times that way, and a caller who only wants Y (inference) or who would rather recompute P in
 * the backward step than keep it (training, per layer and head) has no use for S and P.  This object holds the pattern alone and does
 *     hsat_forward_device    Y[r][j] = sum_{e in row r} P[e] * V[col(e)][j]  and  lse[r],   Q: num_rows x ldq, K: num_cols x ldk,
 *                                                                                         V: num_cols x ldv, Y: num_rows x ldy, lse: num_rows words
 * in one kernel that gathers K's and V's row per entry and carries an online softmax between the two.  With row(e), col(e) and the order
 * of the entries as in hisparse_wide.h:
 *     s[e]   = sum_{j < d} Q[row(e)][j] * K[col(e)][j]
 *     t[e]   = scale * s[e]
 *     M_r    = max_{e in r} t[e]
 *     P[e]   = exp(t[e] - M_r) / sum_{e' in r} exp(t[e'] - M_r)
 *     Y[r][j] = sum_{e in r} P[e] * V[col(e)][j]
 *     lse[r] = M_r + log sum_{e in r} exp(t[e] - M_r)
 * lse, the row's log-sum-exp, is one word per row: P[e] = exp(t[e] - lse[row(e)]) recomputes the probabilities later, and two partial
 * attentions over disjoint column slabs merge through their lse words.  The BACKWARD step has no fused call yet: recompute S and P with
 * hsw_sddmm_device + hsr_softmax_device and run the five calls of hisparse_wide.h's chain.
 * (hisparse_attention_backward.h, added later, is that fused call: it reads lse and gives the three gradients in two launches.)
 *
 * ALL FEATURES ARE fp32, 1 <= d <= 256, and there is no impl argument, as in hisparse_wide.h.  Same library (libhisparse_hip.so;
 * libhisparse_cpu.so exports the same eight symbols on the host: plain loops on the calling thread, two passes per row, "device"
 * pointers are host pointers, hsat_set_stream accepts and ignores and hsat_sync is a no-op -- a second implementation, never a fallback:
 * without a usable gfx950 device this library's hsat_create fails with HS_ERR_NO_DEVICE / HS_ERR_HIP as hs_create does).  Error codes
 * are those of hisparse_hip.h.
 *
 * hsat_create: indptr[num_rows + 1] and indices[nnz] are HOST arrays and the validation is hsw_create's without its flags: an indptr
 *   that decreases or does not start at 0, or a column index >= num_cols, is HS_ERR_BAD_MATRIX; num_rows == 0, num_cols == 0 or a null
 *   pointer (indices may be NULL when nnz = 0) is HS_ERR_BAD_ARG; *out is then NULL and hsat_last_error(NULL) says why.  A pair held
 *   twice is two entries, the columns of a row may come in any order, nnz = 0 is a valid object.  EVERY allocation happens here: the
 *   object keeps on the device indptr, indices and the list of the rows sorted into the length classes of hisparse_wide.h,
 *       device_bytes = 4 (num_rows + 1) + 4 max(nnz, 1) + 4 num_rows
 *   which hsat_info reports beside nnz (either pointer may be NULL).  hsat_forward_device allocates nothing, synchronises nothing and is
 *   ONE kernel launch on the object's stream; it can be captured into a graph.
 *
 * LAYOUT of hsat_forward_device: hisparse_wide.h's.  Row i of a dense operand starts at word i * ld.  q_dev, k_dev, v_dev and y_dev are
 *   16-byte aligned, every ld is a multiple of 4 and at least d.  Words d ... ld - 1 of an input row may be loaded but reach no result: a
 *   NaN there changes nothing.  Words d ... ldy - 1 of an output row are not written.  lse_dev is a 4-byte aligned array of num_rows words,
 *   or NULL when the caller does not want it.  An operand of n rows reaches from its pointer to the end of the 16-byte chunk that holds
 *   word d - 1 of row n - 1 (that much must be the caller's memory); Y and lse may not share a byte with an input or with each other.
 *   scale must be finite (as in hsr_softmax_device).  Every breach is HS_ERR_BAD_ARG, hsat_last_error(p) says why, and the object
 *   stays usable.  d and scale may change from call to call.
 * HEADS.  H heads stored [index][head][feature] are H calls with ld = H * d and the four feature pointers offset by h * d words (lse: one
 *   array of num_rows words per head).  d must then be a multiple of 4, so that the offset pointers keep the 16-byte alignment; the words
 *   of the other heads lie in the pad of each row and reach no result.
 * hsat_forward: the host-pointer form, ld = d exactly for q, k, v and y, no alignment rule beyond a float's, lse may be NULL; it copies
 *   in, runs, copies out; synchronous; its transient device buffers are the only allocations outside hsat_create.
 *
 * SPECIAL ROWS.                          Y                          lse
 *     no entries                         d words of +0.0f           -inf
 *     every score -inf                   NaN in all d words         -inf
 *     a NaN or a +inf score              NaN in all d words         NaN
 *   No other row is touched by such a row.  A -inf score in a row with a finite maximum has weight exactly 0.  A zero weight times a
 *   non-finite word of V follows IEEE, as in hsw_spmm_device.  Every output word has exactly one writer and there are no atomics: two
 *   calls with the same inputs give the same words.
 *
 * HOW ROWS ARE SCHEDULED: exactly as in hisparse_wide.h (groups of lanes that cover a feature row in 16-byte chunks, teams of groups by
 *   the row's length class, the rows of more than 512 entries on a workgroup of their own and started first; A ROW OF ANY LENGTH RUNS ON
 *   ONE WORKGROUP).  The row's chunk of Q stays in registers.  Per trip a group takes four entries and issues their four gathers of K
 *   and four of V before the first use; it adds each entry's dot over its lanes by shuffles, rounds, scales, and updates its running
 *   state (m, l, the four sums of its chunk) with ONE rescale per trip.  The groups of a team merge their states by lane shuffles --
 *   the maximum first, then the rescaled sums -- and a long row's four wavefronts through LDS.  No matrix engine.
 *
 * STREAM ORDER: hisparse_wide.h's.  hsat_set_stream(NULL) restores the object's own stream; hsat_sync waits for the current one; a
 *   caller-owned stream must be synchronised by its owner before hsat_destroy.
 *
 * COST (MI355X; tools/attention_times.py, profiles/attention_times.txt; DESIGN.md section 6b has the table and the bar).  ogbl-ppa (576 K rows,
 *   42.5 M entries), d = 16 and 64: 1531 and 3496 us against 1795 and 3594 us for the chain's three calls in the same run (0.85, 0.97);
 *   transformer-50 (every row a long row): 147 and 581 us against 232 and 721.  The call costs what its two gathers cost.
 *
 * ARITHMETIC.
 *   Every product Q[r][j] * K[c][j] is ONE fp32 multiply (no FMA contraction: -ffp-contract=off); the d products of an entry are added
 *   in double, in any order, and s[e] is rounded once to fp32 -- exactly what hsw_sddmm_device promises.  t[e] = scale * s[e] is one
 *   fp32 multiply.  From there on everything is double: the weight exp((double)t[e] - (double)m) with the library's exp (never a fast
 *   intrinsic), where the running maximum m is one of the t words; the rescaling by exp(m_old - m_new); the products w * (double)V, the
 *   sums in any order, the quotient and m + log(l).  There is one rounding to fp32 per output word.
 *   With u = 2^-24, per entry S_e = the exact sum of the fp32 products, A_e = the sum of their magnitudes and
 *       delta_e = u |S_e| + d 2^-52 A_e + 2^-149,     T_e = scale * S_e,     eta_e = (1 + u) |scale| delta_e + u |T_e| + 2^-149,
 *   and per row, with P, Y and LSE exact from the T_e: eta_r = max_e eta_e, rho_r = expm1(eta_r), D_j = sum_e P_e |V_ej - Y_j|,
 *   B_j = sum_e P_e |V_ej|, n = the row's length:
 *       |y[r][j] - Y_j| <= u |Y_j| + rho_r / (1 - rho_r) D_j + (n + 16) 2^-52 B_j + 2^-149
 *       |lse[r] - LSE|  <= u |LSE| + eta_r + (n + 16) 2^-52 (1 + |LSE|) + 2^-149
 *   (every score is off by at most eta_e; a common shift cancels; a relative error rho on the weights moves a weighted mean by at most
 *   rho / (1 - rho) D).  fp32 weights would NOT keep this: the number of rescales of a row is bounded by its length alone. */
#ifndef HISPARSE_ATTENTION_H_
#define HISPARSE_ATTENTION_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsat_pattern hsat_pattern;

int hsat_create(hsat_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr,
                const uint32_t* indices); /* indptr, indices: HOST arrays */
int hsat_destroy(hsat_pattern* p);
const char* hsat_last_error(const hsat_pattern* p); /* p == NULL: the last failed hsat_create of this thread */
int hsat_info(const hsat_pattern* p, uint64_t* nnz, uint64_t* device_bytes);
int hsat_set_stream(hsat_pattern* p, void* hip_stream); /* NULL restores the object's own stream */
int hsat_sync(hsat_pattern* p);
int hsat_forward_device(hsat_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv,
                        uint32_t d, float scale, float* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */);
int hsat_forward(hsat_pattern* p, const float* q, const float* k, const float* v, uint32_t d, float scale, float* y,
                 float* lse /* may be NULL */); /* host pointers, ld = d, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_ATTENTION_H_ */
