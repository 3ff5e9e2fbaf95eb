/* hisparse_heads.h — MULTI-HEAD attention over a matrix's CSR pattern, forward and backward, ALL HEADS OF A CALL IN ONE PASS over the
 * pattern: forward is ONE launch, backward is TWO, and no per-entry array exists at any point (EXTENSION; no reference counterpart).
 *
 * hisparse_attention.h and hisparse_attention_backward.h do one head per call; H heads stored [index][head][feature] are H calls there,
 * each of which gathers a d * 4-byte piece out of a row of H * d * 4 bytes and reads indptr and indices again.  This object gathers the
 * whole row of H * d words once per entry and keeps one softmax state (forward) or one D word (backward) per head:
 *     hsmh_forward_device    Y: num_rows x ldy and lse: num_rows x ldl   from   Q: num_rows rows, K, V: num_cols rows
 *     hsmh_backward_device   gQ: num_rows x ldgq, gK: num_cols x ldgk, gV: num_cols x ldgv   from   Q, gY, K, V and lse
 * Per head h these are exactly the formulas of the two single-head headers applied to the head's d words:
 *     s[e][h]   = sum_{j < d} Q[row(e)][h d + j] * K[col(e)][h d + j]        t[e][h] = scale * s[e][h]
 *     P[e][h]   = the row softmax of t[.][h]                                  lse[r][h] = the row's log-sum-exp of t[.][h]
 *     Y[r][h d + j]  = sum_{e in r} P[e][h] * V[col(e)][h d + j]
 *     GP[e][h]  = sum_{j < d} gY[row(e)][h d + j] * V[col(e)][h d + j]       D[r][h] = sum_{e in r} P[e][h] * GP[e][h]
 *     GS[e][h]  = scale * P[e][h] * (GP[e][h] - D[row(e)][h])                 with P[e][h] = exp(t[e][h] - lse[row(e)][h]) in the backward
 *     gQ[r][h d + j] = sum_{e in r} GS[e][h] * K[col(e)][h d + j]
 *     gK[c][h d + j] = sum_{col(e) = c} GS[e][h] * Q[row(e)][h d + j]
 *     gV[c][h d + j] = sum_{col(e) = c} P[e][h] * gY[row(e)][h d + j]
 * One scale serves all heads.
 *
 * ALL FEATURES ARE fp32 and there is no impl argument, as in hisparse_wide.h.  Same library (libhisparse_hip.so; libhisparse_cpu.so
 * exports the same ten symbols on the host: plain loops on the calling thread, two passes per row, "device" pointers are host pointers,
 * hsmh_set_stream accepts and ignores and hsmh_sync is a no-op -- a second implementation, never a fallback: without a usable gfx950
 * device this library's hsmh_create fails with HS_ERR_NO_DEVICE / HS_ERR_HIP as hs_create does).  Error codes are those of
 * hisparse_hip.h.
 *
 * SHAPES ACCEPTED: d in {4, 8, 16, 32, 64, 128, 256} (a head is a power-of-two number of 16-byte chunks), 1 <= heads <= max_heads <= 64
 *   and heads * d <= 256.  Anything else is HS_ERR_BAD_ARG and the message names the rule; every other d is covered by the per-head
 *   calls of hsat_forward_device / hsab_backward_device (the HEADS paragraphs of their headers).  heads, d and scale may change from call
 *   to call.
 *
 * hsmh_create: indptr[num_rows + 1] and indices[nnz] are HOST arrays and the validation is hsat_create's: an indptr that decreases or
 *   does not start at 0, or a column index >= num_cols, is HS_ERR_BAD_MATRIX; num_rows == 0, num_cols == 0 or a null pointer (indices
 *   may be NULL when nnz = 0) is HS_ERR_BAD_ARG.  In addition max_heads outside 1 ... 64 and unknown flag bits (HSMH_BACKWARD = 1 is the
 *   only one) are HS_ERR_BAD_ARG.  *out is then NULL and hsmh_last_error(NULL) says why.  A pair held twice is two entries, the columns
 *   of a row may come in any order, nnz = 0 is a valid object.  EVERY allocation happens here.  Without HSMH_BACKWARD the object keeps
 *   what an hsat object keeps, indptr, indices and the list of the rows sorted into the length classes of hisparse_wide.h:
 *       device_bytes = 4 (num_rows + 1) + 4 max(nnz, 1) + 4 num_rows
 *   With HSMH_BACKWARD it also keeps the transposed pattern and its class list as an hsab object does, and one double per row and
 *   head, the D words, stored [row][max_heads]:
 *       device_bytes += 4 (num_cols + 1) + 4 max(nnz, 1) + 4 num_cols + 8 num_rows max_heads
 *   hsmh_info reports exactly that beside nnz (either pointer may be NULL).  hsmh_backward and hsmh_backward_device on an object created
 *   without the flag are HS_ERR_BAD_ARG.  hsmh_forward_device is ONE kernel launch and hsmh_backward_device exactly TWO on the object's
 *   stream; neither allocates or synchronises, and both can be captured into a graph (one linear branch).
 *   ONE BACKWARD CALL MAY BE IN FLIGHT PER OBJECT, because of the D words, as in hisparse_attention_backward.h.
 *
 * LAYOUT of the _device calls.  Word j of head h of row i of a feature operand sits at i * ld + h * d + j.  The feature pointers are
 *   16-byte aligned, every ld is a multiple of 4 and at least heads * d.  Words heads * d ... ld - 1 of an input row may be loaded but
 *   reach no result: a NaN there changes nothing.  Words heads * d ... ld - 1 of an output row are not written.  lse of (row r, head h)
 *   sits at r * ldl + h, ldl >= heads, with 4-byte alignment: [row][head], so that the column side of the backward reads the H words of
 *   an entry's row from one place.  Words h >= heads of a row of lse are neither read nor written.  lse may be NULL in the forward and
 *   is REQUIRED in the backward.  A feature operand of n rows reaches from its pointer to the end of the 16-byte chunk that holds its
 *   last word (word heads * d - 1 of row n - 1); lse reaches ((num_rows - 1) * ldl + heads) * 4 bytes.  That much must be the caller's
 *   memory.  An output (lse of the forward among them) may not share a byte with an input or with another output.  scale must be
 *   finite.  Every breach is HS_ERR_BAD_ARG, hsmh_last_error(p) says why, and the object stays usable.
 * hsmh_forward / hsmh_backward: the host-pointer forms, ld = heads * d exactly for every feature array and ldl = heads, no alignment rule
 *   beyond a float's; they copy in, run, copy out; synchronous; their transient device buffers are the only allocations outside
 *   hsmh_create.  lse may be NULL in hsmh_forward.
 *
 * SPECIAL ROWS AND VALUES: per head, the tables of hisparse_attention.h (SPECIAL ROWS) and hisparse_attention_backward.h (SPECIAL
 *   VALUES).  A row without entries is +0.0f in all heads * d words of Y and of gQ and -inf in all heads words of lse; a column without
 *   entries is +0.0f in all heads * d words of gK and gV.  HEADS DO NOT LEAK: a NaN, a +-inf score or a non-finite lse word in one head
 *   reaches only that head's d words of that row and that head's d words of the columns the row touches; the other heads of the same
 *   rows and columns are computed as if it were not there.  Every output word has exactly one writer and there are no atomics: two
 *   calls with the same inputs give the same words.
 *
 * HOW THE WORK IS SCHEDULED: all three kernels exactly as in hisparse_wide.h, taken at the width heads * d (groups of lanes that cover
 *   the heads * d words of a row in 16-byte chunks, teams of groups by the length class, more than 512 entries on a workgroup of their
 *   own and started first; A ROW, AND A COLUMN, OF ANY LENGTH RUNS ON ONE WORKGROUP).  Inside a group the d / 4 lanes of a head add the
 *   head's dots by shuffles among themselves and share the head's weight; every lane carries its own head's running maximum and sum
 *   (forward) or D (backward).  The groups of a team merge lane by lane through shuffles, the four wavefronts of a long row or column
 *   lane by lane through LDS.  Lanes of a group past heads * d / 4 (3 heads of d = 16 in a group of 16 lanes) compute on head 0's
 *   addresses and store nothing.  No matrix engine.
 *
 * STREAM ORDER: hisparse_wide.h's.  hsmh_set_stream(NULL) restores the object's own stream; hsmh_sync waits for the current one; a
 *   caller-owned stream must be synchronised by its owner before hsmh_destroy.  A training step with H heads on one stream is three
 *   launches: hsmh_forward_device, then (after the caller's own work on Y) hsmh_backward_device.
 *
 * COST (MI355X; tools/heads_times.py, profiles/heads_times.txt; DESIGN.md section 6b has the table and the bar): the one call against
 *   the `heads` per-head calls it replaces, measured in the same run.  ogbl-ppa (576 K rows, 42.5 M entries), 4 heads of d = 16: 3465 us
 *   forward and 8125 us backward against 6454 and 16990 us for the four per-head calls each (0.54, 0.48); 8 heads of d = 16: 0.53 and
 *   0.46; 4 heads of d = 64 and 2 of d = 128, where a head alone is whole cache lines: 0.91 / 0.86 and 0.99 / 0.95.  transformer-50:
 *   0.82 to 0.94 forward, 0.73 to 0.96 backward.  The call costs what its gathers of whole rows of heads * d words cost.  The object
 *   holds 386 MB on ogbl-ppa with max_heads = 8 and hsmh_create takes 462 ms there (the host's counting sort of the transposed pattern).
 *
 * ARITHMETIC: per head, the ARITHMETIC blocks of hisparse_attention.h and hisparse_attention_backward.h with the head's d words: one
 *   fp32 multiply per product (no FMA contraction: -ffp-contract=off), the d products of a head and entry added in double in any order,
 *   s rounded once to fp32, t = scale * s one fp32 multiply, everything after that in double with the library's exp and log, one
 *   rounding to fp32 per output word.  The error bounds are those of the two headers, per head, with d the head's width and n_r, m_c the
 *   row's and the column's length. */
#ifndef HISPARSE_HEADS_H_
#define HISPARSE_HEADS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsmh_pattern hsmh_pattern;

#define HSMH_BACKWARD 1u /* keep the transposed pattern and the D words: hsmh_backward and hsmh_backward_device */

int hsmh_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices,
                uint32_t max_heads, uint32_t flags); /* indptr, indices: HOST arrays */
int hsmh_destroy(hsmh_pattern* p);
const char* hsmh_last_error(const hsmh_pattern* p); /* p == NULL: the last failed hsmh_create of this thread */
int hsmh_info(const hsmh_pattern* p, uint64_t* nnz, uint64_t* device_bytes);
int hsmh_set_stream(hsmh_pattern* p, void* hip_stream); /* NULL restores the object's own stream */
int hsmh_sync(hsmh_pattern* p);
int hsmh_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv,
                        uint32_t heads, uint32_t d, float scale, float* y_dev, uint64_t ldy, float* lse_dev /* may be NULL */, uint64_t ldl);
int hsmh_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, uint32_t heads, uint32_t d, float scale, float* y,
                 float* lse /* may be NULL */); /* host pointers, ld = heads * d, ldl = heads, synchronous */
int hsmh_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv,
                         const float* gy_dev, uint64_t ldgy, const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float scale,
                         float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv);
int hsmh_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t heads, uint32_t d,
                  float scale, float* gq, float* gk, float* gv); /* host pointers, ld = heads * d, ldl = heads, synchronous */

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_HEADS_H_ */
