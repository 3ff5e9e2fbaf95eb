/* hisparse_pattern.h — the sampled dense product (SDDMM) over a matrix's CSR pattern (EXTENSION; no reference counterpart).
 *
 * The callers of hs_update_values / hs_load_matrix_csr_transposed (hisparse_hip.h) keep a sparsity pattern and change its numbers: the
 * forward product y = W x, the backward product g_x = W^T g_y, then new values.  The product that MAKES the new values is this one:
 *     out[e] = sum_{j < k} U_j[row(e)] (x) V_j[col(e)]            for every entry e of the pattern, in CSR order
 * -- dW[e] = sum_j g_y_j[row(e)] x_j[col(e)] of a sparse layer, the edge score <h_row(e), h_col(e)> of a graph.  The result is in the
 * order of the CSR arrays, the order hs_update_values_device takes: forward, backward, gradient and update work on one array order, with
 * no reload and no host round trip.
 *
 * The product needs nothing a context holds (no image, no plan, no x / y), only the pattern: it is an object of its own, hsp_pattern.
 * Same library (libhisparse_hip.so; libhisparse_cpu.so exports the same symbols on host threads, where "device" pointers are host
 * pointers, hsp_set_stream accepts and ignores and hsp_sync is a no-op -- a second implementation, never a fallback: without a usable
 * gfx950 device this library's hsp_create fails with HS_ERR_NO_DEVICE / HS_ERR_HIP as hs_create does).  Error codes and HS_IMPL_* are
 * those of hisparse_hip.h.
 *
 * hsp_create: indptr[num_rows + 1] and indices are HOST arrays, exactly what hs_load_matrix_csr takes (unpadded dimensions).  Columns
 *   inside a row may come in any order; a (row, column) pair held twice is two entries, each with its own output word.  Validation as
 *   the CSR load, on the host, before anything is allocated on the device: an index >= num_cols, an indptr that decreases or does not
 *   start at 0 is HS_ERR_BAD_MATRIX; max_k outside 1 ... 64, an unknown impl, a zero dimension or a null pointer is HS_ERR_BAD_ARG; *out
 *   is then NULL and hsp_last_error(NULL) says why.  The object keeps on the device: the column of every entry, the row of every entry
 *   (expanded from indptr by a kernel, 4 bytes per entry) and two staging buffers for max_k vectors (below).  EVERY allocation happens
 *   here: hsp_sddmm_device allocates nothing, is asynchronous and can be captured into a hipGraph.  hsp_info reports the entries and the
 *   device bytes the object holds (either pointer may be NULL).
 *
 * hsp_sddmm_device: U_j at u_dev + j * ldu words (num_rows words used), V_j at v_dev + j * ldv words (num_cols words used); words are
 *   value words of the numeric mode -- the layouts of hs_read_result and hs_load_vector, so ldu = padded_rows and ldv = padded_cols of a
 *   context work directly.  u_dev, v_dev and out_dev 16-byte aligned, ldu >= num_rows and ldv >= num_cols multiples of 4 (the rules of
 *   hs_spmm_device); 1 <= k <= max_k.  out_dev holds nnz words: fp32 in the float modes (hs_update_values_device and a caller's optimiser
 *   read them as they are), Q8.24 words in fixed point.  accumulate = 1 adds to what out_dev holds (batches wider than 64, mini-batch
 *   chunks), accumulate = 0 overwrites.  Asynchronous on the object's stream.  With k >= 2 the call first transposes U and V into the
 *   staging buffers in groups of four vectors ([group][index][4], a last group padded with zero words in BOTH operands), then makes one
 *   pass over the entries whatever k is; k = 1 gathers from u_dev / v_dev directly.
 * hsp_sddmm: the host-pointer form.  Columns back to back with ldu = num_rows rounded up to 4 and ldv = num_cols rounded up to 4 (u holds
 *   k * ldu words, v holds k * ldv, out nnz); copies in, runs with accumulate = 0, copies out; synchronous.
 *
 * STREAM ORDER WITH A CONTEXT.  Give one caller-owned stream to both: hs_set_stream on the context, hsp_set_stream on the pattern.  On a
 *   caller-owned stream every context call completes in itself (hisparse_hip.h, hs_run), so hs_run -> hsp_sddmm_device on the context's y
 *   -> hs_update_values_device are ordered by the stream alone; nothing needs a host synchronisation.  hsp_set_stream(NULL) restores the
 *   object's own stream; hsp_sync waits for the current one.  A caller-owned stream must be synchronised by its owner before hsp_destroy.
 *
 * ARITHMETIC (as the ARITHMETIC block of hisparse_hip.h; its symbols are used here).
 *   Fixed point: every product is q8_24_mul (AP_RND then AP_SAT -- the product of the SpMV kernels, spmv_device.h), the sum of an entry is
 *     saturated once at 2^32 - 1: bit-exact in any order.  accumulate is a saturating add: the same words as one call over all the
 *     vectors would give.
 *   Float (both float modes are the same here): one fp32 multiply per (entry, j), no FMA contraction; the products are added in double
 *     from +0.0 in ascending j and rounded once.  With p the k fp32 products of an entry, E their exact sum, A = sum |p| and u = 2^-24:
 *         |out - E| <= u |E| + k 2^-52 A + 2^-149                                  (class L = 1, n = k of that contract)
 *     With accumulate over S calls the partials are rounded once each and added in fp32:
 *         |out - E| <= gamma(S) A + k 2^-52 A + S 2^-149                           (as S passes there)
 *     Non-finite results follow IEEE double summation of p; 0 x inf = NaN reaches its entry (the padding of a last group is 0 x 0 in both
 *     operands and never 0 x inf).  The sign of a zero result is not promised. */
#ifndef HISPARSE_PATTERN_H_
#define HISPARSE_PATTERN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsp_pattern hsp_pattern;

int hsp_create(hsp_pattern** out, int device_id, int impl, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices,
               uint32_t max_k);
int hsp_destroy(hsp_pattern* p);
const char* hsp_last_error(const hsp_pattern* p); /* p == NULL: the last failed hsp_create of this thread */
int hsp_info(const hsp_pattern* p, uint64_t* nnz, uint64_t* device_bytes);
int hsp_set_stream(hsp_pattern* p, void* hip_stream); /* NULL restores the object's own stream */
int hsp_sync(hsp_pattern* p);
int hsp_sddmm_device(hsp_pattern* p, const void* u_dev, uint64_t ldu, const void* v_dev, uint64_t ldv, uint32_t k, void* out_dev, int accumulate);
int hsp_sddmm(hsp_pattern* p, const void* u, const void* v, uint32_t k, void* out);

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_PATTERN_H_ */
