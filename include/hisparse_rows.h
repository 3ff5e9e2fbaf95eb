/* hisparse_rows.h — the row softmax over a matrix's CSR pattern, forward and backward (EXTENSION; no reference counterpart).
 *
 * hisparse_pattern.h computes edge scores in the order of the CSR arrays; hs_update_values_device (hisparse_hip.h) takes matrix values
 * in that order.  What sits between them in graph attention and sparse attention is a softmax of the scores over every row:
 *     forward    t[e] = scale * s[e],  m = max_row t,  d[e] = t[e] - m,  p[e] = exp(d[e]) / sum_row exp(d[e'])
 *     backward   D = sum_row p[e'] gp[e'],  gs[e] = scale * p[e] * (gp[e] - D)          (the gradient with respect to the scores s)
 * where row i owns the entries e in [indptr[i], indptr[i + 1]).  With it the attention step runs on one caller-owned stream, in one
 * array order and with no host round trip:
 *     forward    hsp_sddmm_device -> hsr_softmax_device (in place) -> hs_update_values_device -> hs_run / hs_spmm_device
 *     backward   on the transposed context: hsp_sddmm_device (the gradient of the values) -> hsr_softmax_backward_device
 *
 * The operation needs only indptr -- no columns, no numeric mode, no context: it is an object of its own, hsr_rows.  ALL VALUES ARE
 * fp32 in every case (hs_update_values_device takes float in all three numeric modes), so there is no impl argument.  Same library
 * (libhisparse_hip.so; libhisparse_cpu.so exports the same ten symbols on the host: one loop on the calling thread, "device" pointers
 * are host pointers, hsr_set_stream accepts and ignores and hsr_sync is a no-op -- a second implementation, never a fallback: without a usable gfx950
 * device this library's hsr_create fails with HS_ERR_NO_DEVICE / HS_ERR_HIP as hs_create does).  Error codes are those of hisparse_hip.h.
 *
 * hsr_create: indptr[num_rows + 1] is a HOST array, exactly what hs_load_matrix_csr and hsp_create take.  Validation on the host, before
 *   anything is allocated on the device: an indptr that decreases or does not start at 0 is HS_ERR_BAD_MATRIX; num_rows == 0 or a null
 *   pointer is HS_ERR_BAD_ARG; *out is then NULL and hsr_last_error(NULL) says why.  nnz = indptr[num_rows] = 0 is a valid object: its
 *   calls succeed and touch nothing.  The object keeps on the device: indptr, a list of the non-empty rows sorted into length classes
 *   (one word per non-empty row; below) and a table of 16 words that maps workgroups to classes.  EVERY allocation happens here: the
 *   _device calls allocate nothing, synchronise nothing and are one kernel launch each on the object's stream.  hsr_info reports nnz and the device bytes the
 *   object holds (either pointer may be NULL):
 *       device_bytes = 4 (num_rows + 1) + 4 max(non-empty rows, 1) + 64
 *
 * hsr_softmax_device: s_dev and p_dev hold nnz fp32 words in CSR order.  p_dev == s_dev exactly is allowed (in place); any other overlap
 *   of the two nnz-word ranges is refused.  Empty rows write nothing.  A row of one entry gives p = 1.0f exactly.
 * hsr_softmax_backward_device: p_dev is the forward's result, gp_dev the gradient with respect to p, gs_dev receives the gradient with
 *   respect to s; `scale` is the forward's.  gs_dev may equal gp_dev exactly (in place); it may not overlap p_dev or partially overlap
 *   gp_dev.
 * Both: pointers non-null and 4-byte aligned, scale finite; every refusal is HS_ERR_BAD_ARG, hsr_last_error(r) says why, and the object
 *   stays usable.  Asynchronous on the object's stream.
 * hsr_softmax, hsr_softmax_backward: the host-pointer forms (nnz words each; the same in-place and overlap rules; no alignment rule).
 *   They copy in, run, copy out; synchronous; their transient device buffers are the only allocations outside hsr_create.
 *
 * HOW ROWS ARE SCHEDULED.  hsr_create sorts every non-empty row into a class by its length n:
 *     group classes  G = 4, 8, 16, 32, 64 lanes per row, the smallest G with n <= 4 G: a lane holds at most four scores in registers, the
 *                    row is read once and written once, max and sum are reduced by lane shuffles inside the group; a wavefront
 *                    (64 lanes) serves 64 / G rows;
 *     long rows      n > 256: one workgroup of 256 lanes per row; passes (max, sum, write; backward: sum, write) separated by workgroup
 *                    barriers, reductions by shuffles and then LDS; the first 1024 entries stay in registers, the rest is read again
 *                    in every pass.
 *   One launch serves all classes; the long rows are started first, longest first.  A ROW OF ANY LENGTH RUNS ON ONE WORKGROUP: a row of
 *   millions of entries is correct but takes the time 256 lanes need for it; splitting a row across workgroups is not done.
 *
 * COST (MI355X; tools/rows_times.py, profiles/rows_times.txt).  ogbl-ppa (576 K rows, 42.5 M entries): 209 us forward, 145 us
 *   backward; transformer-50 (512 rows of about 16 600 entries, all long rows): 59 us and 46 us.  That is 1.2 to 3.6 TB/s of the bytes a
 *   call must move (8 nnz forward, 12 nnz backward), below the 6.3 TB/s of a streaming kernel: the forward call pays expf and a double-precision
 *   division per entry, and a workload of few long rows has one workgroup per row to work with.
 *
 * STREAM ORDER WITH A CONTEXT AND A PATTERN.  Give one caller-owned stream to all three: hs_set_stream on the context, hsp_set_stream on
 *   the pattern, hsr_set_stream on the rows.  On a caller-owned stream every context call completes in itself (hisparse_hip.h, hs_run),
 *   so hsp_sddmm_device -> hsr_softmax_device -> hs_update_values_device -> hs_run are ordered by the stream alone; nothing needs a host
 *   synchronisation.  hsr_set_stream(NULL) restores the object's own stream; hsr_sync waits for the current one.  A caller-owned stream
 *   must be synchronised by its owner before hsr_destroy.
 *
 * ARITHMETIC.
 *   Forward: t = scale * s is one fp32 multiply, the maximum is exact, d = t - m is one fp32 subtract.  The exponential is expf (the
 *     device library's, libm's in libhisparse_cpu.so; both documented at most 1 ulp off; never the fast __expf), widened to double; the row
 *     sum is taken in double, in any order; the quotient is taken in double and rounded once to fp32.  With d the fp32 word above,
 *     E[e] = exp(d[e]) exactly and P = E / sum E (the sum is >= 1: the maximum contributes exp(0)):
 *         |p - P| <= 3 * 2^-23 * P + 2^-125
 *     (1 ulp in the numerator, 1 ulp in the sum, half an ulp in the final rounding; the absolute term covers a flushed denormal).
 *     scale = 0 gives (float)(1.0 / n) bit for bit.
 *   Backward: the products p * gp are formed in double (exact there), D is summed in double in any order, scale * p (exact in double)
 *     times (gp - D) is rounded once to fp32.  With G the exact value, n the row length and A = sum_row |p gp|:
 *         |gs - G| <= 2^-23 |G| + |scale| p[e] (n + 4) 2^-52 (A + |gp[e]|) + 2^-149
 *   Non-finite inputs follow IEEE through these formulas.  A -inf score in a row whose maximum is finite gives exactly 0; a row that holds
 *     a NaN, a +inf, or only -inf gives NaN in every entry of that row and in no other row (what torch.softmax gives). */
#ifndef HISPARSE_ROWS_H_
#define HISPARSE_ROWS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsr_rows hsr_rows;

int hsr_create(hsr_rows** out, int device_id, uint32_t num_rows, const uint32_t* indptr); /* indptr: HOST array, num_rows + 1 words */
int hsr_destroy(hsr_rows* r);
const char* hsr_last_error(const hsr_rows* r); /* r == NULL: the last failed hsr_create of this thread */
int hsr_info(const hsr_rows* r, uint64_t* nnz, uint64_t* device_bytes);
int hsr_set_stream(hsr_rows* r, void* hip_stream); /* NULL restores the object's own stream */
int hsr_sync(hsr_rows* r);
int hsr_softmax_device(hsr_rows* r, const float* s_dev, float scale, float* p_dev);
int hsr_softmax_backward_device(hsr_rows* r, const float* p_dev, const float* gp_dev, float scale, float* gs_dev);
int hsr_softmax(hsr_rows* r, const float* s, float scale, float* p); /* host pointers, synchronous */
int hsr_softmax_backward(hsr_rows* r, const float* p, const float* gp, float scale, float* gs);

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_ROWS_H_ */
