/* hisparse_wide.h — the three products of the attention / sparse-training chain over a matrix's CSR pattern, with ROW-MAJOR dense
 * operands (EXTENSION; no reference counterpart).
 *
 * hisparse_pattern.h and the contexts of hisparse_hip.h take a dense operand as a stack of SpMV vectors, [vector][index].  Callers of
 * the chain hold node features, [index][feature] with 16 to 256 features per node, and their sparse values -- probabilities, score
 * gradients -- change on every step.  This object holds the pattern alone and does the chain's three products in that layout, with the
 * values read from a device array in CSR order on every call: no image, no value map, no hs_update_values_device, no context.
 *     hsw_sddmm_device    out[e] = sum_{j < d} U[row(e)][j] * V[col(e)][j]              U: num_rows x ldu, V: num_cols x ldv, out: nnz words
 *     hsw_spmm_device     Y[r][j] = sum_{e in row r} w[e] * X[col(e)][j]                X: num_cols x ldx, Y: num_rows x ldy
 *     hsw_spmm_t_device   Y[c][j] = sum_{e: col(e) = c} w[e] * X[row(e)][j]             X: num_rows x ldx, Y: num_cols x ldy
 * where e runs over the entries in the order of the CSR arrays, row i owns [indptr[i], indptr[i + 1]) and col(e) = indices[e].  w and
 * out are in that order in all three calls: hsw_spmm_t_device takes w exactly as hsw_spmm_device does.  With hisparse_rows.h the
 * attention step is, on one caller-owned stream and with zero contexts:
 *     forward    hsw_sddmm_device (Q, K) -> hsr_softmax_device -> hsw_spmm_device (P, V)
 *     backward   hsw_spmm_t_device (P, gY) = gV;  hsw_sddmm_device (gY, V) = gP;  hsr_softmax_backward_device = gS;
 *                hsw_spmm_device (gS, K) = gQ;  hsw_spmm_t_device (gS, Q) = gK
 *
 * ALL VALUES AND FEATURES ARE fp32 and there is no impl argument, as in hisparse_rows.h (the softmax on both sides of these products is
 * fp32 in every numeric mode; fixed-point callers keep the context path).  Same library (libhisparse_hip.so; libhisparse_cpu.so exports
 * the same twelve symbols on the host: plain loops on the calling thread, "device" pointers are host pointers, hsw_set_stream accepts and
 * ignores and hsw_sync is a no-op -- a second implementation, never a fallback: without a usable gfx950 device this library's hsw_create
 * fails with HS_ERR_NO_DEVICE / HS_ERR_HIP as hs_create does).  Error codes are those of hisparse_hip.h.
 *
 * hsw_create: indptr[num_rows + 1] and indices[nnz] are HOST arrays, exactly what hs_load_matrix_csr and hsp_create take, and the
 *   validation is hsp_create's, on the host, before anything is allocated on the device: an indptr that decreases or does not start at
 *   0, or a column index >= num_cols, is HS_ERR_BAD_MATRIX; num_rows == 0, num_cols == 0, a null pointer (indices may be NULL when
 *   nnz = 0) or a flag bit other than HSW_TRANSPOSED is HS_ERR_BAD_ARG; *out is then NULL and hsw_last_error(NULL) says why.  A (row,
 *   column) pair held twice is two entries; the columns of a row may come in any order; nnz = 0 is a valid object (its hsw_sddmm*
 *   write nothing, its hsw_spmm* write zeros).  The object keeps on the device indptr, indices and a list of the rows sorted into length
 *   classes (one word per row; below).  With HSW_TRANSPOSED it also keeps the transposed pattern, built by a counting sort on the host:
 *   column pointers, the row of every entry in column order, the CSR index of every such entry (where hsw_spmm_t_device fetches w[e])
 *   and the list of the columns by length class.  The transposed pattern is STABLE: the entries of a column are in ascending CSR index.
 *   hsw_spmm_t* on an object created without the flag is HS_ERR_UNSUPPORTED.  EVERY allocation happens here: the _device calls allocate
 *   nothing, synchronise nothing and are ONE kernel launch each on the object's stream.  hsw_info reports nnz and the device bytes the
 *   object holds (either pointer may be NULL):
 *       device_bytes = 4 (num_rows + 1) + 4 max(nnz, 1) + 4 num_rows
 *                      + with HSW_TRANSPOSED: 4 (num_cols + 1) + 8 max(nnz, 1) + 4 num_cols
 *
 * LAYOUT of the _device calls.  Row i of a dense operand starts at word i * ld; an operand of n rows holds n * ld words.  Feature
 *   pointers (u_dev, v_dev, x_dev, y_dev) are 16-byte aligned, every ld is a multiple of 4 and at least d, and 1 <= d <= 256.  Words
 *   d ... ld - 1 of an input row may be loaded but are never used: a NaN there reaches no result.  Words d ... ldy - 1 of an output row are
 *   not written.  w_dev and out_dev are 4-byte aligned arrays of nnz words.  The output range (nnz words; num_rows * ldy or num_cols * ldy
 *   words) may not share a byte with an input range.  Every breach is HS_ERR_BAD_ARG, hsw_last_error(p) says why, and the object stays
 *   usable.  d may change from call to call.
 * VALUES.  A row without entries is written as d words of +0.0f by hsw_spmm_device, and so is a column without entries by
 *   hsw_spmm_t_device.  Every output word has exactly one writer and there are no memory-side atomics: two calls with the same inputs
 *   give the same words.
 * hsw_sddmm, hsw_spmm, hsw_spmm_t: the host-pointer forms, ld = d exactly for every dense operand (u: num_rows x d, and so on), no
 *   alignment rule beyond a float's; they copy in, run, copy out; synchronous; their transient device buffers are the only allocations outside hsw_create.
 *   A null pointer, a bad d or a result that overlaps an input is HS_ERR_BAD_ARG.
 *
 * HOW ROWS ARE SCHEDULED.  All three calls are scheduled by row (hsw_spmm_t_device by the rows of the transposed pattern), and one
 *   16-byte gather brings four features of an entry's row:
 *     group     the lanes that cover one feature row, four features each: ceil(d / 4) rounded up to a power of two (1 ... 64);
 *     team      the groups that work on one row; they take different entries, four per group and trip, so every lane keeps four gathers
 *               in flight.  hsw_create sorts the rows by length n into classes that want 4 (n <= 4, the empty rows included), 16
 *               (n <= 16) and 64 (n <= 512) groups; a team never exceeds a wavefront (64 lanes), so short rows share one, team beside
 *               team, and at d > 128 every such team is one group;
 *     long rows n > 512: one workgroup of 256 lanes per row, started first, longest first.
 *   Sums are doubles in registers; a team's groups are added by lane shuffles, a long row's four wavefronts through 8 KiB of LDS.
 *   hsw_sddmm_device holds the row's chunk of U in registers for the whole row and adds the lanes of a group by shuffles per entry.  A
 *   ROW OF ANY LENGTH RUNS ON ONE WORKGROUP: splitting a row across workgroups is not done.
 *
 * COST (MI355X; tools/wide_times.py, profiles/wide_times.txt; DESIGN.md section 6b has the table).  ogbl-ppa (576 K rows, 42.5 M entries), d = 16
 *   and 64: hsw_sddmm_device 789 and 1679 us (hsp_sddmm_device with k = d: 2661 and 11922), hsw_spmm_device 789 and 1746 us
 *   (hs_update_values_device + hs_spmm_device: 1535 and 4357), hsw_spmm_t_device 1719 and 2948 us (1606 and 4439).  transformer-50 (512 rows
 *   of about 16 600 entries: 512 workgroups, every row a long row) is where the row schedule loses: hsw_sddmm_device 86 and 374 us against
 *   74 and 257, hsw_spmm_device 93 and 290 us against 102 and 176.  hsw_create: 40 ms on ogbl-ppa, 457 ms with HSW_TRANSPOSED.
 *
 * STREAM ORDER.  As hisparse_rows.h: give one caller-owned stream to every object of a chain (hsw_set_stream, hsr_set_stream, ...); the
 *   calls are then ordered by the stream alone.  hsw_set_stream(NULL) restores the object's own stream; hsw_sync waits for the current
 *   one.  A caller-owned stream must be synchronised by its owner before hsw_destroy.
 *
 * ARITHMETIC (class D, L = 1 of tests/float_contract.py).
 *   Every product -- U[r][j] * V[c][j], w[e] * X[c][j] -- is ONE fp32 multiply (no FMA contraction: -ffp-contract=off).  The products of
 *   one output word are added in double, in any order, and the sum is rounded once to fp32.  With E the exact sum of the fp32 products,
 *   A the sum of their magnitudes, n their count (d for hsw_sddmm*, the row's or the column's length for hsw_spmm* / hsw_spmm_t*) and
 *   u = 2^-24:
 *       |result - E| <= u |E| + n 2^-52 A + 2^-149
 *   Non-finite words follow IEEE summation of the products, which no order changes: NaN if a product is NaN or both infinities occur,
 *   the infinity if one occurs.  The sign of a zero result is not promised, except that a row or column without entries is +0.0f. */
#ifndef HISPARSE_WIDE_H_
#define HISPARSE_WIDE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsw_pattern hsw_pattern;

#define HSW_TRANSPOSED 1u /* hsw_create: keep the transposed pattern too (hsw_spmm_t*) */

int hsw_create(hsw_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices,
               uint32_t flags); /* indptr, indices: HOST arrays */
int hsw_destroy(hsw_pattern* p);
const char* hsw_last_error(const hsw_pattern* p); /* p == NULL: the last failed hsw_create of this thread */
int hsw_info(const hsw_pattern* p, uint64_t* nnz, uint64_t* device_bytes);
int hsw_set_stream(hsw_pattern* p, void* hip_stream); /* NULL restores the object's own stream */
int hsw_sync(hsw_pattern* p);
int hsw_sddmm_device(hsw_pattern* p, const float* u_dev, uint64_t ldu, const float* v_dev, uint64_t ldv, uint32_t d, float* out_dev);
int hsw_spmm_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy);
int hsw_spmm_t_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy);
int hsw_sddmm(hsw_pattern* p, const float* u, const float* v, uint32_t d, float* out); /* host pointers, ld = d, synchronous */
int hsw_spmm(hsw_pattern* p, const float* w, const float* x, uint32_t d, float* y);
int hsw_spmm_t(hsw_pattern* p, const float* w, const float* x, uint32_t d, float* y);

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_WIDE_H_ */
