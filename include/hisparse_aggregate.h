/* hisparse_aggregate.h — NEIGHBOUR AGGREGATION OVER A CSR PATTERN: sum, mean, max and min of the neighbours' feature rows, and the
 * backward that sends a gradient to the winning source only (EXTENSION; no reference counterpart).  Four calls on the pattern object of
 * hisparse_wide.h: hsw_create, hsw_destroy, hsw_info, hsw_set_stream, hsw_sync and hsw_last_error stay that header's, nothing is created
 * and nothing is allocated here (as hisparse_gat.h adds its calls to hisparse_heads.h's object).
 *
 * hsw_spmm_device is the weighted sum of the neighbours.  GraphSAGE-pool, GIN-max, PNA and PointNet / EdgeConv layers aggregate without
 * weights, and not only by a sum: with row(e), col(e) and the order of the entries as in hisparse_wide.h, n_r the entries of row r and X
 * a num_cols x ldx operand,
 *     ysum[r][j] = sum_{e in row r} X[col(e)][j]                      HSAGG_SUM   (HSAGG_MEAN: that sum / n_r, in the same output)
 *     ymax[r][j] = max_{e in row r} X[col(e)][j]                      HSAGG_MAX   amax[r][j] = the CSR index e of the winner
 *     ymin[r][j] = min_{e in row r} X[col(e)][j]                      HSAGG_MIN   amin[r][j] = the CSR index e of the winner
 * ONE launch computes every aggregator whose bit is set in `ops`, from ONE 16-byte gather of X[col(e)]'s chunk per entry: PNA's mean,
 * max and min are one pass over the pattern, not three.  No array of nnz x d words exists anywhere, and no array of nnz words either.
 *
 * hsagg_forward_device: any hsw_pattern.  Only the outputs whose bit is set in ops are touched, and their pointers must then be non-NULL
 *   (ysum_dev for HSAGG_SUM or HSAGG_MEAN, ymax_dev for HSAGG_MAX, ymin_dev for HSAGG_MIN); the pointers of the other outputs are not
 *   looked at.  amax_dev and amin_dev may be NULL (inference: no backward will ask for them).  All five outputs are num_rows x ldy.
 * hsagg_backward_device: needs HSW_TRANSPOSED (HS_ERR_UNSUPPORTED otherwise, as hsw_spmm_t_device); one launch over the transposed
 *   pattern.  With k the entries of column c in the order of the transposed pattern, r = row(k), e_k the CSR index of k and w_r = 1
 *   (HSAGG_MEAN: 1 / n_r),
 *     gx[c][j] = sum_{k: col = c} ( w_r gsum[r][j] + [amax[r][j] == e_k] gmax[r][j] + [amin[r][j] == e_k] gmin[r][j] )
 *   over the terms whose bit is set.  HSAGG_SUM / HSAGG_MEAN needs gsum_dev, HSAGG_MAX needs gmax_dev AND amax_dev, HSAGG_MIN gmin_dev AND
 *   amin_dev; the five are num_rows x ldg, gx is num_cols x ldgx.  An arg word is only ever COMPARED with e_k, never used as an address:
 *   a word that matches no entry (HSAGG_NONE, garbage) contributes nothing, whatever its gradient word holds.  A column without entries
 *   is d words of +0.0f.  Every output word has one writer and there are no atomics: two calls with the same inputs give the same words.
 *
 * THE WINNER RULE.  Candidate (v, e), the word v = X[col(e)][j] of entry e, is ranked
 *     1. a NaN outranks every non-NaN, for the maximum AND for the minimum (NaN propagates, as in torch.amax / torch.amin);
 *     2. among non-NaNs the IEEE comparison decides, > for the maximum and < for the minimum, so +0.0 and -0.0 are equal;
 *     3. among equals (equal under ==, or both NaN) the SMALLEST CSR INDEX wins.
 *   This is a lexicographic order on (rank, e), a total order on the entries of a row: the winner does not depend on how the entries are
 *   dealt to groups, lanes, trips or wavefronts, and both libraries give the same words.  Consequently
 *     ymax[r][j] is, BIT FOR BIT, the word X[indices[amax[r][j]]][j] (a NaN's payload and a zero's sign included), likewise ymin / amin;
 *     a row without entries gives +0.0f in ysum, ymax and ymin and HSAGG_NONE in amax and amin.
 *
 * LAYOUT AND REFUSALS: hisparse_wide.h's.  1 <= d <= 256; the feature pointers and the arg arrays (which share ldy / ldg with the floats
 *   beside them) are 16-byte aligned; every ld is a multiple of 4 and at least d; words d ... ld - 1 of an input row may be loaded but reach
 *   no result, words d ... ld - 1 of an output row are not written.  No output may share a byte with an input or with another output of
 *   the call.  ops == 0, a bit other than the four, or HSAGG_SUM together with HSAGG_MEAN is refused.  Every breach is HS_ERR_BAD_ARG,
 *   hsw_last_error(p) says why, and the object stays usable.  hsw_info is unchanged by these calls.  The _device forms allocate nothing,
 *   synchronise nothing, are ONE kernel launch each on the object's stream and can be captured into a graph.  d and ops may change from
 *   call to call.
 * hsagg_forward, hsagg_backward: the host-pointer forms, every ld = d exactly, no alignment rule beyond a word's; they copy in, run, copy
 *   out; synchronous; their transient device buffers are the only allocations.  A missing pointer of a set bit, a bad d or ops, or a
 *   result that overlaps an input or another result is HS_ERR_BAD_ARG.
 *
 * HOW THE WORK IS SCHEDULED: two kernel templates (neighbor_aggregate.hip) on the unchanged schedule of hisparse_wide.h: a lane owns one
 *   16-byte chunk of a feature row, a group covers the row, the groups of a team take different entries, four per group and trip, all four
 *   gathers issued before the first use; a row (forward) or column (backward) of any length runs on one workgroup.  A lane keeps four
 *   double sums and, per requested extreme, four (value, index) pairs; the groups of a team merge by lane shuffles and the four
 *   wavefronts of a long row through LDS, the pairs by the winner rule itself.  The aggregators are selected per launch by template
 *   (sum / max / min wanted or not: seven instantiations per side), so HSAGG_SUM alone carries no pair and HSAGG_MAX alone no sum.  The
 *   column side gathers, per entry and requested extreme, the arg chunk and the gradient chunk of the entry's row.  No scratch, no
 *   global atomics, no matrix engine.
 *
 * COST (MI355X; tools/aggregate_times.py, profiles/aggregate_times.txt; DESIGN.md section 6f has the table).  ogbl-ppa (576 K rows, 42.5 M
 *   entries), d = 16, 64 and 256, us: HSAGG_SUM 872, 1894 and 7689 -- SLOWER than hsw_spmm_device with an array of ones (792, 1728 and
 *   6771: ratio 1.10 to 1.14), so a caller who has that array loses nothing by staying; HSAGG_MEAN the same (877, 1899, 7694 against 793,
 *   1734, 6789 with an array of 1 / n_r); HSAGG_MAX with the args 948, 2047 and 7771, where torch index_select + scatter_reduce_(amax)
 *   takes 37 626 and 66 863 at d = 16 and 64 and was not run at d = 256 (its array is 43 GB); MEAN | MAX | MIN in one call 1714, 3517 and
 *   12 177 against 2776, 6005 and 23 288 for the three calls (0.62, 0.59, 0.52); the backward of MEAN | MAX 2755, 5309 and 20 309 against
 *   2224, 4756 and 16 684 for hsw_spmm_t_device plus the torch scatter of gmax (1.24, 1.12, 1.22: SLOWER -- per entry it gathers an arg
 *   chunk and a gradient chunk where that baseline scatters num_rows x d words; it saves the launches, the temporary and the atomics).
 *   transformer-50 (512 long rows): SUM 91, 341, 1025 against 91, 295, 1044; MAX 128, 485, 1792; one call for three 0.58 to 0.64; the
 *   backward 1.31 to 1.92 of its baseline.  Registers and LDS (no scratch): forward 68 VGPRs and 8 KiB for SUM alone, 82 and 8 KiB for one
 *   extreme, 106 and 24 KiB for all three; backward 88 to 168 VGPRs and 8 KiB.
 *
 * ARITHMETIC.  ymax, ymin, amax and amin are exact (words of X and indices).  A sum is formed in double in registers and rounded once to
 *   fp32; the mean is the double sum divided by double(n_r), then rounded once.  In the backward every term is formed in double --
 *   double(g), and with HSAGG_MEAN the ONE double division double(g) / double(n_r) -- and the terms of an output word are added in double,
 *   in any order, and rounded once.  With E the exact value (of the sum of the terms as just defined; for the mean, that sum over n_r), A
 *   the sum of the magnitudes of the terms (for the mean, over n_r), n their count and u = 2^-24:
 *       |result - E| <= u |E| + (n + 16) 2^-52 A + 2^-149
 *   Non-finite sums follow IEEE: NaN if a term is NaN or both infinities occur, the infinity if one occurs. */
#ifndef HISPARSE_AGGREGATE_H_
#define HISPARSE_AGGREGATE_H_

#include <stdint.h>

#include "hisparse_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSAGG_SUM 1u
#define HSAGG_MEAN 2u /* excludes HSAGG_SUM; same output slot */
#define HSAGG_MAX 4u
#define HSAGG_MIN 8u
#define HSAGG_NONE 0xFFFFFFFFu /* arg word of a row without entries */

int hsagg_forward_device(hsw_pattern* p, uint32_t ops, const float* x_dev, uint64_t ldx, uint32_t d, float* ysum_dev, float* ymax_dev,
                         uint32_t* amax_dev /* may be NULL */, float* ymin_dev, uint32_t* amin_dev /* may be NULL */, uint64_t ldy);
int hsagg_backward_device(hsw_pattern* p, uint32_t ops, const float* gsum_dev, const float* gmax_dev, const uint32_t* amax_dev,
                          const float* gmin_dev, const uint32_t* amin_dev, uint64_t ldg, uint32_t d, float* gx_dev, uint64_t ldgx);
int hsagg_forward(hsw_pattern* p, uint32_t ops, const float* x, uint32_t d, float* ysum, float* ymax, uint32_t* amax /* may be NULL */,
                  float* ymin, uint32_t* amin /* may be NULL */); /* host pointers, every ld = d, synchronous */
int hsagg_backward(hsw_pattern* p, uint32_t ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin,
                   const uint32_t* amin, uint32_t d, float* gx);

#ifdef __cplusplus
}
#endif

#endif /* HISPARSE_AGGREGATE_H_ */
