// hs_spmspv.cpp — the SpMSpV extension of include/hisparse_hip.h (kernels: spmspv.hip): y = A x for a sparse x
// over the matrix once more in CSC form, with an opt-in dispatch to the dense SpMV of the loaded matrix above a crossover.
#include "hs_context.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using hisparse::Geometry;

extern "C" {

int hs_load_matrix_csc(hs_context* ctx, const uint32_t* indptr, const uint32_t* row_indices, const uint32_t* value_words, uint32_t num_rows,
                       uint32_t num_cols) {
    if (!ctx || !indptr || num_rows == 0 || num_cols == 0) return fail(ctx, HS_ERR_BAD_ARG, "null argument or empty matrix");
    const uint64_t nnz = indptr[num_cols];
    if (indptr[0] != 0 || (nnz && (!row_indices || !value_words))) return fail(ctx, HS_ERR_BAD_MATRIX, "indptr must start at 0; arrays missing");
    for (uint32_t c = 0; c < num_cols; ++c)
        if (indptr[c + 1] < indptr[c]) return fail(ctx, HS_ERR_BAD_MATRIX, "CSC indptr must be non-decreasing");
    for (uint64_t e = 0; e < nnz; ++e)
        if (row_indices[e] >= num_rows) return fail(ctx, HS_ERR_BAD_MATRIX, "CSC row index out of range");
    const uint32_t bins = hisparse::dev::spmspv_bins(num_rows), block_bits = hisparse::dev::spmspv_block_bits(num_rows);
    if (bins > hisparse::dev::spmspv_max_bins()) return fail(ctx, HS_ERR_UNSUPPORTED, "more than 16 384 row blocks of 16 384 rows (268 M rows)");
    if (nnz > 0xfffffff0ull) return fail(ctx, HS_ERR_UNSUPPORTED, "more than 2^32 non-zeros");
    // a bin per row block, as large as the block's share of the matrix: products of an x that names every column at most once always fit
    std::vector<uint32_t> bin_base(size_t(bins) + 1, 0);
    for (uint64_t e = 0; e < nnz; ++e) bin_base[(row_indices[e] >> block_bits) + 1]++;
    for (uint32_t b = 0; b < bins; ++b) bin_base[b + 1] += bin_base[b];
    if (int rc = enter(ctx, 0)) return rc;
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->csc = CscData();
    CscData& w = ctx->csc;
    HS_HIP(ctx, w.indptr.alloc((size_t(num_cols) + 1) * 4));
    HS_HIP(ctx, w.rows.alloc(std::max<size_t>(nnz, 1) * 4));
    HS_HIP(ctx, w.vals.alloc(std::max<size_t>(nnz, 1) * 4));
    w.capacity = std::max<uint64_t>(nnz, 1);
    HS_HIP(ctx, w.keys.alloc(size_t(w.capacity) * 4));
    HS_HIP(ctx, w.products.alloc(size_t(w.capacity) * 4));
    HS_HIP(ctx, w.bin_base.alloc((size_t(bins) + 1) * 4));
    HS_HIP(ctx, w.cursors.alloc(size_t(bins) * 4));
    HS_HIP(ctx, w.overflow.alloc(4));
    HS_HIP(ctx, hipMemcpy(w.bin_base.get(), bin_base.data(), bin_base.size() * 4, hipMemcpyHostToDevice));
    HS_HIP(ctx, hipMemset(w.cursors.get(), 0, size_t(bins) * 4));
    HS_HIP(ctx, hipMemset(w.overflow.get(), 0, 4));
    // y: also large enough for the dense SpMV's padded rows (dense dispatch of hs_spmspv writes it directly)
    w.y_words = std::max(num_rows, ctx->mat.loaded ? ctx->mat.num_rows : 0u);
    w.y_words = std::max<uint32_t>(w.y_words, uint32_t((uint64_t(num_rows) + ctx->geom.row_divisor - 1) / ctx->geom.row_divisor * ctx->geom.row_divisor));
    HS_HIP(ctx, w.y.alloc(size_t(w.y_words) * 4));
    HS_HIP(ctx, hipMemcpy(w.indptr.get(), indptr, (size_t(num_cols) + 1) * 4, hipMemcpyHostToDevice));
    if (nnz) {
        HS_HIP(ctx, hipMemcpy(w.rows.get(), row_indices, nnz * 4, hipMemcpyHostToDevice));
        HS_HIP(ctx, hipMemcpy(w.vals.get(), value_words, nnz * 4, hipMemcpyHostToDevice));
    }
    HS_HIP(ctx, hipMemset(w.y.get(), 0, size_t(w.y_words) * 4));
    w.col_len.resize(num_cols);
    for (uint32_t c = 0; c < num_cols; ++c) w.col_len[c] = indptr[c + 1] - indptr[c];
    w.num_rows = num_rows;
    w.num_cols = num_cols;
    ctx->dense_spmv_us = 0.0;
    return HS_OK;
}

namespace {

// one pass: expand + accumulate over `count` device-resident entries
int spmspv_pass(hs_context* ctx, const hisparse::dev::hs_idx_val_dev* x_dev, uint32_t count, bool add_to_y) {
    const CscData& w = ctx->csc;
    HS_HIP(ctx, hisparse::dev::launch_spmspv(ctx->is_float(), w.indptr.get(), w.rows.get(), w.vals.get(), x_dev, count, w.num_rows, w.num_cols, w.scratch(),
                                             add_to_y, w.y.get(), ctx->stream));
    return HS_OK;
}

// The dense SpMV instead (hs_spmspv above the crossover): x scattered into a zero vector, the context's loaded matrix, y into the SpMSpV
// result buffer.  Only when hs_load_matrix holds a matrix of the CSC matrix's shape (padded) -- the caller's contract is that it is the
// SAME matrix (hisparse_hip.h) -- and x names no column twice.
bool dense_dispatch_possible(const hs_context* ctx) {
    if (!ctx->mat.loaded) return false;
    const Geometry& g = ctx->geom;
    const uint64_t rows = (uint64_t(ctx->csc.num_rows) + g.row_divisor - 1) / g.row_divisor * g.row_divisor, cols = (uint64_t(ctx->csc.num_cols) + 7) / 8 * 8;
    return rows == ctx->mat.num_rows && cols == ctx->mat.num_cols && ctx->csc.y_words >= ctx->mat.num_rows;
}
int spmspv_dense(hs_context* ctx, const hisparse::dev::hs_idx_val_dev* x_dev, uint32_t count) {
    CscData& w = ctx->csc;
    if (!w.x_dense) HS_HIP(ctx, w.x_dense.alloc(size_t(ctx->mat.num_cols) * 4));
    HS_HIP(ctx, hisparse::dev::launch_spmspv_scatter_x(x_dev, count, ctx->mat.num_cols, w.x_dense.get(), ctx->stream));
    const int rc = run_steps(ctx, w.x_dense.get(), 0, w.y.get(), 0, 1);
    if (rc == HS_OK) ++ctx->spmspv_dense_dispatches;
    return rc;
}

}  // namespace

int hs_spmspv_device(hs_context* ctx, const hs_idx_val* x_entries_dev, uint32_t count) {
    if (int rc = enter(ctx, kCsc | kHostOnly, !count || x_entries_dev)) return rc;
    if (reinterpret_cast<uintptr_t>(x_entries_dev) & 7u) return fail(ctx, HS_ERR_BAD_ARG, "device entries must be 8-byte aligned");
    if (int rc = enter(ctx, 0)) return rc;
    return spmspv_pass(ctx, reinterpret_cast<const hisparse::dev::hs_idx_val_dev*>(x_entries_dev), count, false);
}

int hs_spmspv(hs_context* ctx, const hs_idx_val* x_entries, uint32_t count) {
    if (int rc = enter(ctx, kCsc, !count || x_entries)) return rc;
    CscData& w = ctx->csc;
    // One pass over the entries: range check, repeat check (a bit per column, kept zero between calls) and this call's product count.
    // A bin of the product list holds as many products as the matrix has non-zeros in that row block: an x that names a column more than once
    // can ask for more.  Such a call is cut into passes of UNIQUE columns -- pass i takes the i-th occurrence of every column: each pass fits by
    // construction -- y = first pass, y += the others (the sums are order-free: exact in fixed point, tolerance in float).  Repeats also rule
    // the dense dispatch out (two entries of one column are two separately rounded products, not one product of their sum).
    std::vector<uint32_t> pass_end;      // entries [pass_end[i-1], pass_end[i]) of the STAGED order form pass i
    bool repeats = false;
    uint64_t products = 0;
    {
        if (w.sx_seen.size() != (size_t(w.num_cols) + 7) / 8) w.sx_seen.assign((size_t(w.num_cols) + 7) / 8, 0);
        uint8_t* seen = w.sx_seen.data();
        uint32_t k = 0;
        for (; k < count; ++k) {
            const uint32_t col = x_entries[k].index;
            if (col >= w.num_cols) break;
            repeats |= (seen[col >> 3] >> (col & 7)) & 1u;
            seen[col >> 3] |= uint8_t(1u << (col & 7));
            products += w.col_len[col];
        }
        for (uint32_t j = 0; j < k; ++j) seen[x_entries[j].index >> 3] = 0;
        if (k < count) return fail(ctx, HS_ERR_BAD_ARG, "sparse vector index out of range");
    }
    if (count > w.sx_capacity) {
        HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        w.h_sx.reset();
        w.d_sx = nullptr;
        w.sx_capacity = 0;
        const uint32_t cap = std::max<uint32_t>(count, 1024);
        // pinned AND mapped: the expand kernel reads the entries straight out of host memory (8 bytes per entry, once, coalesced) -- no copy
        // command in front of it (an H2D of 46 KB put ~15 us between the call and its first kernel).  Two halves used in turn, so that the
        // host fills one while the previous call's kernels may still be reading the other.
        hisparse::dev::hs_idx_val_dev* pinned = nullptr;
        HS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&pinned), size_t(cap) * 2 * 8, hipHostMallocMapped));
        w.h_sx.adopt(pinned);
        HS_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&w.d_sx), pinned, 0));
        for (DeviceEvent& e : w.sx_read) HS_HIP(ctx, e.create(hipEventDisableTiming));
        w.sx_capacity = cap;
        w.sx_turn = 0;
    }
    const uint32_t half = w.sx_turn & 1u;
    w.sx_turn++;
    if (count) HS_HIP(ctx, hipEventSynchronize(w.sx_read[half].get()));      // the call before last read this half (long done, normally; a never-recorded event is complete)
    hisparse::dev::hs_idx_val_dev* const staged = w.h_sx.get() + size_t(half) * w.sx_capacity;
    const hisparse::dev::hs_idx_val_dev* const staged_dev = w.d_sx + size_t(half) * w.sx_capacity;
    if (!repeats) {
        if (count) std::memcpy(staged, x_entries, size_t(count) * sizeof(hs_idx_val));
        pass_end.push_back(count);
    } else {
        // occurrence number of every entry, then a stable counting sort by it into the staging buffer
        std::vector<uint32_t> occurrence(count), seen_times(w.num_cols, 0), per_pass;
        for (uint32_t k = 0; k < count; ++k) {
            occurrence[k] = seen_times[x_entries[k].index]++;
            if (occurrence[k] >= per_pass.size()) per_pass.resize(occurrence[k] + 1, 0);
            per_pass[occurrence[k]]++;
        }
        std::vector<uint32_t> at(per_pass.size(), 0);
        for (size_t i = 1; i < per_pass.size(); ++i) at[i] = at[i - 1] + per_pass[i - 1];
        for (size_t i = 0; i < per_pass.size(); ++i) pass_end.push_back(at[i] + per_pass[i]);
        for (uint32_t k = 0; k < count; ++k) {
            staged[at[occurrence[k]]].index = x_entries[k].index;
            staged[at[occurrence[k]]].val = x_entries[k].val;
            ++at[occurrence[k]];
        }
    }
    // Above the crossover the dense SpMV is faster (it reads every non-zero once, coalesced, at 6-8 bytes; the sparse path reads a column
    // entry, writes its product into a bin and reads it again): hisparse_hip.h.  The host knows this call's product count exactly (the
    // columns' lengths), the sparse path costs ~14 us + products / 45 G/s (profiles/r04_spmspv_binned.txt: ogbl-ppa, mouse_gene, pokec), and the dense SpMV of the
    // loaded matrix is TIMED once, on the first call that could use it (three launches on a zero vector and one synchronisation; hyper-
    // sparse matrices run at a third of the roofline, so no formula over the non-zero count would do).  `spmspv_crossover` (a fraction of
    // the columns) overrides the rule; `spmspv` = sparse | dense forces a path.
    const char* force = ctx_option(ctx, "HISPARSE_SPMSPV");
    const bool possible = !repeats && dense_dispatch_possible(ctx);
    bool want_dense = false;
    // The dense dispatch is OPT-IN: the CSC matrix is independent of the matrix hs_load_matrix holds -- a caller may keep
    // A for SpMV and A^T (or anything else of the same shape) as CSC -- and only the caller knows that the two are the same matrix.  It says
    // so with `spmspv` = auto (the rule below) | dense (always), or by setting `spmspv_crossover`; without one of them every call takes the
    // sparse path over the CSC arrays, whatever its size.
    const bool automatic = force && std::string(force) == "auto";
    if (force && !automatic) {
        want_dense = std::string(force) == "dense";
    } else if (const char* v = ctx_option(ctx, "HISPARSE_SPMSPV_CROSSOVER")) {
        const double crossover = std::atof(v);
        want_dense = crossover > 0.0 && double(count) > crossover * double(w.num_cols);
    } else if (automatic && possible && 14.0 + double(products) / 45000.0 > 30.0) {      // (below 30 us no dense SpMV of a matrix worth a CSC copy competes)
        if (ctx->dense_spmv_us <= 0.0) {
            if (!w.x_dense) {
                HS_HIP(ctx, w.x_dense.alloc(size_t(ctx->mat.num_cols) * 4));
                HS_HIP(ctx, hipMemsetAsync(w.x_dense.get(), 0, size_t(ctx->mat.num_cols) * 4, ctx->stream));
            }
            // one warm step, then three timed.  A carried plan owes the last step's sum to the result buffer then; if the rule below takes
            // the SPARSE path, that combine would run after spmspv_pass and overwrite its y with A*0: time_steps settles it inside the region
            double us = -1.0;
            if (int rc = time_steps(ctx, w.x_dense.get(), w.y.get(), /*warm=*/1, /*regions=*/1, /*runs=*/3, &us)) return rc;
            if (us > 0.0) ctx->dense_spmv_us = std::max(1.0, us);
        }
        // + the scatter of x into the zero vector (a memset and a small kernel: ~8 us)
        want_dense = ctx->dense_spmv_us > 0.0 && 14.0 + double(products) / 45000.0 > ctx->dense_spmv_us + 8.0;
    }
    int rc = HS_OK;
    if (want_dense && possible) {
        rc = spmspv_dense(ctx, staged_dev, count);
    } else {
        uint32_t begin = 0;
        for (size_t i = 0; i < pass_end.size() && rc == HS_OK; ++i) {
            rc = spmspv_pass(ctx, staged_dev + begin, pass_end[i] - begin, i != 0);
            begin = pass_end[i];
        }
    }
    if (count && rc == HS_OK) HS_HIP(ctx, hipEventRecord(w.sx_read[half].get(), ctx->stream));      // the kernels that read the staging buffer are behind this
    return rc;
}

int hs_read_spmspv_result(hs_context* ctx, void* packed_y, uint32_t num_rows) {
    if (int rc = enter(ctx, kCsc | kHostOnly, packed_y != nullptr)) return rc;
    if (num_rows != ctx->csc.num_rows) return fail(ctx, HS_ERR_BAD_ARG, "result length must equal the CSC matrix's row count");
    if (int rc = enter(ctx, 0)) return rc;
    const CscData& w = ctx->csc;
    uint32_t overflow = 0;
    HS_HIP(ctx, hipMemcpyAsync(packed_y, w.y.get(), size_t(num_rows) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HS_HIP(ctx, hipMemcpyAsync(&overflow, w.overflow.get(), sizeof(overflow), hipMemcpyDeviceToHost, ctx->stream));
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (overflow) {      // only hs_spmspv_device can get here: hs_spmspv cuts such a call into passes
        HS_HIP(ctx, hipMemset(w.overflow.get(), 0, sizeof(overflow)));
        HS_HIP(ctx, hipMemset(w.cursors.get(), 0, size_t(hisparse::dev::spmspv_bins(w.num_rows)) * 4));
        return fail(ctx, HS_ERR_BAD_ARG, "hs_spmspv_device: the entries asked for more products than the matrix has non-zeros (columns named more than "
                                         "once): the result is incomplete; hs_spmspv with host entries splits such a call");
    }
    return HS_OK;
}

int hs_spmspv_status(hs_context* ctx, uint32_t* overflowed, void** overflow_word_dev) {
    if (int rc = enter(ctx, kCsc | kHostOnly)) return rc;
    if (overflow_word_dev) *overflow_word_dev = ctx->csc.overflow.get();
    if (overflowed) {      // (only reading the word back touches the stream)
        if (int rc = enter(ctx, 0)) return rc;
        HS_HIP(ctx, hipMemcpyAsync(overflowed, ctx->csc.overflow.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HS_OK;
}

}  // extern "C"
