// hs_spmm.cpp — the SpMM extension of include/hisparse_hip.h: Y = A X for k columns over the resident image.
#include "hs_context.h"

#include <algorithm>

extern "C" {

// SpMM as k SpMVs over the resident image (hisparse_hip.h): every column of X through the same kernels, so every column of Y is
// exactly what hs_run gives for it.
int hs_spmm_device(hs_context* ctx, const void* x_dev, uint64_t ldx, void* y_dev, uint64_t ldy, uint32_t k) {
    // (no settling on entry: the first column's step carries the caller's last combine; the matrix-engine and fused BITMAP routes leave
    // it owed until the closing settle)
    if (int rc = enter(ctx, kMatrix | kHostOnly)) return rc;
    MatrixData& m = ctx->mat;
    if (k == 0) return HS_OK;
    if (!x_dev || !y_dev) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    if ((reinterpret_cast<uintptr_t>(x_dev) & 15u) || (reinterpret_cast<uintptr_t>(y_dev) & 15u) || (ldx & 3u) || (ldy & 3u))
        return fail(ctx, HS_ERR_BAD_ARG, "device matrices must be 16-byte aligned with leading dimensions that are multiples of 4 words");
    if (ldx < m.num_cols || ldy < m.num_rows) return fail(ctx, HS_ERR_BAD_ARG, "leading dimensions must cover the padded column / row counts");
    if (int rc = enter(ctx, kNoSettle)) return rc;
    const bool is_float = ctx->is_float();
    const uint32_t* const x = static_cast<const uint32_t*>(x_dev);
    uint32_t* const y = static_cast<uint32_t*>(y_dev);
    uint32_t j = 0;
    // BITMAP images (dense rows: pruned-NN layers, which are multiplied with batches in practice): 4, then 2 columns at a time through
    // the fused kernel of spmm_bitmap.hip -- masks and values are streamed once for them.  Everything else, and a last odd column:
    // one SpMV per column.
    const char* fused_env = ctx_option(ctx, "HISPARSE_SPMM_FUSED");      // read per call (a test may change it)
    const bool fused_enabled = !(fused_env && std::string(fused_env) == "0");
    const char* mfma_env = ctx_option(ctx, "HISPARSE_SPMM_MFMA");
    // float BITMAP matrices, 16 columns at a time on the matrix engine: the matrix is streamed once per 16 columns and every x word is
    // shared by 16 rows in registers (spmm_mfma.hip)
    if (fused_enabled && !(mfma_env && std::string(mfma_env) == "0") && m.mfma.words && is_float) {
        // (5 .. 15 columns left over: still one pass -- 25 us on transformer-50 whatever it carries, against 25 us per FOUR columns of the fused kernel)
        while (k - j >= 5) {
            const uint32_t vectors = std::min<uint32_t>(16, k - j);
            hisparse::dev::SpmmMfmaLaunch a;
            a.vectors = vectors;
            a.words = m.mfma.words.get();
            a.offsets_word = m.mfma.info.offsets_word; a.values_word = m.mfma.info.values_word;
            a.tiles = m.mfma.info.tiles; a.groups = m.mfma.info.groups; a.chunk = m.mfma.info.chunk; a.chunks = m.mfma.info.chunks;
            a.x = x + size_t(j) * ldx;
            a.ldx = ldx;
            a.x_interleaved = m.mfma.x.get();
            a.partial = m.mfma.partial.get();
            a.flag = m.mfma.flag.get();
            a.call = ++ctx->mfma_call ? ctx->mfma_call : ++ctx->mfma_call;
            a.y = y + size_t(j) * ldy;
            a.ldy = ldy;
            a.num_rows = m.num_rows;
            a.num_cols = m.num_cols;
            HS_HIP(ctx, hisparse::dev::launch_spmm_mfma(a, ctx->stream));
            j += vectors;
        }
    }
    if (fused_enabled && m.launch.format == hisparse::dev::kFormatBitmap && m.col_slices == 1) {
        for (uint32_t group : {4u, 2u}) {
            if (m.max_block_rows > hisparse::dev::spmm_bitmap_max_block_rows(is_float, group)) continue;
            while (k - j >= group) {
                if (!m.x_interleaved) HS_HIP(ctx, m.x_interleaved.alloc(size_t(m.num_cols) * 4 * 4 + 64));
                hisparse::dev::SpmmLaunch a;
                a.image = m.image.get();
                a.blocks = m.blocks.get();
                a.units = m.units.get();
                a.x = x + size_t(j) * ldx;
                a.ldx = ldx;
                a.x_interleaved = m.x_interleaved.get();
                a.y = y + size_t(j) * ldy;
                a.ldy = ldy;
                a.vectors = group;
                a.num_cols = m.num_cols;
                a.num_workgroups = m.launch.num_workgroups;
                a.max_block_rows = m.max_block_rows;
                HS_HIP(ctx, hisparse::dev::launch_spmm_bitmap(is_float, a, ctx->stream));
                j += group;
            }
        }
    }
    // SWEEP images planned for it (option spmm_vectors = 4 at load time): four columns per pass through the matrix (spmm_sweep.hip); the
    // last pass may carry fewer (its missing columns are zero vectors whose results are not copied out)
    if (fused_enabled && m.launch.format == hisparse::dev::kFormatSweep && m.spmm_vectors == 4 && k - j >= 2) {
        if (int rc = settle(ctx)) return rc;
        const size_t rows = m.num_rows;
        if (!m.spmm_x4) HS_HIP(ctx, m.spmm_x4.alloc(size_t(m.num_cols) * 16 + 64));
        if (!m.spmm_y) HS_HIP(ctx, m.spmm_y.alloc(rows * 16));
        if (m.col_slices > 1 && !m.spmm_partial) HS_HIP(ctx, m.spmm_partial.alloc(size_t(m.col_slices) * rows * 16));
        while (j < k) {
            const uint32_t vectors = std::min<uint32_t>(4, k - j);
            hisparse::dev::SpmmSweepLaunch a;
            a.image = m.image.get();
            a.blocks = m.blocks.get();
            a.x = x + size_t(j) * ldx;
            a.ldx = ldx;
            a.x4 = m.spmm_x4.get();
            a.out = m.col_slices > 1 ? m.spmm_partial.get() : m.spmm_y.get();
            a.vectors = vectors;
            a.num_rows = m.num_rows;
            a.num_cols = m.num_cols;
            a.num_workgroups = m.launch.num_workgroups;
            a.max_block_rows = m.max_block_rows;
            HS_HIP(ctx, hisparse::dev::launch_spmm_sweep(is_float, a, ctx->stream));
            if (m.col_slices > 1)      // the four vectors' partial rows lie back to back inside a slice: ONE combine over 4 x rows "rows"
                HS_HIP(ctx, hisparse::dev::launch_combine_slices(is_float, m.spmm_partial.get(), m.spmm_y.get(), uint32_t(4 * rows), m.col_slices, 0,
                                                                 uint32_t(4 * rows), ctx->stream));
            HS_HIP(ctx, hipMemcpy2DAsync(y + size_t(j) * ldy, size_t(ldy) * 4, m.spmm_y.get(), rows * 4, rows * 4, vectors,
                                         hipMemcpyDeviceToDevice, ctx->stream));
            j += vectors;
        }
    }
    // one SpMV per column that is left; the last column's sum is not left owed to the caller's memory (run_steps)
    return run_steps(ctx, x + size_t(j) * ldx, ldx, y + size_t(j) * ldy, ldy, k - j);
}

int hs_spmm(hs_context* ctx, const void* packed_x, uint32_t num_cols, uint32_t k, void* packed_y, uint32_t num_rows) {
    if (int rc = enter(ctx, kMatrix | kHostOnly)) return rc;
    if (num_cols != ctx->mat.num_cols || num_rows != ctx->mat.num_rows) return fail(ctx, HS_ERR_BAD_ARG, "dimensions must equal the matrix's padded column / row counts");
    if (k == 0) return HS_OK;
    if (!packed_x || !packed_y) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    if (int rc = enter(ctx, kNoSettle)) return rc;
    const uint64_t ldx = (uint64_t(num_cols) + 3u) & ~uint64_t(3), ldy = (uint64_t(num_rows) + 3u) & ~uint64_t(3);
    DeviceBuffer<uint32_t> x, y;
    HS_HIP(ctx, x.alloc(size_t(ldx) * k * 4 + 64));
    HS_HIP(ctx, y.alloc(size_t(ldy) * k * 4));
    HS_HIP(ctx, hipMemcpy2DAsync(x.get(), size_t(ldx) * 4, packed_x, size_t(num_cols) * 4, size_t(num_cols) * 4, k, hipMemcpyHostToDevice, ctx->stream));
    const int rc = hs_spmm_device(ctx, x.get(), ldx, y.get(), ldy, k);      // (settled when it returns)
    if (rc != HS_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    HS_HIP(ctx, hipMemcpy2DAsync(packed_y, size_t(num_rows) * 4, y.get(), size_t(ldy) * 4, size_t(num_rows) * 4, k, hipMemcpyDeviceToHost, ctx->stream));
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return HS_OK;
}

}  // extern "C"
