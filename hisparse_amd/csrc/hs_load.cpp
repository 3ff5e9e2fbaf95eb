// hs_load.cpp — hs_load_matrix (CPSR channel buffers), hs_load_matrix_csr and hs_load_matrix_csr_transposed behind one body, the opt-in autotune around it,
// hs_update_values and the debug reads of what a load left on the device (include/hisparse_hip.h).
#include "hs_context.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "hisparse/channel_packets.h"

using hisparse::Geometry;
using hisparse::dev::Block;
using hisparse::dev::Unit;

namespace {

constexpr size_t kImageSlackBytes = 16384;  // the clamped prefetches of a wavefront without chunks (offset w * 512 past a short block) stay inside the allocation

// plan-time option value_map = 1: hs_load_matrix_csr keeps the value map of hs_update_values
bool value_map_asked(const hs_context* c) {
    const char* v = ctx_option(c, "HISPARSE_VALUE_MAP");
    return v && std::atoi(v) != 0;
}

template <typename T>
hipError_t upload(DeviceBuffer<T>& dst, const void* src, size_t bytes, size_t slack) {
    const hipError_t e = dst.alloc(std::max<size_t>(bytes + slack, 256));
    if (e != hipSuccess || bytes == 0) return e;
    return hipMemcpy(dst.get(), src, bytes, hipMemcpyHostToDevice);
}

// `csr_in` != nullptr: the CSR source (channel / n_packets null).  want_map: build the value map of hs_update_values if the option asks
// for it (autotune's candidate loads do not)
int load_matrix_once(hs_context* ctx, const void* const* channel, const uint64_t* n_packets, const hisparse::dev::CsrView* csr_in,
                     uint32_t num_rows, uint32_t num_cols, uint32_t num_row_partitions, uint32_t num_col_partitions, bool want_map) {
    const Geometry& g = ctx->geom;
    if (num_rows == 0 || num_cols == 0) return fail(ctx, HS_ERR_BAD_ARG, "empty matrix");
    if (num_rows % g.row_divisor != 0 || num_cols % hisparse::PACK_SIZE != 0)
        return fail(ctx, HS_ERR_BAD_ARG, "dimensions are not padded: rows must divide by " + std::to_string(g.row_divisor) +
                                             " and columns by 8 (util_round_csr_matrix_dim)");
    if (num_row_partitions != (num_rows + g.logical_ob - 1) / g.logical_ob || num_col_partitions != (num_cols + g.logical_vb - 1) / g.logical_vb)
        return fail(ctx, HS_ERR_BAD_ARG, "partition counts do not match the dimensions and the bank sizes of this context");
    if (int rc = enter(ctx, 0)) return rc;
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_matrix(ctx);
    MatrixData& m = ctx->mat;
    const auto t0 = std::chrono::steady_clock::now();
    const bool map_on = value_map_asked(ctx);
    hisparse::dev::CsrView csr_view;
    const hisparse::dev::CsrView* csr = nullptr;
    if (csr_in) {
        csr_view = *csr_in;
        csr_view.value_map = map_on && want_map;
        csr_view.plain_values = map_on;
        csr = &csr_view;
    }

    hisparse::dev::StreamTiles tiles;
    std::string why;
    // What a builder leaves on the device belongs to the context the moment the builder returns: no exit below needs a cleanup call --
    // free_matrix (the next load, hs_destroy) gives it back; m.loaded stays false until the end.
    auto adopt_device_images = [&]() {
        m.image.adopt(tiles.d_image);
        m.mfma.words.adopt(reinterpret_cast<uint32_t*>(tiles.mfma.d_words));
        m.value_map.adopt(tiles.d_value_map);
        m.mfma.value_map.adopt(tiles.d_value_map2);
        tiles.d_image = nullptr;
        tiles.mfma.d_words = nullptr;
        tiles.d_value_map = tiles.d_value_map2 = nullptr;
    };
    auto start_over_on_host = [&]() {      // a device build that gave up: its images go back before the host builder allocates
        adopt_device_images();
        m = MatrixData();
        tiles = hisparse::dev::StreamTiles();
    };
    // The per-non-zero passes of the re-tiling run on the GPU (gpu_tiles.h) unless HISPARSE_RETILE=host; BITMAP images and matrices
    // with duplicate entries are built by the host code, which also remains the byte-for-byte checker of the GPU path.
    const hisparse::dev::detail::OptionScope option_scope(&ctx->options);      // this context's hs_set_option values rule the planning below
    const char* retile = hisparse::dev::detail::env_switch("HISPARSE_RETILE");
    bool on_gpu = csr || !(retile && std::string(retile) == "host");
    int rc = HS_OK;
    try {
        // one 1024-thread workgroup per CU: its row accumulators and x ring fill the 160 KiB LDS
        bool ok = hisparse::dev::build_stream_tiles(channel, n_packets, g, num_rows, num_cols, num_row_partitions, num_col_partitions,
                                                    uint32_t(ctx->compute_units), tiles, why, ctx->stream, on_gpu, kImageSlackBytes, csr);
        if (!ok && csr && why == "gpu re-tile: duplicate entries") {
            // A (row, column) that occurs twice is legal input for the reference's formatter (csr2cpsr keeps both entries and the PEs add
            // both products), but the device sort has no defined order among equal positions.  Do what a reference driver does instead:
            // format on the host (sw/benchmark.cpp:110-195) and hand the CPSR buffers to the host builder, like hs_load_matrix does for
            // such a matrix.
            // (A transposed load formats A^T's own CSR, made on the host here: HostCsr, tiles_common.h.)
            start_over_on_host();
            const hisparse::dev::detail::HostCsr rows(csr);
            on_gpu = false;
            if (rows.ok()) {      // (the device passes have checked every index already)
                spmv::io::CSRMatrix<float> mat;
                mat.num_rows = rows->num_rows;
                mat.num_cols = rows->num_cols;
                const uint64_t nnz = rows->indptr[rows->num_rows];
                mat.adj_indptr.assign(rows->indptr, rows->indptr + rows->num_rows + 1);
                mat.adj_indices.assign(rows->indices, rows->indices + nnz);
                mat.adj_data.assign(rows->values, rows->values + nnz);
                const hisparse::ChannelPackets packets = hisparse::format_matrix(mat, g, /*skip_empty_rows=*/true);
                const void* chan[hisparse::NUM_HBM_CHANNELS];
                uint64_t count[hisparse::NUM_HBM_CHANNELS];
                for (uint32_t c = 0; c < hisparse::NUM_HBM_CHANNELS; ++c) { chan[c] = packets.channel[c].data(); count[c] = packets.channel[c].size(); }
                ok = packets.num_rows == num_rows && packets.num_cols == num_cols &&
                     hisparse::dev::build_stream_tiles(chan, count, g, num_rows, num_cols, num_row_partitions, num_col_partitions, uint32_t(ctx->compute_units), tiles, why);
            } else {
                why = "CSR column index outside the matrix";
            }
        }
        if (!ok && !csr && on_gpu && why.rfind("gpu re-tile:", 0) == 0) {       // duplicates, or a HIP failure on the way: the host path decides
            start_over_on_host();
            on_gpu = false;
            ok = hisparse::dev::build_stream_tiles(channel, n_packets, g, num_rows, num_cols, num_row_partitions, num_col_partitions,
                                                   uint32_t(ctx->compute_units), tiles, why);
        }
        if (!ok) rc = fail(ctx, why == hisparse::dev::detail::kBadMfmaChunk ? HS_ERR_BAD_ARG : HS_ERR_BAD_MATRIX, why);      // (an option of the environment the load cannot take)
    } catch (const std::bad_alloc&) {
        rc = fail(ctx, HS_ERR_NO_MEMORY, "out of host memory while re-tiling the matrix");
    } catch (const std::exception& e) {      // whatever a builder task threw (WorkerPool rethrows it): never through the C ABI
        rc = fail(ctx, HS_ERR_BAD_MATRIX, std::string("re-tiling the matrix failed: ") + e.what());
    } catch (...) {
        rc = fail(ctx, HS_ERR_BAD_MATRIX, "re-tiling the matrix failed");
    }
    const bool image_on_device = tiles.d_image != nullptr, mfma_on_device = tiles.mfma.d_words != nullptr;
    adopt_device_images();
    if (rc != HS_OK) return rc;
    const bool debug = ctx_option(ctx, "HISPARSE_PLAN_DEBUG") != nullptr;
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (debug) std::fprintf(stderr, "load: image built after %.1f ms\n", since());
    // (BITMAP: + the block's stretch of x behind the accumulators when the builder asks for it, spmv_bitmap.hip kXLds)
    const uint32_t lds_bytes = tiles.format == hisparse::dev::kFormatSweep ? hisparse::dev::spmv_sweep_lds_bytes(tiles.max_block_rows, ctx->is_float())
                               : tiles.light ? hisparse::dev::spmv_light_lds_bytes(tiles.max_block_rows)
                                           : hisparse::dev::spmv_lds_bytes(tiles.max_block_rows, tiles.ring_buffers, tiles.format) +
                                                 tiles.bitmap_x_groups * hisparse::dev::kBitmapGroupCols * 4u;
    if (lds_bytes > hisparse::dev::kMaxLdsBytes) return fail(ctx, HS_ERR_UNSUPPORTED, "row block does not fit the LDS");

    // the dynamic-LDS cap is a property of the FUNCTION, not of this context: always raise it to the full 160 KiB, so that a
    // second context with a smaller matrix on the same device cannot lower it under a first one's launches
    HS_HIP(ctx, hisparse::dev::configure_spmv_kernels(hisparse::dev::kMaxLdsBytes));
    if (!image_on_device)      // (built on the device: adopted above, slack included)
        HS_HIP(ctx, upload(m.image, tiles.image.data(), tiles.image.size(), kImageSlackBytes));
    HS_HIP(ctx, upload(m.blocks, tiles.blocks.data(), tiles.blocks.size() * sizeof(Block), 0));
    HS_HIP(ctx, upload(m.units, tiles.units.data(), tiles.units.size() * sizeof(Unit), 0));
    HS_HIP(ctx, upload(m.part_heads, tiles.part_heads.data(), tiles.part_heads.size() * sizeof(uint32_t), 0));
    HS_HIP(ctx, m.y.alloc(size_t(num_rows) * 4));
    HS_HIP(ctx, hipMemset(m.y.get(), 0, size_t(num_rows) * 4));  // the host zero-initialises y (sw/benchmark.cpp:217-222)
    // the two decisions of stream_tiles.h, unless an option decides otherwise
    const uint64_t image_bytes = image_on_device ? tiles.image_bytes : uint64_t(tiles.image.size());
    const char* resident_opt = ctx_option(ctx, "HISPARSE_STREAM_RESIDENT");
    // (stream residency: the load says whether the image MAY be streamed resident; each launch decides whether it is: hs_api.cpp, launch_args)
    m.resident_forced = resident_opt ? int(std::atoi(resident_opt) != 0) : -1;
    m.resident_eligible = hisparse::dev::stream_policy_applies(tiles.format, tiles.light) &&
                          hisparse::dev::plan_stream_resident(tiles.format, tiles.light, image_bytes, tiles.units.size(), tiles.blocks.size());
    m.image_id = hisparse::next_image_id();
    m.image_bytes = image_bytes;
    const char* carry_opt = ctx_option(ctx, "HISPARSE_CARRY_COMBINE");
    // (a packed DELTA image is judged by the size of its plain form here too: packing changes the bytes of a step, not which of the two regimes it is in)
    const uint64_t carry_bytes = tiles.format == hisparse::dev::kFormatDelta && tiles.value_bits == 24
                                     ? image_bytes / hisparse::dev::kRecordBytes24 * hisparse::dev::kRecordBytes : image_bytes;
    const bool carries = tiles.col_slices > 1 && (carry_opt ? std::atoi(carry_opt) != 0 : hisparse::dev::plan_carries(tiles.format, carry_bytes));
    HS_HIP(ctx, ctx->carry.reset(ctx->is_float(), num_rows, num_cols, tiles.col_slices, carries));
    if (mfma_on_device || (tiles.mfma.words_bytes != 0 && !tiles.mfma.words.empty())) {      // float BITMAP matrix: the second image for the SpMM on the matrix engine + its scratch
        // OPTIONAL: SpMV works without it.  If the image or its scratch cannot be had (out of memory), the matrix loads without a second
        // image (and without a map into it) and hs_spmm takes the fused 4-column kernel instead.
        const hisparse::dev::MfmaImage& mi = tiles.mfma;
        MatrixData::Mfma& mf = m.mfma;
        bool ok = mfma_on_device || upload(mf.words, mi.words.data(), mi.words.size(), 0) == hipSuccess;
        ok = ok && mf.x.alloc(hisparse::dev::spmm_mfma_x_words(mi.groups) * 4) == hipSuccess &&
             mf.partial.alloc(hisparse::dev::spmm_mfma_partial_words(mi.tiles, mi.chunks) * 4) == hipSuccess &&
             mf.flag.alloc(64) == hipSuccess && hipMemset(mf.flag.get(), 0, 64) == hipSuccess;
        if (ok) {
            mf.info = std::move(tiles.mfma);
            mf.info.words = {};
        } else {
            (void)hipGetLastError();
            mf = MatrixData::Mfma();
        }
    }
    // the value map: kept, or why there is none (hs_update_values reports it)
    if (m.value_map) {
        m.value_map_nnz = tiles.nnz;
        m.value_map_why.clear();
    } else if (!map_on) {
        m.value_map_why = "the value_map option was off when the matrix was loaded";
    } else if (!csr) {
        m.value_map_why = "the matrix came from hs_load_matrix (CPSR): only hs_load_matrix_csr and hs_load_matrix_csr_transposed keep a value map";
    } else if (!image_on_device) {
        m.value_map_why = "the image was built by the host builder (duplicate (row, column) entries, bitmap_build=host, or SWEEP chunks spanning more than 65535 "
                          "columns): it has no value map";
    } else {
        m.value_map_why = "the image is 16 GiB or larger: its word indices do not fit 32 bits";
    }
    if (debug) std::fprintf(stderr, "load: descriptors + result buffers on the device after %.1f ms\n", since());
    m.num_rows = num_rows;
    m.num_cols = num_cols;
    m.row_parts = num_row_partitions;
    m.col_slices = tiles.col_slices;
    m.spmm_vectors = tiles.spmm_vectors;
    if (tiles.spmm_vectors == 4) {
        const uint32_t need = hisparse::dev::spmm_sweep_lds_bytes(tiles.max_block_rows, ctx->is_float());
        if (need > hisparse::dev::kMaxLdsBytes) m.spmm_vectors = 1;      // (cannot happen with the planner's row cap; the k-SpMV path then)
        else HS_HIP(ctx, hisparse::dev::configure_spmm_sweep_kernels(hisparse::dev::kMaxLdsBytes));
    }
    for (const Block& b : tiles.blocks) m.crossing_blocks = m.crossing_blocks || b.last_part != b.row_part;
    m.max_block_rows = tiles.max_block_rows;
    hisparse::dev::SpmvLaunch& a = m.launch;
    a.image = m.image.get();
    a.blocks = m.blocks.get();
    a.units = m.units.get();
    a.part_heads = m.part_heads.get();
    a.ring_buffers = tiles.ring_buffers;
    a.format = tiles.format;
    a.value_bits = tiles.value_bits;
    a.num_cols = num_cols;
    a.num_workgroups = tiles.num_workgroups;
    a.lds_bytes = lds_bytes;
    a.bitmap_x_groups = tiles.bitmap_x_groups;
    a.light = tiles.light;
    ctx->dense_spmv_us = 0.0;
    m.loaded = true;

    hs_stats& s = ctx->stats;
    s = hs_stats{};
    s.nnz = tiles.nnz;
    for (int c = 0; n_packets && c < HS_NUM_CHANNELS; ++c) s.cpsr_bytes += n_packets[c] * sizeof(hisparse::MatPkt);
    s.stream_bytes = tiles.image_bytes;
    s.stream_elements = tiles.elements;
    s.num_blocks = uint32_t(tiles.blocks.size());
    s.num_units = uint32_t(tiles.units.size());
    s.col_slices = tiles.col_slices;
    s.ring_buffers = tiles.ring_buffers;
    s.stream_format = tiles.format;
    s.num_workgroups = tiles.num_workgroups;
    s.lds_bytes = lds_bytes;
    s.num_compute_units = uint32_t(ctx->compute_units);
    s.load_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    s.retiled_on_gpu = image_on_device;
    s.light_kernel = tiles.light ? 1u : 0u;
    s.value_bits = tiles.value_bits;
    s.stream_resident = (m.resident_forced >= 0 ? m.resident_forced != 0 : m.resident_eligible) && hisparse::dev::stream_policy_applies(tiles.format, tiles.light) ? 1u : 0u;
    return HS_OK;
}

// EXTENSION, opt-in (hs_set_option "autotune" = 1): the plan by MEASUREMENT.  The planner's model is within 10 % of the best plan that can be forced on 23 of 24
// + 9 of 12 out-of-sample matrices (tools/planner_check.py); what is left are close calls no statistic it has separates (a fixed-point one-slice plan that OWNER24
// would run 1.3 x faster next to others of the same shape it would slow down; hollywood: OWNER24 3-6 % ahead of the DELTA image the gap rule picks).  With the
// option set the load builds the planner's own image, times a few SpMVs of it on a zero vector (the step time does not depend on the values), does the same for
// every other element format the matrix can take, and keeps the fastest -- a caller that will run thousands of SpMVs of one matrix trades a few more loads
// (each tens of milliseconds) for it.  The reference's analogue is its design-space sweep (performance_model/design_space_exp.cpp:496-547), done there by a
// model because a bitstream cannot be rebuilt per matrix; an image can.
double time_loaded_plan(hs_context* ctx, int runs) {
    DeviceBuffer<uint32_t> zero_x;
    if (zero_x.alloc(size_t(ctx->mat.num_cols) * 4 + 64) != hipSuccess) { (void)hipGetLastError(); return -1.0; }
    double us = -1.0;
    if (hipMemsetAsync(zero_x.get(), 0, size_t(ctx->mat.num_cols) * 4, ctx->stream) == hipSuccess)
        (void)time_steps(ctx, zero_x.get(), ctx->mat.y.get(), /*warm=*/3, /*regions=*/2, runs, &us);
    (void)hipStreamSynchronize(ctx->stream);
    return us;
}

int load_matrix_impl(hs_context* ctx, const void* const* channel, const uint64_t* n_packets, const hisparse::dev::CsrView* csr,
                     uint32_t num_rows, uint32_t num_cols, uint32_t num_row_partitions, uint32_t num_col_partitions) {
    const char* tune = ctx_option(ctx, "HISPARSE_AUTOTUNE");
    const bool tuning = tune && std::atoi(tune) != 0 && !ctx_option(ctx, "HISPARSE_STREAM_FORMAT");      // (a forced format is the caller's decision)
    // (the value map, when asked for, is built by the load that is kept: the candidate loads of autotune go without)
    int rc = load_matrix_once(ctx, channel, n_packets, csr, num_rows, num_cols, num_row_partitions, num_col_partitions, !tuning);
    if (rc != HS_OK || !tuning) return rc;
    const bool debug = ctx_option(ctx, "HISPARSE_PLAN_DEBUG") != nullptr;
    const char* const names[] = {"pairs", "delta", "bitmap", "owner", "pairs24", "owner24", "sweep"};      // StreamFormat order (stream_tiles.h)
    const MatrixData& m = ctx->mat;
    const std::string own = m.launch.light ? "light" : names[m.launch.format < 7 ? m.launch.format : 0];
    const uint64_t nnz = ctx->stats.nnz;
    const int runs = int(std::max<uint64_t>(5, std::min<uint64_t>(50, (uint64_t(40) << 20) / std::max<uint64_t>(1, nnz))));      // ~ 1-3 ms of SpMVs per candidate
    double best_us = time_loaded_plan(ctx, runs);
    if (best_us <= 0.0)                                     // could not time: the planner's plan stands
        return value_map_asked(ctx) ? load_matrix_once(ctx, channel, n_packets, csr, num_rows, num_cols, num_row_partitions, num_col_partitions, true) : HS_OK;
    std::string best = own;
    if (debug) std::fprintf(stderr, "autotune: planner's plan %s x%u: %.2f us\n", own.c_str(), m.col_slices, best_us);
    const double own_us = best_us;
    const auto light_it = ctx->options.find("HISPARSE_LIGHT");      // the caller's own setting, put back at the end
    const bool had_light = light_it != ctx->options.end();
    const std::string caller_light = had_light ? light_it->second : std::string();
    auto restore = [&]() {
        ctx->options.erase("HISPARSE_STREAM_FORMAT");
        if (had_light) ctx->options["HISPARSE_LIGHT"] = caller_light; else ctx->options.erase("HISPARSE_LIGHT");
    };
    for (const char* fmt : {"delta", "pairs", "owner24", "sweep"}) {
        if (own == fmt) continue;
        ctx->options["HISPARSE_STREAM_FORMAT"] = fmt;
        ctx->options["HISPARSE_LIGHT"] = "0";
        const int rc2 = load_matrix_once(ctx, channel, n_packets, csr, num_rows, num_cols, num_row_partitions, num_col_partitions, false);
        double us = -1.0;
        if (rc2 == HS_OK && std::string(names[m.launch.format < 7 ? m.launch.format : 0]) == fmt) us = time_loaded_plan(ctx, runs);
        if (debug) std::fprintf(stderr, "autotune: %s x%u: %s\n", fmt, rc2 == HS_OK ? m.col_slices : 0u, us > 0.0 ? (std::to_string(us) + " us").c_str() : "not available");
        if (us > 0.0 && us < 0.97 * best_us) { best_us = us; best = fmt; }      // (3 %: below that it is the box's noise, and the planner's plan wins ties)
    }
    restore();
    if (best != own) {
        ctx->options["HISPARSE_STREAM_FORMAT"] = best;
        ctx->options["HISPARSE_LIGHT"] = "0";
    }
    rc = load_matrix_once(ctx, channel, n_packets, csr, num_rows, num_cols, num_row_partitions, num_col_partitions, true);      // the winner (or the planner's own plan again)
    restore();
    if (debug) std::fprintf(stderr, "autotune: kept %s (%.2f us against the planner's %.2f)\n", best.c_str(), best_us, own_us);
    return rc;
}

// EXTENSION: new values for the loaded CSR matrix, in place (hisparse_hip.h).  A carried combine pass is settled first, as at most other
// entry points: it reads only the partial vectors, never the image, so leaving it owed would be correct too, but settling keeps the rule
// "every entry point but hs_run settles" without an exception to reason about, for one combine launch of a few microseconds.
int update_values(hs_context* ctx, const float* values, uint64_t nnz, bool from_host) {
    if (int rc = enter(ctx, kMatrix | kHostOnly)) return rc;
    MatrixData& m = ctx->mat;
    if (!values) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    if (!m.value_map) return fail(ctx, HS_ERR_UNSUPPORTED, "no value map: " + m.value_map_why);
    if (nnz != m.value_map_nnz)
        return fail(ctx, HS_ERR_BAD_ARG, "nnz must equal the loaded CSR's indptr[num_rows] (" + std::to_string(m.value_map_nnz) + ")");
    if (!from_host && reinterpret_cast<uintptr_t>(values) % 4 != 0) return fail(ctx, HS_ERR_BAD_ARG, "values_dev must be 4-byte aligned");
    if (int rc = enter(ctx, 0)) return rc;
    if (nnz == 0) return HS_OK;
    const float* src = values;
    if (from_host) {
        if (!m.value_stage) HS_HIP(ctx, m.value_stage.alloc(size_t(nnz) * 4));
        // (stream order: the previous update's kernel has read the staging buffer before this copy writes it)
        HS_HIP(ctx, hipMemcpyAsync(m.value_stage.get(), values, size_t(nnz) * 4, hipMemcpyHostToDevice, ctx->stream));
        src = m.value_stage.get();
    }
    HS_HIP(ctx, hisparse::dev::launch_value_update(ctx->impl == HS_IMPL_FIXED, src, nnz, m.value_map.get(), reinterpret_cast<uint32_t*>(m.image.get()),
                                                   ctx->stats.stream_bytes / 4, m.mfma.value_map.get(), m.mfma.words.get(), m.mfma.value_map ? m.mfma.info.words_bytes / 4 : 0,
                                                   uint32_t(ctx->compute_units), ctx->stream));
    m.image_id = hisparse::next_image_id();      // the image was rewritten: cold to the device's reuse tracker, like a reload
    if (from_host) HS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the caller may reuse `values` immediately (as after hs_load_vector)
    return HS_OK;
}

// hs_load_matrix_csr and hs_load_matrix_csr_transposed: the arrays describe a num_rows x num_cols matrix A; the context gets A, or A^T
int load_csr(hs_context* ctx, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, const float* values, bool transposed,
             uint32_t* padded_rows, uint32_t* padded_cols) {
    if (!ctx || !indptr) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    const Geometry& g = ctx->geom;
    if (num_rows == 0 || num_cols == 0) return fail(ctx, HS_ERR_BAD_ARG, "empty matrix");
    hisparse::dev::CsrView view;
    view.num_rows = num_rows;
    view.num_cols = num_cols;
    view.indptr = indptr;
    view.indices = indices;
    view.values = values;
    view.transposed = transposed;
    // util_round_csr_matrix_dim (sw/data_formatter.h:15-29): rows up to a multiple of P*C*F, columns to a multiple of 8
    const uint64_t rows = (uint64_t(view.out_rows()) + g.row_divisor - 1) / g.row_divisor * g.row_divisor;
    const uint64_t cols = (uint64_t(view.out_cols()) + hisparse::PACK_SIZE - 1) / hisparse::PACK_SIZE * hisparse::PACK_SIZE;
    if (rows > 0xffffffffull || cols > 0xffffffffull) return fail(ctx, HS_ERR_BAD_ARG, "padded dimensions exceed 32 bits");
    const int rc = load_matrix_impl(ctx, nullptr, nullptr, &view, uint32_t(rows), uint32_t(cols), uint32_t((rows + g.logical_ob - 1) / g.logical_ob),
                                    uint32_t((cols + g.logical_vb - 1) / g.logical_vb));
    if (rc == HS_OK) {
        if (padded_rows) *padded_rows = uint32_t(rows);
        if (padded_cols) *padded_cols = uint32_t(cols);
    }
    return rc;
}

}  // namespace

extern "C" {

int hs_load_matrix(hs_context* ctx, const void* const channel[HS_NUM_CHANNELS], const uint64_t n_packets[HS_NUM_CHANNELS],
                   uint32_t num_rows, uint32_t num_cols, uint32_t num_row_partitions, uint32_t num_col_partitions) {
    if (!ctx || !channel || !n_packets) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    return load_matrix_impl(ctx, channel, n_packets, nullptr, num_rows, num_cols, num_row_partitions, num_col_partitions);
}

int hs_load_matrix_csr(hs_context* ctx, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, const float* values,
                       uint32_t* padded_rows, uint32_t* padded_cols) {
    return load_csr(ctx, num_rows, num_cols, indptr, indices, values, false, padded_rows, padded_cols);
}

int hs_load_matrix_csr_transposed(hs_context* ctx, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, const float* values,
                                  uint32_t* padded_rows, uint32_t* padded_cols) {
    return load_csr(ctx, num_rows, num_cols, indptr, indices, values, true, padded_rows, padded_cols);
}

int hs_update_values(hs_context* ctx, const float* values, uint64_t nnz) { return update_values(ctx, values, nnz, true); }
int hs_update_values_device(hs_context* ctx, const float* values_dev, uint64_t nnz) { return update_values(ctx, values_dev, nnz, false); }

int hs_debug_read_tiles(hs_context* ctx, void* image, uint64_t image_capacity, void* blocks, void* units) {
    if (int rc = enter(ctx, kMatrix | kHostOnly)) return rc;
    const hs_stats& s = ctx->stats;
    if (image && image_capacity < s.stream_bytes) return fail(ctx, HS_ERR_BAD_ARG, "image buffer too small");
    if (int rc = enter(ctx, kNoSettle)) return rc;
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (image && s.stream_bytes) HS_HIP(ctx, hipMemcpy(image, ctx->mat.image.get(), s.stream_bytes, hipMemcpyDeviceToHost));
    if (blocks && s.num_blocks) HS_HIP(ctx, hipMemcpy(blocks, ctx->mat.blocks.get(), size_t(s.num_blocks) * sizeof(Block), hipMemcpyDeviceToHost));
    if (units && s.num_units) HS_HIP(ctx, hipMemcpy(units, ctx->mat.units.get(), size_t(s.num_units) * sizeof(Unit), hipMemcpyDeviceToHost));
    return HS_OK;
}

int hs_debug_read_mfma_image(hs_context* ctx, void* words, uint64_t capacity, uint64_t* bytes) {
    if (int rc = enter(ctx, kMatrix | kHostOnly)) return rc;
    const uint64_t n = ctx->mat.mfma.words ? ctx->mat.mfma.info.words_bytes : 0;
    if (bytes) *bytes = n;
    if (!words || !n) return HS_OK;
    if (capacity < n) return fail(ctx, HS_ERR_BAD_ARG, "buffer too small");
    if (int rc = enter(ctx, kNoSettle)) return rc;
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    HS_HIP(ctx, hipMemcpy(words, ctx->mat.mfma.words.get(), n, hipMemcpyDeviceToHost));
    return HS_OK;
}

}  // extern "C"
