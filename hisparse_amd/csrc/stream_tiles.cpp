// stream_tiles.cpp — CPSR image -> row-block element streams (see stream_tiles.h for the format and the why).
//
// The decode follows the reference's loader in MEANING (header layout, per-lane lengths, marker = row
// advance, interleaved virtual channels):
//   spmv/libfpga/spmv_cluster.h:41-98        fixed point, INTERLEAVE_FACTOR 1
//   spmv-fp/libfpga/spmv_cluster.h:46-117    float, INTERLEAVE_FACTOR 1 or 8
// with the row <-> (channel, lane, round) mapping of sw/data_formatter.h:410,432 and the result drain
// order of spmv/spmv_result_drain.cpp:36,104-113 (net effect: natural row order in y).
#include "stream_tiles.h"
#include "tiles_common.h"
#include "gpu_tiles.h"
#include "stream_plan.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <numeric>
#include <string>
#include <thread>

namespace hisparse {
namespace dev {

namespace {

using namespace detail;

// One build of the element-stream image: what the passes below share.  The driver (build_stream_tiles_attempt) reads as the list of the
// passes; the decisions between them are the functions of stream_plan.h.
struct TileBuild {
    // the source and what the caller asked for
    const void* const* const channel;
    const uint64_t* const n_packets;
    const CsrView* const csr;
    const uint32_t max_workgroups;
    const uint64_t image_slack;
    const bool is_float;
    const PlanSwitches& sw;
    StreamTiles& out;
    std::string& error;
    Layout L;
    uint32_t num_rows, num_cols, CP, RP, S;
    PhaseTimer timer;
    std::unique_ptr<GpuTiler> gpu;       // the per-non-zero passes on the device (gpu_tiles.h) instead of the host walks; null: host path
    // what the passes hand on
    std::vector<uint32_t> row_nnz;
    TileCensus census;
    TilePlan plan;
    std::vector<RowRange> ranges;
    std::vector<uint64_t> range_nnz;
    std::vector<uint32_t> block_of_row;   // row -> row range
    size_t slots_per_range = 0;
    std::vector<uint32_t> cnt;            // (row range, sub-tile, source channel) counters, then offsets; released before the sort
    std::vector<uint32_t> unit_of;        // (row range, cp, s) -> unit index
    std::vector<UnitPlan> plans;
    std::vector<uint64_t> scratch;        // high word position, low word value: sorts by position (host path only)
    uint64_t scratch_elems = 0;
    std::vector<uint32_t> block_of_unit;
    std::vector<uint64_t> block_nnz;      // weight of a block for the workgroup assignment
    uint64_t image_bytes = 0;
    uint32_t record_bytes = kRecordBytes;   // DELTA: kRecordBytes24 once choose_value_bits has decided to pack
    uint64_t outlier_count = 0;             // packed DELTA: value words that do not fit the field at the chosen shift
    std::vector<std::vector<uint32_t>> mine;

    TileBuild(const void* const channel_[NUM_HBM_CHANNELS], const uint64_t n_packets_[NUM_HBM_CHANNELS], const Geometry& geom, uint32_t num_rows_,
              uint32_t num_cols_, uint32_t num_row_partitions, uint32_t num_col_partitions, uint32_t max_workgroups_, StreamTiles& out_,
              std::string& error_, uint64_t image_slack_, const CsrView* csr_, const PlanSwitches& sw_)
        : channel(channel_), n_packets(n_packets_), csr(csr_), max_workgroups(max_workgroups_), image_slack(image_slack_),
          is_float(geom.impl != IMPL_FIXED), sw(sw_), out(out_), error(error_), num_rows(num_rows_), num_cols(num_cols_), timer{sw_.debug} {
        L.g = &geom;
        L.num_rows = num_rows;
        L.num_cols = num_cols;
        L.row_parts = num_row_partitions;
        L.col_parts = num_col_partitions;
        L.F = geom.interleave;
        L.sub_width = uint32_t(std::min<uint64_t>(kSubTileCols, geom.logical_vb));
        L.subs_per_cp = uint32_t((geom.logical_vb + L.sub_width - 1) / L.sub_width);
        L.cross_parts = sw.cross_parts;
        CP = num_col_partitions, RP = num_row_partitions, S = L.subs_per_cp;
    }

    const MatPkt* chan(uint32_t pc) const { return static_cast<const MatPkt*>(channel[pc]); }
    size_t slot(uint32_t b, uint32_t cp, uint32_t s, uint32_t pc) const { return size_t(b) * slots_per_range + (size_t(cp) * S + s) * NUM_HBM_CHANNELS + pc; }
    size_t walk_tasks() const { return L.cross_parts ? size_t(CP) * NUM_HBM_CHANNELS : size_t(RP) * CP * NUM_HBM_CHANNELS; }      // host passes 1 and 2 (see count_units)
    PlanInputs plan_inputs() const { return PlanInputs{L, row_nnz, out.nnz, census, max_workgroups, is_float, sw}; }
    bool gpu_failed() { error = gpu->error(); return false; }
    void set_format(StreamFormat format) { plan.format = out.format = format; }
    uint32_t chunk_bytes() const { return plan.aux24() ? kChunkBytes24 : kChunkBytes; }
    uint32_t wave_stride() const { return chunk_bytes() * kConsumerWaves; }
    // one element slot of a chunk: value word + position word (32-bit: interleaved pairs; 24-bit: 64 values, then 64 x 3 bytes)
    static void put(bool aux24, uint8_t* chunk, uint32_t lane, uint32_t value, uint32_t where) {
        if (aux24) {
            reinterpret_cast<uint32_t*>(chunk)[lane] = value;
            uint8_t* a = chunk + kWaveLanes * 4 + lane * 3;
            a[0] = uint8_t(where); a[1] = uint8_t(where >> 8); a[2] = uint8_t(where >> 16);
        } else {
            reinterpret_cast<uint32_t*>(chunk)[2 * lane] = value;
            reinterpret_cast<uint32_t*>(chunk)[2 * lane + 1] = where;
        }
    }

    bool count_rows(void* gpu_stream, bool use_gpu);
    bool take_census();
    void cut_row_ranges();
    bool count_units();
    uint32_t block_flags(uint32_t b) const;
    bool enumerate_blocks();
    bool collect_and_sort();
    void fall_back_to_pairs();
    bool owner_shares(uint32_t max_span);
    bool lay_out_streams();
    bool choose_value_bits();
    void place_outliers(const std::vector<uint32_t>& unit, const std::vector<Outlier>& entry);
    void assign_to_workgroups();
    void finish_blocks();
    bool emit_on_gpu();
    void emit_owner();
    void emit_pairs();
    void emit_delta();
};

// `out` as pass 0 left it: the builders that take over (BITMAP refused, SWEEP) and the element-format passes start from empty tables
void reset_keeping_nnz(StreamTiles& out) {
    const uint64_t nnz_keep = out.nnz;      // (no device image to give back: the tiler keeps its buffers until a build succeeds)
    out = StreamTiles();
    out.nnz = nnz_keep;
}

// ---- pass 0: non-zeros per row (rows of different physical channels are disjoint) ------------
bool TileBuild::count_rows(void* gpu_stream, bool use_gpu) {
    row_nnz.assign(num_rows, 0);
    if (use_gpu) {
        if (csr) gpu.reset(new GpuTiler(L, *csr, static_cast<hipStream_t>(gpu_stream)));
        else gpu.reset(new GpuTiler(L, channel, n_packets, static_cast<hipStream_t>(gpu_stream)));
        if (!gpu->count_rows(row_nnz, out.nnz)) return gpu_failed();
    } else {
    std::vector<WalkResult> res0(size_t(RP) * NUM_HBM_CHANNELS);
    parallel_for(res0.size(), [&](size_t w) {
        const uint32_t rp = uint32_t(w / NUM_HBM_CHANNELS), pc = uint32_t(w % NUM_HBM_CHANNELS);
        for (uint32_t cp = 0; cp < CP && res0[w].ok; ++cp) {
            WalkResult r = walk_channel_partition(L, chan(pc), n_packets[pc], pc, rp, cp,
                                                  [&](uint32_t row, uint32_t, uint32_t) { row_nnz[row]++; });
            if (!r.ok) res0[w] = r; else res0[w].nnz += r.nnz;
        }
    });
    for (const auto& r : res0) {
        if (!r.ok) { error = r.error; return false; }
        out.nnz += r.nnz;
    }
    }
    timer.lap("pass 0 (row counts)");
    return true;
}

// ---- tile census (TileCensus, stream_plan.h): non-zeros per (fine row range of equal non-zero count, x sub-tile) -----------------------------
bool TileBuild::take_census() {
    census.tiles = CP * S;
    if (out.nnz && sw.census) {
        census.fine = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>({512, (uint64_t(4) << 20) / std::max<uint32_t>(1, census.tiles), num_rows})));
        std::vector<uint32_t> fine_of_row(num_rows);
        uint64_t seen = 0;
        for (uint32_t r = 0; r < num_rows; ++r) {
            fine_of_row[r] = uint32_t(std::min<uint64_t>(census.fine - 1, seen * census.fine / out.nnz));
            seen += row_nnz[r];
        }
        if (gpu) {
            if (!gpu->count_tiles(fine_of_row, census.fine, census.cnt)) { error = gpu->error(); return false; }
        } else {
            const size_t cells = size_t(census.fine) * census.tiles;
            std::unique_ptr<std::atomic<uint32_t>[]> cell(new std::atomic<uint32_t>[cells]);
            for (size_t i = 0; i < cells; ++i) cell[i].store(0, std::memory_order_relaxed);
            parallel_for(size_t(RP) * NUM_HBM_CHANNELS, [&](size_t w) {
                const uint32_t rp = uint32_t(w / NUM_HBM_CHANNELS), pc = uint32_t(w % NUM_HBM_CHANNELS);
                for (uint32_t cp = 0; cp < CP; ++cp)
                    walk_channel_partition(L, chan(pc), n_packets[pc], pc, rp, cp, [&](uint32_t row, uint32_t col, uint32_t) {
                        cell[size_t(fine_of_row[row]) * census.tiles + size_t(cp) * S + col / L.sub_width].fetch_add(1, std::memory_order_relaxed);
                    });
            });
            census.cnt.resize(cells);
            for (size_t i = 0; i < cells; ++i) census.cnt[i] = cell[i].load(std::memory_order_relaxed);
        }
        // (over the sub-tiles that exist: the last column partition's table ends where the matrix does)
        size_t live = 0, existing = 0;
        for (uint32_t cp = 0; cp < CP; ++cp)
            for (uint32_t sub = 0; sub < S; ++sub) existing += uint64_t(sub) * L.sub_width < L.cols_in_part(cp);
        existing *= census.fine;
        for (uint32_t c : census.cnt) live += c != 0;
        census.populated = existing ? std::min(1.0, std::max(1.0 / double(existing), double(live) / double(existing))) : 1.0;
        if (sw.debug)
            std::fprintf(stderr, "census: %u fine row ranges x %u sub-tiles, %.1f %% of the cells hold anything\n", census.fine, census.tiles, census.populated * 100.0);
    }
    timer.lap("tile census");
    return true;
}

// ---- row ranges: equal non-zero count, <= max_rows rows, never across a row partition; the x ring depth that fits beside them --------
void TileBuild::cut_row_ranges() {
    const uint32_t G = plan.G, slices = plan.slices, max_rows = plan.max_rows;
    const bool light = plan.light;
    // as many ranges as workgroup slots (G / slices), or the next multiple of that when the LDS row cap forces more, so that
    // every workgroup ends up with the same number of blocks
    const uint64_t per_round = std::max<uint32_t>(1, G / slices);
    const uint64_t rounds = std::max<uint64_t>(1, ((uint64_t(num_rows) + max_rows - 1) / max_rows + per_round - 1) / per_round);
    const uint64_t want_ranges = std::max<uint64_t>(1, std::min<uint64_t>(per_round * rounds, out.nnz / (light ? kLightMinBlockNnz : 4096u)));
    build_row_ranges_at_most(L, row_nnz, out.nnz, want_ranges, max_rows, ranges, range_nnz, out.nnz / 4096 >= per_round * rounds ? per_round : 0);
    const uint32_t NR = uint32_t(ranges.size());
    block_of_row.resize(num_rows);
    for (uint32_t b = 0; b < NR; ++b) {
        std::fill(block_of_row.begin() + ranges[b].row0, block_of_row.begin() + ranges[b].row0 + ranges[b].nrows, b);
        out.max_block_rows = std::max(out.max_block_rows, ranges[b].nrows);
    }
    const uint32_t ring_fit = (kMaxLdsBytes - (((out.max_block_rows + plan.spare_rows()) * plan.acc_bytes() + 15u) & ~15u)) / (kSubTileCols * 4u);
    out.ring_buffers = std::max(kMinXBuffers, std::min(kMaxXBuffers, ring_fit));
    timer.lap("plan + row ranges");
}

// ---- pass 1: elements per (row range, column partition, sub-tile, source channel) -------------------
bool TileBuild::count_units() {
    const uint32_t NR = uint32_t(ranges.size());
    slots_per_range = size_t(CP) * S * NUM_HBM_CHANNELS;
    // (row range, sub-tile, source channel) counters: rows x columns / (rows per block x 8192) x 16 words -- a matrix of 10^8 x 10^8
    // would ask for gigabytes here and for as many Unit descriptors: refuse instead of swapping
    if (uint64_t(NR) * slots_per_range > (uint64_t(1) << 28)) {
        error = "matrix too large for this build: " + std::to_string(NR) + " row ranges x " + std::to_string(uint64_t(CP) * S) + " x sub-tiles exceed the unit table";
        return false;
    }
    cnt.assign(size_t(NR) * slots_per_range, 0);
    std::vector<WalkResult> res1(size_t(RP) * CP * NUM_HBM_CHANNELS);
    if (gpu) {      // totals per (range, sub-tile); the per-source-channel split only serves the host's scatter
        std::vector<uint32_t> totals;
        if (!gpu->count_tiles(block_of_row, NR, totals)) { error = gpu->error(); return false; }
        for (uint32_t b = 0; b < NR; ++b)
            for (uint32_t cp = 0; cp < CP; ++cp)
                for (uint32_t sub = 0; sub < S; ++sub) cnt[slot(b, cp, sub, 0)] = totals[(size_t(b) * CP + cp) * S + sub];
    } else {
    // (row ranges that cross partition borders: the counters of a (range, sub-tile, channel) are fed from two row partitions, so one task
    //  takes ALL row partitions of its (column partition, channel), one after the other)
    parallel_for(walk_tasks(), [&](size_t w) {
        const uint32_t pc = uint32_t(w % NUM_HBM_CHANNELS), cp = uint32_t((w / NUM_HBM_CHANNELS) % CP);
        for (uint32_t rp = L.cross_parts ? 0u : uint32_t(w / NUM_HBM_CHANNELS / CP), rp_end = L.cross_parts ? RP : rp + 1; rp < rp_end; ++rp)
            res1[(size_t(rp) * CP + cp) * NUM_HBM_CHANNELS + pc] = walk_channel_partition(L, chan(pc), n_packets[pc], pc, rp, cp, [&](uint32_t row, uint32_t col, uint32_t) {
                cnt[slot(block_of_row[row], cp, col / L.sub_width, pc)]++;
            });
    });
    for (const auto& r : res1)
        if (!r.ok) { error = r.error; return false; }
    }
    timer.lap("pass 1 (unit counts)");
    return true;
}

// The flags of the blocks of row range b under the plan's format
uint32_t TileBuild::block_flags(uint32_t b) const {
    if (plan.delta()) {   // long rows: position gaps well inside a row (HISPARSE_ROW_RUNS=0|1 forces, for the tests)
        // (over the rows that HAVE non-zeros: the padding rows at the end of a float_stall matrix would make the last block look sparse)
        uint32_t live_rows = 0, heaviest = 0;
        for (uint32_t r = 0; r < ranges[b].nrows; ++r) {
            live_rows += row_nnz[ranges[b].row0 + r] != 0;
            heaviest = std::max(heaviest, row_nnz[ranges[b].row0 + r]);
        }
        const double gap = range_nnz[b] ? double(live_rows) * double(num_cols) / double(range_nnz[b]) : 1e30;
        // (a hub row: an eighth of the block in one row -- eight lanes of every step, more in the hub's own sub-tiles, would add to ONE accumulator; see hub_share, stream_plan.h)
        const bool hub_block = heaviest >= 4096 && uint64_t(heaviest) * 8 >= range_nnz[b];
        return (sw.row_runs.set ? sw.row_runs.value != 0 : (gap < kDenseMeanGap || hub_block)) ? kBlockDenseRows : 0u;
    }
    if (plan.owner()) return 0;
    if (plan.light) return 0;                    // strided dealing for every block: a lane of the light kernel walks consecutive sorted elements
    return pairs_block_is_dense(ranges[b], range_nnz[b]) ? kBlockDenseRows : 0u;
}

// ---- enumerate blocks (row range x column slice) and their units; counts -> offsets into a scratch element list ----
bool TileBuild::enumerate_blocks() {
    const uint32_t NR = uint32_t(ranges.size()), slices = plan.slices;
    const Geometry& geom = *L.g;
    unit_of.assign(size_t(NR) * CP * S, 0xffffffffu);
    const uint32_t sub_tiles = CP * S;
    std::vector<uint64_t> tile_nnz(sub_tiles);
    std::vector<uint32_t> slice_of(sub_tiles), by_weight(sub_tiles);
    for (uint32_t b = 0; b < NR; ++b) {
        // Column slices of this row range: its sub-tiles are dealt to the slices heaviest first, each to the lightest slice
        // so far.  (Round-robin by index left the slices of a power-law graph 7 % apart -- the columns of sub-tile 0 are
        // the popular ones in EVERY row range -- and with one block per workgroup the slowest block is the kernel time.)
        for (uint32_t k = 0; k < sub_tiles; ++k) {
            tile_nnz[k] = 0;
            for (uint32_t pc = 0; pc < NUM_HBM_CHANNELS; ++pc) tile_nnz[k] += cnt[slot(b, k / S, k % S, pc)];
        }
        uint64_t slice_load[kMaxForcedColSlices] = {0};
        uint32_t slice_tiles[kMaxForcedColSlices] = {0};
        deal_tiles_to_slices(tile_nnz, slices, by_weight, slice_load, slice_tiles, slice_of.data());
        const uint32_t flags = block_flags(b);
        for (uint32_t slice = 0; slice < slices; ++slice) {   // device block index (before finish_blocks) = b * slices + slice
            Block blk{};
            blk.row0 = ranges[b].row0;
            blk.nrows = ranges[b].nrows;
            blk.row_part = ranges[b].row_part;
            blk.last_part = ranges[b].last_part;
            blk.flags = flags;
            blk.out_offset = slices > 1 ? slice * num_rows + ranges[b].row0 : ranges[b].row0;
            blk.unit_begin = uint32_t(out.units.size());
            for (uint32_t k = 0; k < sub_tiles; ++k) {
                if (slice_of[k] != slice) continue;
                const uint32_t cp = k / S, s = k % S;
                uint64_t n = 0;
                for (uint32_t pc = 0; pc < NUM_HBM_CHANNELS; ++pc) {   // counts -> exclusive offsets inside the unit
                    const uint32_t c = cnt[slot(b, cp, s, pc)];
                    cnt[slot(b, cp, s, pc)] = uint32_t(n);
                    n += c;
                }
                if (n == 0) continue;
                if (n > 0x7fffffffull) { error = "unit too large"; return false; }
                UnitPlan up;
                up.n = uint32_t(n);
                up.scratch = scratch_elems;
                scratch_elems += n;
                Unit u{};
                u.col0 = uint32_t(uint64_t(cp) * geom.logical_vb + uint64_t(s) * L.sub_width);
                u.ncols = std::min<uint32_t>(L.sub_width, L.cols_in_part(cp) - s * L.sub_width);
                unit_of[(size_t(b) * CP + cp) * S + s] = uint32_t(out.units.size());
                out.units.push_back(u);
                plans.push_back(up);
            }
            blk.unit_end = uint32_t(out.units.size());
            out.blocks.push_back(blk);
        }
    }
    block_of_unit.resize(out.units.size());
    for (uint32_t bi = 0; bi < out.blocks.size(); ++bi)
        for (uint32_t u = out.blocks[bi].unit_begin; u < out.blocks[bi].unit_end; ++u) block_of_unit[u] = bi;
    timer.lap("enumerate blocks + units");
    return true;
}

// ---- pass 2: collect every unit's elements as (position, value), position = local_row * 8192 + local_col; sort them by position -------
//      (cnt is released before the sort; the device path never allocates scratch)
bool TileBuild::collect_and_sort() {
    const uint32_t NR = uint32_t(ranges.size()), NU = uint32_t(out.units.size());
    const bool delta = plan.delta();
    if (gpu) {
        std::vector<uint32_t> range_row0(NR);
        for (uint32_t b = 0; b < NR; ++b) range_row0[b] = ranges[b].row0;
        bool duplicates = false;
        if (!gpu->sort_elements(block_of_row, range_row0, unit_of, plans, duplicates)) { error = gpu->error(); return false; }
        if (duplicates) { error = "gpu re-tile: duplicate entries"; return false; }      // the caller rebuilds on the host
        std::vector<uint32_t>().swap(cnt);
        timer.lap("gpu: keys + radix sort");
        if (delta) {
            if (!gpu->delta_slots(plans)) { error = gpu->error(); return false; }
        } else {
            for (UnitPlan& up : plans) up.slots = up.n;
        }
        return true;
    }
    scratch.resize(scratch_elems);
    parallel_for(walk_tasks(), [&](size_t w) {
        const uint32_t pc = uint32_t(w % NUM_HBM_CHANNELS), cp = uint32_t((w / NUM_HBM_CHANNELS) % CP);
        for (uint32_t rp = L.cross_parts ? 0u : uint32_t(w / NUM_HBM_CHANNELS / CP), rp_end = L.cross_parts ? RP : rp + 1; rp < rp_end; ++rp)
            walk_channel_partition(L, chan(pc), n_packets[pc], pc, rp, cp, [&](uint32_t row, uint32_t col, uint32_t val) {
                const uint32_t b = block_of_row[row], s = col / L.sub_width;
                const UnitPlan& up = plans[unit_of[(size_t(b) * CP + cp) * S + s]];
                const uint32_t pos = (row - ranges[b].row0) * kSubTileCols + (col - s * L.sub_width);
                scratch[up.scratch + cnt[slot(b, cp, s, pc)]++] = (uint64_t(pos) << 32) | val;
            });
    });
    std::vector<uint32_t>().swap(cnt);

    timer.lap("pass 2 (scatter)");
    // ---- per unit: sort by position; DELTA: count slots (elements + bridges for gaps that do not fit 16 bits) -------
    parallel_for(NU, [&](size_t u) {
        UnitPlan& up = plans[u];
        uint64_t* e = scratch.data() + up.scratch;
        std::sort(e, e + up.n);
        uint64_t slots = up.n;
        for (uint32_t i = 1; delta && i < up.n; ++i) {
            const uint64_t d = (e[i] >> 32) - (e[i - 1] >> 32);
            if (d > kMaxGap) slots += (d - kMaxGap + kBridgeAdvance - 1) / kBridgeAdvance;
        }
        up.slots = slots;
    });
    return true;
}

// DELTA -> PAIRS after the sort (stream_plan.h: delta_or_pairs)
void TileBuild::fall_back_to_pairs() {
    set_format(kFormatPairs);
    for (UnitPlan& up : plans) up.slots = up.n;
    for (uint32_t bi = 0; bi < out.blocks.size(); ++bi) {
        const uint32_t b = bi / plan.slices;     // blocks were pushed range by range, slice by slice
        out.blocks[bi].flags = pairs_block_is_dense(ranges[b], range_nnz[b]) ? kBlockDenseRows : 0u;
    }
}

// ---- OWNER: every unit's elements, sorted by (row, column), are cut into the 14 wavefronts' shares (balanced_owner_shares) -----
bool TileBuild::owner_shares(uint32_t max_span) {
    if (gpu) {
        if (!gpu->owner_shares(plans, max_span)) return gpu_failed();
        return true;
    }
    parallel_for(out.units.size(), [&](size_t u) {
        UnitPlan& up = plans[u];
        const uint64_t* e = scratch.data() + up.scratch;
        auto row_of = [&](uint32_t i) { return uint32_t(e[i] >> (32 + kOwnerColBits)); };
        balanced_owner_shares(up.n, row_of, up.own_begin, max_span);
        for (uint32_t w = 0; w < kConsumerWaves; ++w) {
            const bool any = up.own_begin[w + 1] > up.own_begin[w];
            up.own_row[w] = any ? row_of(up.own_begin[w]) : 0u;
            up.own_last[w] = any ? row_of(up.own_begin[w + 1] - 1) : 0u;
        }
    });
    return true;
}

// ---- per block: deal every unit's 64-slot chunks to the consumer wavefronts round-robin; lay out the streams -------
bool TileBuild::lay_out_streams() {
    const bool delta = plan.delta(), owner = plan.owner(), owner24 = plan.owner24();
    const uint32_t NB = uint32_t(out.blocks.size()), chunk_bytes = this->chunk_bytes(), wave_stride = this->wave_stride();
    // DELTA runs are dealt lane-major ("spread"; HISPARSE_DELTA_DEAL=wave: rounds 1-4's dealing, kept for the A/B): see first_slot below
    const bool delta_spread = sw.delta_spread;
    block_nnz.assign(NB, 0);
    image_bytes = 0;
    out.elements = 0;
    for (uint32_t bi = 0; bi < NB; ++bi) {
        Block& blk = out.blocks[bi];
        uint32_t pos[kConsumerWaves] = {0};   // chunk / record position of every wavefront in its stream
        uint32_t chunk_counter = 0;
        for (uint32_t u = blk.unit_begin; u < blk.unit_end; ++u) {
            UnitPlan& up = plans[u];
            if (up.slots > 0x7fffffffull) { error = "unit too large"; return false; }
            if (owner) {
                // the unit's elements are sorted by (row, column): wavefront w's share is the contiguous stretch of its rows;
                // steps = its 64-slot chunks; lane l takes elements [l * steps, (l + 1) * steps) of the share
                for (uint32_t w = 0; w < kConsumerWaves; ++w) {
                    const uint32_t steps = (up.own_begin[w + 1] - up.own_begin[w] + kWaveLanes - 1) / kWaveLanes;
                    up.run_len[w] = steps;
                    up.start_step[w] = up.start_record[w] = pos[w];
                    pos[w] += steps;
                    // OWNER24: the share's first row rides in the high half (stream_tiles.h)
                    out.units[u].end_step[w] = owner24 ? (pos[w] | up.own_row[w] << 16) : pos[w];
                    out.elements += uint64_t(steps) * kWaveLanes;
                }
                continue;
            }
            const uint32_t chunks = uint32_t((up.slots + kWaveLanes - 1) / kWaveLanes);
            uint32_t run[kConsumerWaves] = {0};
            for (uint32_t c = 0; c < chunks; ++c) run[(chunk_counter + c) % kConsumerWaves]++;
            up.chunks = chunks;
            up.base = chunk_counter;
            chunk_counter += chunks;
            uint64_t first = 0;
            for (uint32_t w = 0; w < kConsumerWaves; ++w) {
                up.run_len[w] = run[w];
                // DELTA: which run of the position-sorted unit lane l of wavefront w walks.  "spread": runs are dealt lane-major (run
                // l * 14 + w), so the 64 lanes of a wavefront sit a 64th of the unit apart, like PAIRS' chunks.  "wave" (rounds 1-4): the
                // wavefront owns a contiguous 1/14 of the unit, its lanes consecutive runs of it -- then a hub row of a heavy-tailed
                // graph (R-MAT: 850 of a unit's 10 K elements in ONE row) holds ALL 64 lanes of a wavefront on one accumulator, step after
                // step: 64 ds_add_u64 on one address.  Measured (profiles/r05_delta_dealing.txt, whole step): R-MAT ogbl-ppa 85.1 -> 58.9 us
                // (PAIRS: 59.4-59.8), transformer-80 10.9 -> 9.9-10.2, mouse_gene 34.2 -> 33.9, gplus 20.1 -> 19.9, ogbl-ppa / hollywood equal.
                up.first_slot[w] = delta_spread ? first / kWaveLanes : first;
                up.lane_stride[w] = delta_spread ? chunks : run[w];
                first += uint64_t(run[w]) * kWaveLanes;
                up.start_step[w] = up.start_record[w] = pos[w];
                // DELTA: one head record (absolute positions) in front of the wavefront's records of this unit
                pos[w] += delta ? (run[w] ? (run[w] + 2) / 2 : 0) : run[w];      // DELTA: records of two slots, the head is the first slot
                out.units[u].end_step[w] = pos[w];
            }
            out.elements += uint64_t(chunks) * kWaveLanes;
        }
        for (uint32_t w = 0; w < kConsumerWaves; ++w) block_nnz[bi] += pos[w];   // the block's weight: wavefront steps, heads included
        // the kernel addresses a wavefront's stream with a 32-bit byte offset from Block::wave_offset
        for (uint32_t w = 0; w < kConsumerWaves; ++w)
            if (uint64_t(pos[w]) * (delta ? record_bytes : owner ? chunk_bytes : wave_stride) >= (1ull << 32)) { error = "row block stream exceeds 4 GiB"; return false; }
        if (delta || owner) {      // every wavefront's steps are contiguous
            for (uint32_t w = 0; w < kConsumerWaves; ++w) {
                blk.wave_offset[w] = image_bytes;
                // OWNER24: whole records of four steps (the steps behind the last one are never consumed)
                image_bytes += owner24 ? uint64_t((pos[w] + kOwnerRecordSteps - 1) / kOwnerRecordSteps) * kOwnerRecordBytes
                                       : uint64_t(pos[w]) * (delta ? record_bytes : chunk_bytes);
            }
        } else {
            // chunks are stored in dealing order (global chunk g of the block at g * 512 bytes; wavefront w consumes
            // g = w, w + 14, w + 28, ...): the 14 wavefronts of a workgroup sweep ONE contiguous region together
            for (uint32_t w = 0; w < kConsumerWaves; ++w) blk.wave_offset[w] = image_bytes + uint64_t(w) * chunk_bytes;
            image_bytes += uint64_t(chunk_counter) * chunk_bytes;
        }
    }
    return true;
}

// ---- DELTA: 24-bit value fields or plain 32-bit words (stream_tiles.h: kRecordBytes24)?  Called with the plain layout done; lays the streams out again
//      when it packs.  The shift and the misfit count depend on the value words alone, so both builders agree before a byte is emitted. ----
bool TileBuild::choose_value_bits() {
    out.value_bits = 32;
    out.value_shift = 0;
    if (is_float || sw.delta_bits == DeltaValueBits::kPlain || (csr && (csr->value_map || csr->plain_values))) return true;
    uint64_t misfits[kMaxValueShift + 1] = {0};
    if (gpu) {
        if (!gpu->count_value_misfits(misfits)) return gpu_failed();
    } else {
        std::vector<std::array<uint64_t, kMaxValueShift + 1>> part(out.units.size());
        parallel_for(out.units.size(), [&](size_t u) {
            part[u].fill(0);
            const uint64_t* e = scratch.data() + plans[u].scratch;
            for (uint32_t i = 0; i < plans[u].n; ++i)
                for (uint32_t sh = 0; sh <= kMaxValueShift; ++sh) part[u][sh] += !value_fits24(uint32_t(e[i]), sh);
        });
        for (const auto& p : part)
            for (uint32_t sh = 0; sh <= kMaxValueShift; ++sh) misfits[sh] += p[sh];
    }
    uint32_t shift = 0;
    for (uint32_t sh = 1; sh <= kMaxValueShift; ++sh)
        if (misfits[sh] < misfits[shift]) shift = sh;      // the fewest misfits; the smaller shift on a tie
    const uint64_t plain_bytes = image_bytes, outliers = misfits[shift];
    const uint64_t packed_bytes = plain_bytes / kRecordBytes * kRecordBytes24 + ((outliers * sizeof(Outlier) + 15u) & ~uint64_t(15));
    const bool within_cap = outliers * kDelta24OutlierShare <= out.elements;
    const bool wanted = sw.delta_bits == DeltaValueBits::kPacked || plain_bytes >= packed_bytes + kDelta24MinSavedBytes;
    if (sw.debug)
        std::fprintf(stderr, "delta value bits: shift %u leaves %llu outliers among %llu element slots, %llu -> %llu bytes: %s\n", shift, (unsigned long long)outliers,
                     (unsigned long long)out.elements, (unsigned long long)plain_bytes, (unsigned long long)packed_bytes, within_cap && wanted ? "packed" : "plain");
    if (!within_cap || !wanted) return true;
    out.value_bits = 24;
    out.value_shift = shift;
    outlier_count = outliers;
    record_bytes = kRecordBytes24;
    if (!lay_out_streams()) return false;
    image_bytes += (outliers * sizeof(Outlier) + 15u) & ~uint64_t(15);      // the outlier lists, behind the records
    for (Block& blk : out.blocks) { blk.value_shift = shift; blk.value_bits = 24; }
    return true;
}

// The outlier lists of a packed DELTA image: entry[k] belongs to unit unit[k]; the entries arrive in the order of the units and, inside a unit, of the
// positions.  Blocks own contiguous unit ranges in block order, so the entries of one block are contiguous: its list is that stretch.
void TileBuild::place_outliers(const std::vector<uint32_t>& unit, const std::vector<Outlier>& entry) {
    const uint64_t lists = image_bytes - ((outlier_count * sizeof(Outlier) + 15u) & ~uint64_t(15));
    for (size_t k = 0; k < entry.size(); ++k) {
        Block& blk = out.blocks[block_of_unit[unit[k]]];
        if (!blk.outlier_count) {
            const uint64_t at = lists + k * sizeof(Outlier);
            blk.outlier_lo = uint32_t(at);
            blk.outlier_hi = uint32_t(at >> 32);
        }
        blk.outlier_count++;
    }
    out.outliers = entry.size();
}

// ---- workgroups: longest-processing-time assignment of blocks (tiles_common.h) ------------------------------
void TileBuild::assign_to_workgroups() {
    const uint32_t NB = uint32_t(out.blocks.size()), G = plan.G, slices = plan.slices;
    // Blocks to XCDs by column slice (tiles_common.h: assign_workgroups_by_slice) -- OPT-IN (HISPARSE_XCD_AFFINITY=1).  Built in round 3
    // for matrices whose x outgrows an XCD's L2 (ogbn-products: 9.8 MB of x, 5 slices; ~20 % of the x refills miss L2) and measured:
    // same kernel time (203.6 vs 205.5 us, same box) and, by the counters, the SAME traffic (1084.7 vs 1087.5 MB of reads per launch:
    // 208 MB of it x either way) -- the refills are evicted by the matrix stream passing through the same L2, not by the other
    // slices' x.  Kept for experiments; the default stays the spread assignment.
    if (sw.xcd_affinity && slices > 1 && G % 8 == 0 && NB >= G) {
        std::vector<uint32_t> slice_of_block(NB);
        for (uint32_t bi = 0; bi < NB; ++bi) slice_of_block[bi] = bi % slices;      // blocks were pushed range by range, slice by slice
        assign_workgroups_by_slice(out, block_nnz, G, RP, slice_of_block, mine);
    } else {
        assign_workgroups(out, block_nnz, G, RP, mine);
    }
    timer.lap("stream layout + workgroups");
}

// Final block order (chain_blocks) after the copies of unit data the kernel wants inside the Block have been filled in.
void TileBuild::finish_blocks() {
    const bool owner24 = plan.owner24();
    for (Block& blk : out.blocks) {
        if (blk.unit_end > blk.unit_begin) {
            for (uint32_t w = 0; w < kConsumerWaves; ++w) {
                blk.total_steps[w] = out.units[blk.unit_end - 1].end_step[w] & (owner24 ? kOwnerStepMask : 0xffffffffu);
                blk.first_end[w] = out.units[blk.unit_begin].end_step[w];      // OWNER24: with the first share's row_base
            }
            blk.first_col0 = out.units[blk.unit_begin].col0;
            blk.first_ncols = out.units[blk.unit_begin].ncols;
        }
    }
    chain_blocks(out, mine, RP);
}

bool TileBuild::emit_on_gpu() {
    std::vector<uint32_t> outlier_unit;
    std::vector<Outlier> outlier_entry;
    if (!gpu->emit(out.format, image_bytes, image_slack, plans, block_of_unit, out.blocks, is_float, out.value_bits, out.value_shift, outlier_count, out.units, outlier_unit,
                   outlier_entry))
        return gpu_failed();
    if (out.value_bits == 24) place_outliers(outlier_unit, outlier_entry);
    out.d_image = gpu->release_image();
    out.d_value_map = gpu->release_value_map();
    out.image_bytes = image_bytes;
    finish_blocks();
    timer.lap("gpu: emit");
    return true;
}

// ---- OWNER: per (unit, wavefront) share: slot (step s, lane l) holds element l * steps + s of the share; the position word
//      IS the element's (local_row << 13 | local_col); padding aims a zero at the wavefront's own spare accumulator.
//      OWNER24: step S of the wavefront's stream = slot S % 4 of record S / 4, rows relative to the share's first row -------
void TileBuild::emit_owner() {
    uint8_t* image = out.image.data();
    const bool owner24 = plan.owner24();
    const uint32_t chunk_bytes = kChunkBytes;      // (OWNER is never PAIRS24)
    parallel_for(out.units.size(), [&](size_t u) {
        const UnitPlan& up = plans[u];
        const Block& blk = out.blocks[block_of_unit[u]];
        const uint64_t* e = scratch.data() + up.scratch;
        for (uint32_t w = 0; w < kConsumerWaves; ++w) {
            const uint32_t steps = up.run_len[w], n = up.own_begin[w + 1] - up.own_begin[w];
            const uint64_t* mine = e + up.own_begin[w];
            uint8_t* stream = image + blk.wave_offset[w];
            for (uint32_t st = 0; st < steps; ++st) {
                const uint32_t S = up.start_step[w] + st;
                for (uint32_t l = 0; l < kWaveLanes; ++l) {
                    const uint64_t i = uint64_t(l) * steps + st;
                    const uint32_t value = i < n ? uint32_t(mine[i]) : 0u, pos = i < n ? uint32_t(mine[i] >> 32) : 0u;
                    if (owner24) {
                        uint8_t* rec = stream + uint64_t(S / kOwnerRecordSteps) * kOwnerRecordBytes;
                        const uint32_t j = S % kOwnerRecordSteps;
                        const uint32_t where = i < n ? pos - (up.own_row[w] << kOwnerColBits) : kOwnerSpareField << kOwnerColBits;
                        reinterpret_cast<uint32_t*>(rec)[l * kOwnerRecordSteps + j] = value;
                        uint8_t* a = rec + kOwnerRecordValueBytes + (l * kOwnerRecordSteps + j) * 3;
                        a[0] = uint8_t(where); a[1] = uint8_t(where >> 8); a[2] = uint8_t(where >> 16);
                    } else {
                        put(false, stream + uint64_t(S) * chunk_bytes, l, value, i < n ? pos : (blk.nrows + w) << kOwnerColBits);
                    }
                }
            }
        }
    });
    finish_blocks();
    timer.lap("emit OWNER");
}

// ---- PAIRS: normal units: slot (chunk c, lane l) holds sorted element l * chunks + c (neighbouring lanes far
//      apart in the unit); dense-row units: element i sits in chunk i / 64, lane i % 64 ------------------------------
void TileBuild::emit_pairs() {
    uint8_t* image = out.image.data();
    const bool aux24 = plan.aux24();
    const uint32_t wave_stride = this->wave_stride();
    parallel_for(out.units.size(), [&](size_t u) {
        const UnitPlan& up = plans[u];
        const Block& blk = out.blocks[block_of_unit[u]];
        const bool dense = blk.flags & kBlockDenseRows;
        const uint64_t* e = scratch.data() + up.scratch;
        const uint64_t total = uint64_t(up.chunks) * kWaveLanes;
        for (uint64_t i = 0; i < total; ++i) {
            const uint32_t lane = dense ? uint32_t(i % kWaveLanes) : uint32_t(i / up.chunks);
            const uint32_t c = dense ? uint32_t(i / kWaveLanes) : uint32_t(i % up.chunks);
            const uint32_t g = up.base + c, w = g % kConsumerWaves;
            const uint32_t first = up.base + (w + kConsumerWaves - up.base % kConsumerWaves) % kConsumerWaves;  // first chunk of wave w in this unit
            const uint32_t step = up.start_step[w] + (g - first) / kConsumerWaves;
            uint8_t* chunk = image + blk.wave_offset[w] + uint64_t(step) * wave_stride;
            const uint32_t row_shift = aux24 ? kOwnerColBits : 16u;
            if (i < up.n) {
                const uint32_t pos = uint32_t(e[i] >> 32);
                put(aux24, chunk, lane, uint32_t(e[i]), ((pos / kSubTileCols) << row_shift) | (pos % kSubTileCols));
            } else {            // padding: zero value aimed at the block's scratch row
                put(aux24, chunk, lane, 0u, blk.nrows << row_shift);
            }
        }
    });
    finish_blocks();
    timer.lap("emit PAIRS");
}

// ---- DELTA: lane l of wavefront w owns run_len[w] consecutive slots of the sorted unit --------------------------------
void TileBuild::emit_delta() {
    uint8_t* image = out.image.data();
    const bool packed = out.value_bits == 24;
    const uint32_t shift = out.value_shift;
    std::vector<std::vector<Outlier>> unit_outliers(packed ? out.units.size() : 0);
    parallel_for(out.units.size(), [&](size_t u) {
        const UnitPlan& up = plans[u];
        const Block& blk = out.blocks[block_of_unit[u]];
        const uint64_t* e = scratch.data() + up.scratch;
        // expand to the slot sequence: gap (16 bit, 0xffff = bridge: advance 65535, no element), value, position after the slot
        std::vector<uint16_t> gap(up.slots);
        std::vector<uint32_t> val(up.slots), after(up.slots);
        uint64_t k = 0;
        uint32_t at = uint32_t(e[0] >> 32);
        for (uint32_t i = 0; i < up.n; ++i) {
            uint64_t d = (e[i] >> 32) - at;
            while (d > kMaxGap) { at += kBridgeAdvance; d -= kBridgeAdvance; gap[k] = kBridgeGap; val[k] = 0; after[k] = at; ++k; }
            at += uint32_t(d);
            gap[k] = uint16_t(d); val[k] = uint32_t(e[i]); after[k] = at; ++k;
            if (packed && !value_fits24(val[k - 1], shift)) {      // an outlier: its slot carries 0, the full word goes to the block's list
                unit_outliers[u].push_back(Outlier{at / kSubTileCols, out.units[u].col0 + at % kSubTileCols, val[k - 1]});
                val[k - 1] = 0;
            }
        }
        const uint16_t pad_gap = is_float ? kBridgeGap : 0;
        const uint32_t scratch_pos = blk.nrows * kSubTileCols;   // local row nrows = the scratch accumulator
        for (uint32_t w = 0; w < kConsumerWaves; ++w) {
            if (!up.run_len[w]) continue;
            uint8_t* rec = image + blk.wave_offset[w] + uint64_t(up.start_record[w]) * record_bytes;
            const uint32_t slots_in_records = (up.run_len[w] + 2) / 2 * 2;      // head + run, rounded up to whole records
            if (packed) {
                // slot q sits in record q / 2: the lane's 8 bytes at lane * 8 hold field A (bits 0-23), field B (24-47) and gap A (48-63), gap B lies at 512 + lane * 2
                auto put_slot = [&](uint32_t q, uint32_t l, uint32_t field, uint32_t gap16) {
                    uint8_t* r = rec + uint64_t(q / 2) * kRecordBytes24;
                    uint64_t& word = reinterpret_cast<uint64_t*>(r)[l];
                    if (q % 2 == 0) word |= uint64_t(field) | uint64_t(gap16) << 48;
                    else { word |= uint64_t(field) << 24; reinterpret_cast<uint16_t*>(r + kWaveLanes * 8)[l] = uint16_t(gap16); }
                };
                for (uint32_t l = 0; l < kWaveLanes; ++l) {
                    const uint64_t s0 = up.first_slot[w] + uint64_t(l) * up.lane_stride[w];
                    const uint32_t head = s0 >= up.slots ? scratch_pos : (s0 == 0 ? uint32_t(e[0] >> 32) : after[s0 - 1]);
                    put_slot(0, l, head & 0xffffffu, head >> 24);      // the head's position: field A | gap A << 24
                    for (uint32_t j = 0; j < up.run_len[w]; ++j) {
                        const uint64_t si = s0 + j;
                        put_slot(j + 1, l, si < up.slots ? val[si] >> shift : 0u, si < up.slots ? gap[si] : pad_gap);
                    }
                    for (uint32_t q = up.run_len[w] + 1; q < slots_in_records; ++q) put_slot(q, l, 0u, pad_gap);      // the dead slot of an odd run
                }
                continue;
            }
            // slot q of the run (q = 0: the head) sits in record q / 2, half q % 2: value word at (2 lane + half) * 4, gap at 512 + lane * 4 + half * 2
            auto value_at = [&](uint32_t q, uint32_t l) -> uint32_t& { return reinterpret_cast<uint32_t*>(rec + uint64_t(q / 2) * kRecordBytes)[2 * l + q % 2]; };
            auto gap_at = [&](uint32_t q, uint32_t l) -> uint16_t& { return reinterpret_cast<uint16_t*>(rec + uint64_t(q / 2) * kRecordBytes + kWaveLanes * 8)[2 * l + q % 2]; };
            for (uint32_t l = 0; l < kWaveLanes; ++l) {
                const uint64_t s0 = up.first_slot[w] + uint64_t(l) * up.lane_stride[w];
                // position BEFORE the run's first slot; slot 0 carries gap 0 from the first element's own position
                value_at(0, l) = s0 >= up.slots ? scratch_pos : (s0 == 0 ? uint32_t(e[0] >> 32) : after[s0 - 1]);
                for (uint32_t j = 0; j < up.run_len[w]; ++j) {
                    const uint64_t si = s0 + j;
                    value_at(j + 1, l) = si < up.slots ? val[si] : 0u;
                    gap_at(j + 1, l) = si < up.slots ? gap[si] : pad_gap;   // padding: see consume_block
                }
                for (uint32_t q = up.run_len[w] + 1; q < slots_in_records; ++q) gap_at(q, l) = pad_gap;      // the dead slot of an odd run
            }
        }
    });
    if (packed) {      // the outlier lists, behind the records: in the order of the units
        std::vector<uint32_t> unit;
        std::vector<Outlier> entry;
        for (size_t u = 0; u < unit_outliers.size(); ++u)
            for (const Outlier& o : unit_outliers[u]) { unit.push_back(uint32_t(u)); entry.push_back(o); }
        place_outliers(unit, entry);
        if (!entry.empty()) std::memcpy(image + image_bytes - ((outlier_count * sizeof(Outlier) + 15u) & ~uint64_t(15)), entry.data(), entry.size() * sizeof(Outlier));
    }
    finish_blocks();
    timer.lap("emit DELTA");
}

// One attempt at the image.  kOwner24DoesNotFit: a fixed-point OWNER24 image whose shares or step counts exceed the record format -- fixed
// point has no 8-byte OWNER form to fall back to, so build_stream_tiles plans again with owner_allowed = false.
enum class Attempt { kDone, kFailed, kOwner24DoesNotFit };

Attempt build_stream_tiles_attempt(const void* const channel[NUM_HBM_CHANNELS], const uint64_t n_packets[NUM_HBM_CHANNELS], const Geometry& geom,
                                   uint32_t num_rows, uint32_t num_cols, uint32_t num_row_partitions, uint32_t num_col_partitions,
                                   uint32_t max_workgroups, StreamTiles& out, std::string& error, void* gpu_stream, bool use_gpu,
                                   uint64_t image_slack, const CsrView* csr, bool owner_allowed) {
    const PlanSwitches sw = PlanSwitches::read();
    const uint64_t header_pkts = uint64_t(num_row_partitions) * num_col_partitions * (1 + geom.interleave);
    if (csr && !use_gpu) { error = "the CSR source needs the GPU re-tile"; return Attempt::kFailed; }
    for (uint32_t c = 0; !csr && c < NUM_HBM_CHANNELS; ++c) {
        if (!channel[c] && n_packets[c]) { error = "null channel buffer"; return Attempt::kFailed; }
        if (n_packets[c] < header_pkts) { error = "channel " + std::to_string(c) + " is shorter than its partition headers"; return Attempt::kFailed; }
    }
    out = StreamTiles();
    TileBuild b(channel, n_packets, geom, num_rows, num_cols, num_row_partitions, num_col_partitions, max_workgroups, out, error, image_slack, csr, sw);
    if (!b.count_rows(gpu_stream, use_gpu) || !b.take_census()) return Attempt::kFailed;
    const PlanInputs in = b.plan_inputs();
    const double hubs = hub_share(in);

    // ---- early exit 1: BITMAP rows (bitmap_tiles.cpp) ----
    const DenseRowChoice dense = choose_dense_rows(in);
    if (sw.format == ForcedFormat::kInvalid) { error = kBadStreamFormat; return Attempt::kFailed; }
    if (dense.bitmap) {
        // the per-non-zero passes of the BITMAP builder are kernels too (HISPARSE_BITMAP_BUILD=host: the host loops of round 2,
        // from the row counts the device returned -- the checker of tests/test_gpu_retile.py)
        const bool on_host = !b.gpu || sw.bitmap_on_host;
        if (on_host && !csr) b.gpu.reset();      // (a CSR source has no host fallback for the element formats: keep the tiler)
        if (build_bitmap_tiles(b.L, channel, n_packets, b.row_nnz, max_workgroups, out, error, csr, on_host ? nullptr : b.gpu.get(), image_slack)) return Attempt::kDone;
        if (error.rfind("bitmap:", 0) != 0) return Attempt::kFailed;     // a real decode error
        error.clear();                                       // not representable as a bitmap (duplicate entries): element streams
        // The bitmap builder may have filled `out` before it found the duplicate (the device builder sees it only in its mask
        // pass, after blocks / units / max_block_rows / col_slices were laid out): the element-format passes below push_back onto
        // these tables and derive their sort-key widths from their sizes, so give them `out` as pass 0 left it.
        reset_keeping_nnz(out);
    }
    // ---- early exit 2: SWEEP by the gap rules or forced (sweep_tiles.cpp) ----
    const SweepChoice sweep = choose_sweep(in);
    if (sweep.sweep) {
        reset_keeping_nnz(out);
        if (!build_sweep_tiles(b.L, channel, n_packets, b.row_nnz, max_workgroups, out, error, csr, b.gpu.get(), image_slack)) return Attempt::kFailed;
        out.spmm_vectors = sweep.for_spmm ? 4u : 1u;
        return Attempt::kDone;
    }
    // ---- the row-block plan; early exit 3: SWEEP by the tiny-unit rule ----
    b.plan = plan_row_blocks(in, hubs, dense, owner_allowed);
    if (b.plan.tiny_unit_sweep) {
        reset_keeping_nnz(out);
        return build_sweep_tiles(b.L, channel, n_packets, b.row_nnz, max_workgroups, out, error, csr, b.gpu.get(), image_slack) ? Attempt::kDone : Attempt::kFailed;
    }
    out.format = b.plan.format;
    out.light = b.plan.light;
    out.col_slices = b.plan.slices;

    b.cut_row_ranges();
    if (!b.count_units() || !b.enumerate_blocks() || !b.collect_and_sort()) return Attempt::kFailed;
    if (b.plan.delta() && !b.plan.format_forced && delta_or_pairs(b.plans, uint32_t(out.blocks.size()), out.nnz, b.is_float) == kFormatPairs) b.fall_back_to_pairs();
    b.timer.lap("sort units");
    if (b.plan.owner()) {
        if (!b.owner_shares(b.plan.owner24() ? kOwnerShareRows : 0xffffffffu)) return Attempt::kFailed;
        if (b.plan.owner24()) {
            const Owner24Fit fit = owner24_fit(out.blocks, b.plans);
            if (!b.is_float && !fit.fits) return Attempt::kOwner24DoesNotFit;
            if (b.is_float && (!fit.fits || (!b.plan.format_forced && !fit.smaller))) {
                b.set_format(kFormatOwner);
                if (!b.owner_shares(0xffffffffu)) return Attempt::kFailed;
            }
        }
        b.timer.lap("owner shares");
    }
    if (wants_pairs24(b.plan, sw, out.max_block_rows)) b.set_format(kFormatPairs24);
    if (!b.lay_out_streams()) return Attempt::kFailed;
    if (out.format == kFormatDelta && !b.choose_value_bits()) return Attempt::kFailed;
    b.assign_to_workgroups();
    if (b.gpu) return b.emit_on_gpu() ? Attempt::kDone : Attempt::kFailed;
    resize_zeroed(out.image, b.image_bytes);
    out.image_bytes = b.image_bytes;
    if (b.plan.owner()) b.emit_owner();
    else if (b.plan.delta()) b.emit_delta();
    else b.emit_pairs();
    return Attempt::kDone;
}

}  // namespace

bool build_stream_tiles(const void* const channel[NUM_HBM_CHANNELS], const uint64_t n_packets[NUM_HBM_CHANNELS],
                        const Geometry& geom, uint32_t num_rows, uint32_t num_cols, uint32_t num_row_partitions,
                        uint32_t num_col_partitions, uint32_t max_workgroups, StreamTiles& out, std::string& error,
                        void* gpu_stream, bool use_gpu, uint64_t image_slack, const CsrView* csr) {
    Attempt a = build_stream_tiles_attempt(channel, n_packets, geom, num_rows, num_cols, num_row_partitions, num_col_partitions, max_workgroups, out, error,
                                           gpu_stream, use_gpu, image_slack, csr, /*owner_allowed=*/true);
    // the second attempt never plans OWNER24 (automatic choice, forced owner24 -> PAIRS, float one-slice re-plan off), so it cannot end the same way
    if (a == Attempt::kOwner24DoesNotFit)
        a = build_stream_tiles_attempt(channel, n_packets, geom, num_rows, num_cols, num_row_partitions, num_col_partitions, max_workgroups, out, error,
                                       gpu_stream, use_gpu, image_slack, csr, /*owner_allowed=*/false);
    return a == Attempt::kDone;
}

}  // namespace dev
}  // namespace hisparse
