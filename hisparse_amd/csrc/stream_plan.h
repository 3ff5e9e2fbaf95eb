// stream_plan.h — the DECISIONS of the element-stream builder (stream_tiles.cpp), as functions over plain inputs: the options of a load read
// once (PlanSwitches), the tile census, and every choice made before the row ranges are cut -- hub share, BITMAP against sliced DELTA,
// SWEEP against OWNER24, the format by gap, LIGHT, the row-block cost loop -- plus those taken after the sort (delta_or_pairs,
// owner24_fit, wants_pairs24).  Nothing here touches a channel buffer, a StreamTiles or the GpuTiler; the passes that do are in stream_tiles.cpp.
// The cost-model expressions are compared as doubles: change none of them without tools/tiles_ab.py.
#ifndef HISPARSE_STREAM_PLAN_H_
#define HISPARSE_STREAM_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "stream_tiles.h"
#include "tiles_common.h"

namespace hisparse {
namespace dev {
namespace detail {

// ---- the options of one load, read ONCE at the top of the build on the calling thread (a context's option map must not change during its
//      load: tiles_common.h).  Nothing below the top of build_stream_tiles calls env_switch. -------------------------------------------------
enum class ForcedFormat { kNone, kPairs, kDelta, kOwner, kOwner24, kSweep, kBitmap, kInvalid };
struct IntSwitch {      // an option that is read with std::atoi where it is set
    bool set = false;
    int value = 0;
};
struct PlanSwitches {
    ForcedFormat format = ForcedFormat::kNone;      // HISPARSE_STREAM_FORMAT (kInvalid: reported after pass 0 and the census, where it always was)
    DeltaValueBits delta_bits = DeltaValueBits::kByRule;   // ... = delta24 / delta32: DELTA (kDelta above) with packed / plain value words whatever the rule says
    IntSwitch col_slices, max_rows, light, light_wgs, sweep, row_runs;
    bool spmm4 = false;             // HISPARSE_SPMM_VECTORS=4
    bool pow2_slices = false;       // HISPARSE_POW2_SLICES (set at all)
    bool aux24 = false;             // HISPARSE_AUX_BITS=24
    bool delta_spread = true;       // HISPARSE_DELTA_DEAL != wave
    bool xcd_affinity = false;      // HISPARSE_XCD_AFFINITY != 0
    bool census = true;             // HISPARSE_PLAN_CENSUS != 0
    bool bitmap_on_host = false;    // HISPARSE_BITMAP_BUILD=host
    bool cross_parts = true;        // HISPARSE_CROSS_PARTITIONS != 0
    bool debug = false;             // HISPARSE_PLAN_DEBUG (set at all)
    bool format_set() const { return format != ForcedFormat::kNone; }

    static PlanSwitches read() {
        PlanSwitches sw;
        auto number = [](const char* name) {
            IntSwitch s;
            if (const char* v = env_switch(name)) { s.set = true; s.value = std::atoi(v); }
            return s;
        };
        if (const char* force = env_switch("HISPARSE_STREAM_FORMAT")) {
            const std::string f(force);
            if (f == "delta24") sw.delta_bits = DeltaValueBits::kPacked;
            if (f == "delta32") sw.delta_bits = DeltaValueBits::kPlain;
            sw.format = f == "pairs" ? ForcedFormat::kPairs : (f == "delta" || f == "delta24" || f == "delta32") ? ForcedFormat::kDelta : f == "owner" ? ForcedFormat::kOwner :
                        f == "owner24" ? ForcedFormat::kOwner24 : f == "sweep" ? ForcedFormat::kSweep : f == "bitmap" ? ForcedFormat::kBitmap : ForcedFormat::kInvalid;
        }
        sw.col_slices = number("HISPARSE_COL_SLICES");
        sw.max_rows = number("HISPARSE_MAX_ROWS");
        sw.light = number("HISPARSE_LIGHT");
        sw.light_wgs = number("HISPARSE_LIGHT_WGS");
        sw.sweep = number("HISPARSE_SWEEP");
        sw.row_runs = number("HISPARSE_ROW_RUNS");
        sw.spmm4 = number("HISPARSE_SPMM_VECTORS").value == 4;
        sw.pow2_slices = env_switch("HISPARSE_POW2_SLICES") != nullptr;
        sw.aux24 = number("HISPARSE_AUX_BITS").value == 24;
        if (const char* deal = env_switch("HISPARSE_DELTA_DEAL")) sw.delta_spread = std::string(deal) != "wave";
        sw.xcd_affinity = number("HISPARSE_XCD_AFFINITY").value != 0;
        const IntSwitch census = number("HISPARSE_PLAN_CENSUS");      // 0: plan as rounds 1-5 did, from the row counts alone (A/B, tools/planner_check.py)
        sw.census = !(census.set && census.value == 0);
        if (const char* where = env_switch("HISPARSE_BITMAP_BUILD")) sw.bitmap_on_host = std::string(where) == "host";
        const IntSwitch cross = number("HISPARSE_CROSS_PARTITIONS");
        if (cross.set) sw.cross_parts = cross.value != 0;
        sw.debug = env_switch("HISPARSE_PLAN_DEBUG") != nullptr;
        return sw;
    }
};
inline const char* const kBadStreamFormat = "HISPARSE_STREAM_FORMAT must be pairs, delta, delta24, delta32, owner, owner24, sweep or bitmap";

// ---- one copy of the rules that the census and the builder must apply alike -----------------------------------------------------------

// Column slices of one row range: its sub-tiles are dealt to the slices heaviest first, each to the lightest slice so far (ties: the one
// with fewer sub-tiles).  tile_load[k]: non-zeros of sub-tile k (the census evaluates plans in double, the builder counts in uint64_t);
// slice_load / slice_tiles[slices]: zeroed by the caller; slice_of[k] (may be null): the slice sub-tile k went to.
template <typename Load>
inline void deal_tiles_to_slices(const std::vector<Load>& tile_load, uint32_t slices, std::vector<uint32_t>& by_weight, Load* slice_load,
                                 uint32_t* slice_tiles, uint32_t* slice_of) {
    std::iota(by_weight.begin(), by_weight.end(), 0u);
    std::stable_sort(by_weight.begin(), by_weight.end(), [&](uint32_t x, uint32_t y) { return tile_load[x] > tile_load[y]; });
    for (uint32_t k : by_weight) {
        uint32_t best = 0;
        for (uint32_t c = 1; c < slices; ++c)
            if (slice_load[c] < slice_load[best] || (slice_load[c] == slice_load[best] && slice_tiles[c] < slice_tiles[best])) best = c;
        if (slice_of) slice_of[k] = best;
        slice_load[best] += tile_load[k];
        slice_tiles[best] += 1;     // empty sub-tiles still spread evenly (they cost nothing, but keep the rule simple)
    }
}

// PAIRS: a block of a few long rows takes the dense-row path (a wavefront sums a row in registers)
inline bool pairs_block_is_dense(const RowRange& range, uint64_t range_nnz) {
    return range.nrows <= kDenseBlockRows && range_nnz >= 64ull * range.nrows;
}

// ---- tile census (round 6) -------------------------------------------------------------------------------------------------------------
// Until round 5 the plan was made from the rows' non-zero counts alone, i.e. as if every row range met every x sub-tile with the same number
// of elements.  True enough for the scrambled power-law graphs and the Bernoulli layers the constants were measured on -- and wrong by
// 2-6 x on anything with STRUCTURE (tools/planner_check.py, profiles/r06_planner_check_before.txt): a banded or block-diagonal matrix keeps a
// row range's elements in two or three sub-tiles, so a plan of 51 row ranges x 5 column slices has 102 blocks that hold anything, on 102 of
// 256 workgroups (banded 400 K: 56.9 us in the planner's 5 slices, 21.3 us in one).  The census is what the model lacked: non-zeros per
// (fine row range, sub-tile) for `fine` ranges of equal non-zero count -- one more counting pass (the pass-1 kernel / walk with another row
// map) -- from which every candidate plan's REAL units (the non-empty ones), block loads (sub-tiles dealt to slices the way the builder
// deals them) and workgroup loads (heaviest block first, the way assign_workgroups balances) follow.
struct TileCensus {
    uint32_t fine = 0, tiles = 0;
    std::vector<uint32_t> cnt;          // [fine][tiles]
    double populated = 1.0;             // fraction of the (fine range, sub-tile) cells that hold anything
    struct Eval { double nonempty_units, max_wg_load; };
    // a plan of `plan_ranges` row ranges (equal non-zero count, in row order) x `cs` column slices on G workgroups
    Eval evaluate(uint64_t plan_ranges, uint32_t cs, uint32_t G, uint64_t nnz) const {
        plan_ranges = std::max<uint64_t>(1, plan_ranges);
        if (cnt.empty() || !fine) {      // no census (matrix without non-zeros): the uniform picture
            const double blocks = double(plan_ranges) * cs, per_wg = std::ceil(blocks / G);
            return {double(plan_ranges) * tiles, double(nnz) / blocks * per_wg};
        }
        // more plan ranges than census rows: every census row stands for `split` plan ranges of 1 / split of its non-zeros
        const uint64_t split = plan_ranges > fine ? (plan_ranges + fine - 1) / fine : 1;
        const uint64_t groups = plan_ranges > fine ? fine : plan_ranges;
        std::vector<double> t(tiles), block_load;
        std::vector<uint32_t> order(tiles);
        block_load.reserve(size_t(groups * split) * cs);
        double nonempty = 0.0;
        std::vector<double> slice_load(cs);
        std::vector<uint32_t> slice_tiles(cs);
        for (uint64_t j = 0; j < groups; ++j) {
            const uint64_t lo = j * fine / groups, hi = (j + 1) * fine / groups;
            std::fill(t.begin(), t.end(), 0.0);
            for (uint64_t f = lo; f < hi; ++f)
                for (uint32_t k = 0; k < tiles; ++k) t[k] += cnt[f * tiles + k];
            uint32_t live = 0;
            for (uint32_t k = 0; k < tiles; ++k) live += t[k] > 0.0;
            nonempty += double(live) * double(split);
            std::fill(slice_load.begin(), slice_load.end(), 0.0);
            if (cs == 1) {
                for (uint32_t k = 0; k < tiles; ++k) slice_load[0] += t[k];
            } else {      // the builder's dealing
                std::fill(slice_tiles.begin(), slice_tiles.end(), 0u);
                deal_tiles_to_slices(t, cs, order, slice_load.data(), slice_tiles.data(), nullptr);
            }
            for (uint64_t rep = 0; rep < split; ++rep)
                for (uint32_t c = 0; c < cs; ++c) block_load.push_back(slice_load[c] / double(split));
        }
        // heaviest block first, each to the workgroup with the least work so far (assign_workgroups)
        std::sort(block_load.begin(), block_load.end(), std::greater<double>());
        std::vector<double> wg(std::max<uint32_t>(1, G), 0.0);
        std::make_heap(wg.begin(), wg.end(), std::greater<double>());
        double worst = 0.0;
        for (double b : block_load) {
            std::pop_heap(wg.begin(), wg.end(), std::greater<double>());
            wg.back() += b;
            worst = std::max(worst, wg.back());
            std::push_heap(wg.begin(), wg.end(), std::greater<double>());
        }
        return {std::max(1.0, nonempty), std::max(worst, double(nnz) / G)};
    }
};

// What every decision below is made from.  (References: the builder's state outlives the plan.)
struct PlanInputs {
    const Layout& L;
    const std::vector<uint32_t>& row_nnz;
    uint64_t nnz;
    const TileCensus& census;
    uint32_t max_workgroups;
    bool is_float;
    const PlanSwitches& sw;
};

// ---- hub rows (round 6) ---------------------------------------------------------------------------------------------------------------
// A row that holds a large part of its row block puts most lanes of a step on ONE LDS accumulator: same-address ds_add serialises, and a
// matrix whose 50 hub rows hold 64 % of the non-zeros (tools/planner_check.py: hubs_500k) ran 89 us as the PAIRS image the mean gap
// picked, 94 us as a DELTA image -- and 44.9 us as a DELTA image whose lanes sum their runs in registers (kBlockDenseRows: one LDS add per
// lane and row change), which until now only blocks of uniformly long rows got.  So: (a) a DELTA block whose heaviest row holds an
// eighth of it is flagged for per-lane sums whatever its mean gap (stream_tiles.cpp: TileBuild::block_flags); (b) where rows heavy enough to fill a
// quarter of a workgroup's share hold >= 30 % of the matrix, the DELTA image is kept even if PAIRS would be smaller.  Forcing per-lane
// sums on every block costs an ordinary graph 20 % (rmat19: 32.0 -> 39.1 us), hence per block.
inline double hub_share(const PlanInputs& in) {
    const uint64_t hub_min = std::max<uint64_t>(8192, in.nnz / (4ull * std::max<uint32_t>(1, in.max_workgroups)));
    uint64_t in_hubs = 0;
    for (uint32_t r = 0; r < in.L.num_rows; ++r) in_hubs += in.row_nnz[r] >= hub_min ? in.row_nnz[r] : 0u;
    return in.nnz ? double(in_hubs) / double(in.nnz) : 0.0;
}

// ---- dense-row matrices (pruned-NN layers): BITMAP rows, their own builder and kernel (stream_tiles.h) --------------
struct DenseRowChoice {
    bool bitmap = false;
    bool prefer_sliced_delta = false, sliced_delta_possible = false;      // (prefer: decided here or by choose_light)
    double sliced_delta_us = 0.0;
};
inline DenseRowChoice choose_dense_rows(const PlanInputs& in) {
    const uint32_t num_rows = in.L.num_rows, num_cols = in.L.num_cols, max_workgroups = in.max_workgroups, RP = in.L.row_parts;
    const uint64_t nnz = in.nnz;
    const bool is_float = in.is_float;
    DenseRowChoice d;
    // density of the rows that hold anything (padding rows and empty rows cost a mask per group and nothing else -- as long as
    // all masks together stay below a quarter of the 8 bytes per non-zero they replace)
    uint64_t live_rows = 0;
    for (uint32_t r = 0; r < num_rows; ++r) live_rows += in.row_nnz[r] != 0;
    const double density = live_rows ? double(nnz) / (double(live_rows) * double(num_cols)) : 0.0;
    const double mask_bytes = double(num_rows) * double((num_cols + kBitmapGroupCols - 1) / kBitmapGroupCols) * 8.0;
    d.bitmap = density >= kBitmapMinDensity && num_cols >= kBitmapMinCols && mask_bytes <= 2.0 * double(nnz);
    // Round 5: SMALL dense-row layers in FIXED point as a sliced DELTA plan.  With the combine pass carried into the next step's kernel
    // (hs_context.h: CarriedCombine) a plan of one column slice per x sub-tile is ONE launch without x refills and unit barriers, and its lanes sum their
    // rows in registers (kBlockDenseRows): measured on the 512 x 33 288 pruned-NN layers (profiles/r05_sliced_delta_vs_bitmap.txt, fixed
    // point, whole step; with the lane-major dealing of the runs, "after the dealing" there): 10 % dense 7.5 us against 8.6 (LIGHT), 20 % 9.0
    // against 11.9 (BITMAP), 30 % 11.0 against 12.0, 40 % 12.5 against 12.4, 5 % 6.9 against 5.9 (LIGHT) -- ~5.8 us + 1.0 us per million
    // non-zeros, where the BITMAP kernel pays for every 64-column group
    // whatever it holds (~5 us + 7.5 ns per step and CU) and the LIGHT kernel 3.1 us + 3.2 us per million.  The float modes keep their
    // plans: their BITMAP kernel is 2 us faster and their DELTA path 1 us slower, which leaves 0.4-0.5 us at 10 % and 20 % density and a
    // loss everywhere else.
    {
        const uint32_t live_tiles = (num_cols + kSubTileCols - 1) / kSubTileCols;
        const double scale = 256.0 / std::max<uint32_t>(1, max_workgroups);
        d.sliced_delta_us = 5.8 + double(nnz) * 1.0e-6 * scale;
        d.sliced_delta_possible = !is_float && live_tiles >= 1 && live_tiles <= kMaxColSlices && density >= 0.04 && num_cols >= kBitmapMinCols &&
                                  double(nnz) * 7.0 < double(kSlicedDeltaMaxImageBytes) && RP == 1 && nnz >= (1u << 20);      // (measured between 0.85 and 8.5 M non-zeros)
        const double bitmap_us = 5.0 + double(num_rows) * double((num_cols + kBitmapGroupCols - 1) / kBitmapGroupCols) / std::max<uint32_t>(1, max_workgroups) * 7.5e-3;
        if (d.bitmap && d.sliced_delta_possible && d.sliced_delta_us < 0.97 * bitmap_us && !in.sw.format_set()) {
            d.bitmap = false;
            d.prefer_sliced_delta = true;
        }
        if (in.sw.debug)
            std::fprintf(stderr, "format: dense rows (density %.3f): bitmap %.1f us, sliced delta %.1f us (%s) -> %s\n", density, bitmap_us, d.sliced_delta_us,
                         d.sliced_delta_possible ? "possible" : "not possible", d.prefer_sliced_delta ? "sliced delta" : d.bitmap ? "bitmap" : "element streams");
    }
    if (in.sw.format_set() && in.sw.format != ForcedFormat::kInvalid) d.bitmap = in.sw.format == ForcedFormat::kBitmap;
    return d;
}

// ---- SWEEP (stream_tiles.h): hyper-sparse matrices whose x is gathered from L2 instead of staged in LDS -- its own builder (host threads)
//      and kernel.  HISPARSE_SWEEP=0|1 and HISPARSE_STREAM_FORMAT=sweep force.
struct SweepChoice { bool sweep, for_spmm; };
inline SweepChoice choose_sweep(const PlanInputs& in) {
    const Layout& L = in.L;
    const uint32_t num_rows = L.num_rows, num_cols = L.num_cols, max_workgroups = in.max_workgroups, RP = L.row_parts, CP = L.col_parts, S = L.subs_per_cp;
    const uint64_t nnz = in.nnz;
    const bool is_float = in.is_float;
    const TileCensus& census = in.census;
    // Unforced: wherever OWNER24 would be taken (mean position gap > kOwnerMinMeanGap) and SWEEP's plan is modelled faster than OWNER24's.
    // OWNER24 pays ~1.2 us + 0.06 us per wavefront step for every (row range x sub-tile) unit whatever it holds (tools/perf_model.py:
    // UNIT_FLOOR_US, fitted to the rocprofv3 kernels), and its planner cuts at least max_workgroups / 8 row ranges to fill the CUs; the
    // estimate below lands 10 % under the measured steps on six matrices (pokec 87 / 95.5 us, ogbn-products 190 / 205, an 8-way slab of it
    // 60.5 / 59.2, power-law squares 42.5 / 48, 86.6 / 99, 173 / 185), SWEEP's model within 3 %: hence the factor.  What the comparison
    // reproduces (stream_tiles.h, "SWEEP format", has the tables): pokec -> SWEEP, ogbn-products -> OWNER24, ogbn-products cut into 8
    // row slabs (same gap, a quarter of the row ranges: 59.2 -> 46.3 us) -> SWEEP.
    // (the mean position gap INSIDE the (row range x sub-tile) cells that hold anything: a banded or block-diagonal matrix of 12 non-zeros per
    //  row over a million columns is not hyper-sparse where its elements are -- banded 1 M x 1 M, float_stall: 63 us as the SWEEP image the
    //  plain gap asked for, 27 us as a DELTA image)
    const double gap = nnz ? double(num_rows) * double(num_cols) / double(nnz) * census.populated : 0.0;
    bool sweep = false;
    // (from kSweepMinNnz on; smaller matrices too where x is wider than the LIGHT plan's sixteen sub-tiles -- a quarter slab of a 100 K x 4 M
    //  bipartite graph, 1.5 M non-zeros over 489 sub-tiles: 55.9 us as an OWNER24 image of 15 648 units, 11.2 us as a SWEEP image)
    if (gap > kOwnerMinMeanGap && (nnz >= kSweepMinNnz || (nnz >= kSweepMinNnzWide && uint64_t(CP) * S > kLightMaxUnits)) && uint64_t(num_cols) * 4 < (1ull << 32)) {
        uint32_t cs = 1, rows_cap = 0;
        uint64_t want = 1;
        const double sweep_us = sweep_plan(L, nnz, max_workgroups, cs, want, rows_cap);
        const uint32_t cap = owner_max_block_rows(2), G = std::max<uint32_t>(1, max_workgroups);
        uint64_t by_cap = 0;
        for (uint32_t rp = 0; rp < RP; ++rp) by_cap += (uint64_t(L.rows_in_part(rp)) + cap - 1) / cap;
        const double ranges = double(std::max<uint64_t>(by_cap, G / kMaxColSlices));
        const double units = std::max(1.0, ranges * double(CP) * S * census.populated), per_wg = units / G, unit_steps = double(nnz) / units / (kConsumerWaves * kWaveLanes);
        const double owner_slices = std::min<double>(kMaxColSlices, std::max(1.0, std::ceil(G / ranges)));
        const double owner_combine = owner_slices > 1.0 ? 2.0 + double(num_rows) * 4.0 * (owner_slices + 1.0) / 8e6 : 0.0;
        const double owner_us = 1.1 * (std::max(double(nnz) * 7.06 / 6.2e6, per_wg * (1.2 + 0.06 * unit_steps)) + 8.0 + owner_combine);
        sweep = sweep_us < owner_us;
        if (in.sw.debug) std::fprintf(stderr, "format: sweep %.1f us (%u slices) against owner24 %.1f us (%.0f units per workgroup) -> %s\n", sweep_us, cs, owner_us, per_wg, sweep ? "sweep" : "owner24");
    }
    // Short, wide, moderately sparse slabs whose image stays in the Infinity Cache (round 5, the round's last measurement,
    // profiles/r05_hollywood_slab_sweep.txt): one rank's slab of hollywood split 8 ways -- 133 K rows x 1.07 M columns, gap 10 K, 113 MB -- runs
    // 25.4-25.8 us as a SWEEP image (9 slices; ring depth 4, streamed without `nt`) against 31.0 us under the row-block planner's choice (PAIRS, 8
    // slices x 16 units per block of 3.4 K elements: a barrier and an x refill per unit).  Fixed point only, >= 6 columns per row and a gap
    // above kSweepSlabMinMeanGap: what was measured, no further; the float modes and the 4-way slabs keep their plans until they are.
    if (!sweep && !is_float && gap > kSweepSlabMinMeanGap && gap <= kOwnerMinMeanGap && nnz >= kSweepMinNnz && uint64_t(num_cols) >= 6ull * num_rows &&
        double(nnz) * 8.1 <= double(kResidentMaxImageBytes) && uint64_t(num_cols) * 4 < (1ull << 32)) {
        sweep = true;
        if (in.sw.debug) std::fprintf(stderr, "format: sweep for a short, wide slab (gap %.0f, %u x %u)\n", gap, num_rows, num_cols);
    }
    // "spmm_vectors" = 4: the caller wants the four-vector SpMM kernel, which runs SWEEP images only (spmm_sweep.hip)
    const bool for_spmm = in.sw.spmm4 && nnz > 0 && uint64_t(num_cols) * 16 < (1ull << 32);
    if (for_spmm) sweep = true;
    if (in.sw.sweep.set) sweep = in.sw.sweep.value != 0;      // (1: whatever the matrix)
    if (in.sw.format_set()) sweep = in.sw.format == ForcedFormat::kSweep;
    return {sweep, for_spmm};
}

// ---- the row-block plan: format, LIGHT, column slices x rows per block ------------------------------------------------------------------
struct TilePlan {
    StreamFormat format = kFormatPairs;
    bool light = false;
    bool format_forced = false;      // the post-sort revisions (delta_or_pairs, "is OWNER24 smaller") leave the format alone
    uint32_t G = 1, slices = 1, max_rows = 1;
    double best = 1e30, best_units = 1.0;      // the chosen tile plan's modelled cost BESIDE its stream (us); its non-empty (row range x sub-tile) units
    bool tiny_unit_sweep = false;    // the tiny-unit rule: build a SWEEP image instead (nothing else of the plan is valid then)
    bool delta() const { return format == kFormatDelta; }
    bool owner() const { return format == kFormatOwner || format == kFormatOwner24; }
    bool owner24() const { return format == kFormatOwner24; }      // may still fall back to the 8-byte form (owner24_fit)
    bool aux24() const { return format == kFormatPairs24; }
    uint32_t acc_bytes() const { return owner() ? kOwnerAccumulatorBytes : kAccumulatorBytes; }
    uint32_t spare_rows() const { return owner() ? kConsumerWaves : 1u; }     // accumulators behind the block's rows that padding elements aim at
};

// ---- stream format (stream_tiles.h): DELTA for matrices that are sparse but not hyper-sparse; hyper-sparse float matrices: OWNER --
// owner_allowed = false (the second attempt after a fixed-point OWNER24 image did not fit): never OWNER24, a forced owner24 gives PAIRS
inline StreamFormat choose_stream_format(const PlanInputs& in, double hub_share, bool prefer_sliced_delta, bool owner_allowed, bool& keep_delta_for_hubs) {
    const uint32_t num_rows = in.L.num_rows, num_cols = in.L.num_cols;
    const uint64_t nnz = in.nnz;
    const double mean_gap = nnz ? double(num_rows) * double(num_cols) / double(nnz) * in.census.populated : 1e30;      // (inside the populated cells, see SWEEP above)
    StreamFormat format = (mean_gap >= kDeltaMinMeanGap && mean_gap <= kDeltaMaxMeanGap) ? kFormatDelta : kFormatPairs;
    // hyper-sparse matrices: OWNER, in its 7-byte record form (OWNER24) unless that turns out larger (decided after the sort).  Fixed
    // point too since round 3: saturating 32-bit accumulators (spmv_kernels.hip: OwnerOps) -- pokec in PAIRS, with 8-byte atomic
    // accumulators, 12287-row blocks and 26 600 units of 1 150 elements, ran at 24 % of the roofline
    if (mean_gap > kOwnerMinMeanGap && nnz >= 4096 && owner_allowed) format = kFormatOwner24;
    if (prefer_sliced_delta) format = kFormatDelta;
    if (format == kFormatDelta && hub_share >= 0.3 && !prefer_sliced_delta) keep_delta_for_hubs = true;      // (hub rows, above)
    if (in.sw.debug && hub_share > 0.0)
        std::fprintf(stderr, "format: %.1f %% of the non-zeros in hub rows%s\n", hub_share * 100.0, keep_delta_for_hubs ? " -> DELTA kept for its per-lane row sums" : "");
    switch (in.sw.format) {
        case ForcedFormat::kPairs: format = kFormatPairs; break;
        case ForcedFormat::kDelta: format = kFormatDelta; break;
        case ForcedFormat::kOwner: format = in.is_float ? kFormatOwner : kFormatPairs; break;   // float accumulators only
        case ForcedFormat::kOwner24: format = owner_allowed ? kFormatOwner24 : kFormatPairs; break;
        default: break;   // bitmap: was tried and is not representable (duplicate entries): automatic choice
    }
    return format;
}

// ---- LIGHT plan (stream_tiles.h): a small matrix is launch-bound in the row-block kernel -- one slice, up to 4 x CUs small blocks of a
//      PAIRS image, linear dealing, spmv_light_kernel.  Automatic when no format is forced; HISPARSE_LIGHT=0|1 forces (1: with any
//      matrix of at most kLightMaxUnits sub-tiles whose format is not forced to something other than pairs).
// (may still turn a 10 %-dense layer into the sliced DELTA plan: `dense` and `format` are updated)
inline bool choose_light(const PlanInputs& in, DenseRowChoice& dense, StreamFormat& format) {
    const uint32_t num_rows = in.L.num_rows, max_workgroups = in.max_workgroups, CP = in.L.col_parts, S = in.L.subs_per_cp;
    const uint64_t nnz = in.nnz;
    const bool forced = in.sw.format_set();
    const bool fits = nnz > 0 && uint64_t(CP) * S <= kLightMaxUnits && num_rows < (1u << 31);
    bool light = fits && !forced && nnz <= kLightMaxNnz && !dense.prefer_sliced_delta;
    if (light && dense.sliced_delta_possible && dense.sliced_delta_us < 0.97 * (3.1 + double(nnz) * 3.2e-6 * 256.0 / std::max<uint32_t>(1, max_workgroups))) {
        light = false;                       // (10 %-dense layers: see choose_dense_rows)
        dense.prefer_sliced_delta = true;
        format = kFormatDelta;
    }
    if (in.sw.light.set) light = in.sw.light.value != 0 && fits && (!forced || in.sw.format == ForcedFormat::kPairs);
    if (in.sw.col_slices.set) light = light && in.sw.col_slices.value <= 1;      // a forced sliced plan is the row-block kernel's
    if (light) format = kFormatPairs;
    return light;
}

// ---- tile plan: column slices x (rows per block, x ring depth) ------------------------------------------------
// More column slices = longer row ranges = less x pulled through every CU, at the price of the combine pass; fewer
// rows per block = deeper x ring = refill latency hidden even when a (row range, sub-tile) unit holds only a few
// thousand non-zeros (hyper-sparse matrices).  Cost model in microseconds, constants measured on MI355X:
//   x volume through one CU at ~120 GB/s; a refill takes ~0.8 us to land, ring-1 of them overlap, a unit's stream
//   time (~25 GB/s per CU) hides the rest; ~8 us of prologue + epilogue per block; the combine kernel.
// Sets p.slices / p.max_rows / p.best / p.best_units for the format, G and format_forced that p holds.
inline void cost_row_block_plans(const PlanInputs& in, TilePlan& p) {
    const Layout& L = in.L;
    const uint32_t num_rows = L.num_rows, num_cols = L.num_cols, CP = L.col_parts, S = L.subs_per_cp, G = p.G;
    const uint64_t nnz = in.nnz;
    const bool is_float = in.is_float, delta = p.delta(), owner = p.owner(), format_forced = p.format_forced;
    const TileCensus& census = in.census;
    const uint32_t acc_bytes = p.acc_bytes(), spare_rows = p.spare_rows();
    const bool force_slices = in.sw.col_slices.set, force_rows = in.sw.max_rows.set;   // experiments
    struct Shape { uint32_t cap, ring; };
    // OWNER: 4-byte accumulators -> 24561 rows with a ring of 2, 16369 with a ring of 3, sliced or not
    const Shape sliced[2] = {{owner ? owner_max_block_rows(2) : max_block_rows(true), 2},
                             {owner ? owner_max_block_rows(3) : (kMaxLdsBytes - 3 * kSubTileCols * 4) / kAccumulatorBytes - 1, 3}};   // 12287 / 8191 rows
    const Shape whole[1] = {{max_block_rows(false), kMaxXBuffers}};                                       // 4095 rows, ring 4
    const double sub_tiles = double(CP) * S;
    std::map<uint64_t, TileCensus::Eval> census_memo;
    p.best = 1e30;
    for (uint32_t cs = 1; cs <= (force_slices ? kMaxForcedColSlices : kMaxColSlices); ++cs) {
        // unforced: every count the cost model likes.  (Through round 4 only 1, 2, 4, 8 for matrices of more than sixteen sub-tiles -- everything
        // in between for OWNER, where the x volume decides: ogbn-products runs 241 us in 5 slices (102 ranges of 24 K rows, 2 blocks per
        // workgroup) against 280 in 2 (127 ranges) and 275 in 4 -- because five slices had measured as a wash on ogbl-ppa and 3 us slower on
        // its R-MAT stand-in, a PAIRS image then.  Measured again in round 5 (profiles/r05_any_slice_count.txt, whole step, alternating):
        // ogbl-ppa 55.2-56.0 us in 4 slices, 54.0-54.5 in 5 (51 row ranges x 5 = 255 blocks: fewer, longer units); the R-MAT stand-in
        // 58.4-59.0 -> 55.2-55.4; hollywood keeps 2, its slabs and ogbl-ppa's keep 8 (a 2-way slab takes 5 or 7: +-1 %).
        // HISPARSE_POW2_SLICES=1 brings the old rule back for the A/B.)
        // (a matrix of at most sixteen sub-tiles: a slice per sub-tile (or two) is the plan without x refills and
        // unit barriers (gplus, 14 sub-tiles: 23.7 us in 7 slices, 26.1 in 8), and a power of two above the sub-tile count would leave
        // whole slices, i.e. workgroups, empty)
        const uint32_t live_tiles = (num_cols + kSubTileCols - 1) / kSubTileCols;
        if (force_slices ? uint32_t(in.sw.col_slices.value) != cs : (!owner && (cs & (cs - 1)) != 0 && live_tiles > 2 * kMaxColSlices && in.sw.pow2_slices)) continue;
        if (cs > 1 && uint64_t(CP) * S < cs) continue;                                    // fewer sub-tiles than slices
        if (!force_slices && !owner && live_tiles <= kMaxColSlices && cs > live_tiles) continue;
        for (const Shape& shape : (cs > 1 || owner) ? std::vector<Shape>(sliced, sliced + 2) : std::vector<Shape>(whole, whole + 1)) {
            uint32_t cap = shape.cap, ring = shape.ring;
            if (force_rows) {
                cap = std::min<uint32_t>(cap, std::max(1, in.sw.max_rows.value));
                ring = std::max(kMinXBuffers, std::min(kMaxXBuffers, (kMaxLdsBytes - (cap + spare_rows) * acc_bytes) / (kSubTileCols * 4u)));
            }
            const uint64_t per_round = std::max<uint32_t>(1, G / cs);
            const uint64_t need = (uint64_t(num_rows) + cap - 1) / cap;
            const double ranges = double(per_round * std::max<uint64_t>(1, (need + per_round - 1) / per_round));
            const double blocks_per_wg = ranges * cs / G;
            // the plan's real units and loads (TileCensus): the non-empty (row range x sub-tile) cells, the heaviest workgroup's share
            const uint64_t memo_key = (uint64_t(ranges) << 8) | cs;
            auto found = census_memo.find(memo_key);
            if (found == census_memo.end()) found = census_memo.emplace(memo_key, census.evaluate(uint64_t(ranges), cs, G, nnz)).first;
            const TileCensus::Eval& real = found->second;
            const double units_per_wg = std::max(1.0, real.nonempty_units / G);
            const double unit_stream_us = double(nnz) * 8.0 / (units_per_wg * G) / 25e3;
            // x pulled through a CU: 120 GB/s next to a DELTA / PAIRS stream (ogbl-ppa: 0.1 us per row range); OWNER's units are
            // short and every one ends in a flush and a barrier, which also scale with the ranges: 1.34 us per range on
            // ogbn-products = 29 GB/s (tools/slices_probe.sh)
            const double volume_us = real.nonempty_units * double(L.sub_width) * 4.0 / G / (owner ? 29e3 : 120e3);      // (uniform matrix: ranges x num_cols x 4 bytes)
            double latency_us = units_per_wg * std::max(0.0, 0.8 / (ring - 1) - unit_stream_us);
            // Blocks of a few long rows (<= kDenseBlockRows) take the dense-row path: a wavefront sums a row in registers and pays a
            // wavefront-wide reduction at every row change.  That is right for rows that fill many chunks of a sub-tile (pruned-NN
            // layers: 16 K non-zeros per row) and slow when a (row, sub-tile) holds only a chunk or two -- one rank's slab of mouse_gene
            // split 8 ways (5632 rows x 45 K columns, 22-row blocks, 117 non-zeros per row and sub-tile) ran 2.5 us per unit, 22.7 us
            // for 29 MB; in 3 column slices (blocks of 66 rows, ordinary path) 11.5 us + the combine pass.  Price it.
            // an unsliced block walks ALL sub-tiles: every unit boundary costs it a head record per wavefront, a barrier and a refill
            // issue, ~0.3 us that the stream does not hide (gplus, 14 units per block: 28.6 us in one slice, 24.0 in seven, same
            // format; mouse_gene's 2-way slabs 21.9 -> 20.8) -- sliced plans have a fraction of the units and pay the combine pass instead
            if (!owner && cs == 1) latency_us += units_per_wg * 0.3;
            // few sub-tiles dealt to slices that do not divide them: the blocks of the slices with one sub-tile more set the time (gplus,
            // 14 sub-tiles: 23.9 / 27.4 / 24.7 / 26.1 us in 5 / 6 / 7 / 8 slices)
            if (!owner && cs > 1 && live_tiles <= 2 * kMaxColSlices)
                latency_us += 0.75 * (double(nnz) * 8.0 / G / 25e3) * (double((live_tiles + cs - 1) / cs) * cs / live_tiles - 1.0);
            const double rows_per_block = double(num_rows) / ranges, per_row_and_tile = double(nnz) / std::max(1.0, double(num_rows) * sub_tiles * census.populated);
            if (!owner && rows_per_block <= kDenseBlockRows && per_row_and_tile < 4.0 * kWaveLanes) latency_us += units_per_wg * 1.75;
            // PAIRS deals a unit's elements, sorted by (row, column), to the lanes in consecutive runs: the 64 lanes of a step sit
            // 1/896 of the unit apart, and when the block has fewer than 896 rows several of them are in the SAME row -- their
            // ds_add_u64 on one accumulator are serialised.  One rank's slab of mouse_gene split 4 ways (44-row blocks, ~20 lanes
            // per row): 15-26 us in one slice against 12.7-13.7 us in six (268-row blocks, one sub-tile each, combine pass included).
            // ~2 clocks per extra lane and wavefront step, all wavefronts of a workgroup through the one LDS.  (DELTA blocks of
            // long rows keep per-lane sums instead -- no atomics to collide.)
            const double lanes_per_row = std::min(64.0, 896.0 / std::max(1.0, rows_per_block));
            // (DELTA is still tentative here: below ~1.6 bytes saved per non-zero x nnz < the threshold it falls back to PAIRS, see delta_or_pairs)
            const bool pairs_likely = !delta || (!format_forced && double(nnz) * 1.6 < double(is_float ? kDeltaMinSavedBytesFloat : kDeltaMinSavedBytes));
            const double conflict_us = (!owner && pairs_likely && lanes_per_row > 1.0 && per_row_and_tile >= 16.0)
                                           ? double(nnz) / G / kWaveLanes * (lanes_per_row - 1.0) * 2.0 / 2400.0 : 0.0;
            // the combine pass: a launch of its own (3.5 us) + its traffic -- or ~1 us of the NEXT step's kernel where the image is small
            // enough for the carried combine (hs_context.h: CarriedCombine; stream_tiles.h: plan_carries)
            const bool carried = double(nnz) * 8.1 < double(kCarryMaxImageBytes);
            const double combine_us = cs > 1 ? (carried ? 1.0 : 3.5) + double(num_rows) * 4.0 * (cs + 1) / 4e6 : 0.0;
            // workgroup slots that get no block (7 slices x 36 row ranges = 252 blocks on 256 workgroups): the stream they would have taken
            // is the others' -- what tells 7 slices from 8 on mid-size wide matrices (profiles/r05_any_slice_count.txt)
            // -- round 6: the heaviest workgroup's real share (TileCensus): the same term for a uniform matrix, and what makes column slices of a
            // banded matrix as expensive as they are (most of its (row range x slice) blocks are empty)
            // (charged beyond the uniform picture only where the real imbalance exceeds it by more than 15 %: the slice counts of the scrambled
            //  graphs were settled by measurement to within a microsecond -- ogbl-ppa 5 slices, gplus 7 -- and the census rows are coarser than that)
            const double uniform_load = double(nnz) / std::max(1.0, ranges * cs) * std::ceil(blocks_per_wg);
            const double idle_us = double(nnz) * 8.0 / 6.2e6 * ((std::ceil(blocks_per_wg) / std::max(1e-9, blocks_per_wg) - 1.0) +
                                                                 std::max(0.0, real.max_wg_load / std::max(1.0, uniform_load) - 1.15) * uniform_load / std::max(1.0, double(nnz) / G));
            const double cost = volume_us + latency_us + conflict_us + 8.0 * blocks_per_wg + combine_us + idle_us;
            if (in.sw.debug)
                std::fprintf(stderr, "plan cs %u cap %u ring %u: ranges %.0f volume %.1f latency %.1f conflicts %.1f blocks/wg %.2f idle %.2f combine %.1f => %.2f us\n", cs, cap, ring, ranges,
                             volume_us, latency_us, conflict_us, blocks_per_wg, idle_us, combine_us, cost);
            if (cost < p.best) { p.best = cost; p.best_units = real.nonempty_units; p.slices = cs; p.max_rows = cap; }
        }
    }
}

// The format family and the tile plan of the row-block kernels (everything between the SWEEP decision and the row ranges).
// Round 6: the format family and the tile plan are decided TOGETHER where they depend on each other -- a float-mode matrix whose row-block plan
// comes out as ONE column slice of a PAIRS image (ds_add_f64 row sums, 4 095-row blocks) runs 10-30 % faster as an OWNER24 image (owned rows,
// plain read-modify-write on 4-byte sums, 24 561-row blocks) once it is large enough to amortise OWNER's longer prologue: banded 400 K 30.4 ->
// 23.5 us, block-diagonal 200 K 18.6 -> 15.0, 600 K 32.1 -> 22.3, tall 2 M x 50 K 31.1 -> 28.0, 3 M x 8 K 31.2 -> 25.8, in float_pob and
// float_stall alike; sliced plans are a wash (gplus, rmat19, er_300k: +-3 %) and small ones lose (a 4 M-non-zero slab 8.1 -> 9.4 us)
// (profiles/r06_float_pairs_vs_owner24.txt).  So: plan as before; if that gives float / PAIRS-family / one slice / >= kFloatOneSliceOwnerMinNnz
// non-zeros, plan again as OWNER24 and take it.
inline TilePlan plan_row_blocks(const PlanInputs& in, double hub_share, DenseRowChoice dense, bool owner_allowed) {
    const uint32_t num_rows = in.L.num_rows, num_cols = in.L.num_cols, max_workgroups = in.max_workgroups;
    const uint64_t nnz = in.nnz;
    TilePlan p;
    bool keep_delta_for_hubs = false;
    p.format = choose_stream_format(in, hub_share, dense.prefer_sliced_delta, owner_allowed, keep_delta_for_hubs);
    p.light = choose_light(in, dense, p.format);
    for (int attempt = 0; attempt < 2; ++attempt) {
        p.format_forced = in.sw.format_set() || dense.prefer_sliced_delta || (keep_delta_for_hubs && p.format == kFormatDelta);      // (the sliced DELTA plan of a dense-row layer is DELTA for its per-lane row sums, not for its bytes)
        uint32_t light_wgs = kLightWorkgroupsPerCu;
        if (in.sw.light_wgs.set) light_wgs = std::min<uint32_t>(6u, std::max(1, in.sw.light_wgs.value));
        p.G = std::max<uint32_t>(1, max_workgroups) * (p.light ? light_wgs : 1u);
        p.slices = 1;
        p.max_rows = p.light ? kLightMaxBlockRows : max_block_rows(false);
        if (p.light) {
            if (in.sw.max_rows.set) p.max_rows = std::min<uint32_t>(p.max_rows, std::max(1, in.sw.max_rows.value));   // tests: chains of blocks
        } else {
            cost_row_block_plans(in, p);
        }
        // Round 6: below the hyper-sparse border a SWEEP plan can still replace the row-block plan -- where the units are tiny AND the models agree.  A
        // (row range x sub-tile) unit costs the row-block kernel a barrier, a refill and a head record whatever it holds; a matrix of few long rows
        // over millions of columns -- 2048 x 8 M, 2000 per row, mean gap 4000: below every gap rule -- has 131 elements per unit: 67.5 us as the PAIRS
        // image the gap rule gives it, 22.3 us as a SWEEP image (tools/planner_check.py --second).  Both conditions: fewer than 1024 elements per
        // non-empty unit of the chosen plan (the mechanism), and SWEEP's whole modelled step under 60 % of the row-block plan's stream + plan cost
        // (the two models were fitted apart and the row-block one reads 30-80 % high in absolute terms: on their own they would send one rank's slab
        // of mouse_gene -- 14 K elements per unit, 8.3 us as PAIRS, 12.5 as SWEEP -- the wrong way).
        if (attempt == 0 && !p.owner() && !p.light && !p.format_forced && !in.sw.sweep.set && !in.sw.col_slices.set && !in.sw.max_rows.set &&
            nnz >= kSweepMinNnzWide && uint64_t(num_cols) * 4 < (1ull << 32) && p.best < 1e29) {
            uint32_t cs = 1, rows_cap = 0;
            uint64_t want = 1;
            const double sweep_us = sweep_plan(in.L, nnz, max_workgroups, cs, want, rows_cap);
            const double rowblock_us = double(nnz) * 8.0 / 6.2e6 + p.best;
            if (in.sw.debug) std::fprintf(stderr, "format: row-block plan %.1f us (stream + %.1f; %.0f elements per unit) against sweep %.1f us (%u slices)\n", rowblock_us, p.best, double(nnz) / std::max(1.0, p.best_units), sweep_us, cs);
            if (sweep_us < 0.6 * rowblock_us && double(nnz) / std::max(1.0, p.best_units) < 1024.0) {
                p.tiny_unit_sweep = true;
                return p;
            }
        }
        const bool pairs_family = p.format == kFormatPairs || (p.format == kFormatDelta && double(nnz) * 1.6 < double(kDeltaMinSavedBytesFloat));
        if (attempt == 0 && in.is_float && !p.owner() && !p.light && !p.format_forced && owner_allowed && pairs_family && p.slices == 1 && nnz >= kFloatOneSliceOwnerMinNnz &&
            !in.sw.col_slices.set && !in.sw.max_rows.set) {
            if (in.sw.debug) std::fprintf(stderr, "format: float mode, one-slice PAIRS-family plan of %llu non-zeros -> planned again as OWNER24\n", (unsigned long long)nnz);
            p.format = kFormatOwner24;
            continue;
        }
        break;
    }
    if (uint64_t(p.slices) * num_rows > 0xffffffffull) {   // Block::out_offset = slice * num_rows + row0 is a 32-bit word offset
        while (p.slices > 1 && uint64_t(p.slices) * num_rows > 0xffffffffull) p.slices /= 2;
        p.max_rows = p.owner() ? owner_max_block_rows(2) : p.slices > 1 ? max_block_rows(true) : max_block_rows(false);
    }
    return p;
}

// ---- the decisions taken after the sort, when every unit's slots / shares are known --------------------------------------------------

// DELTA or PAIRS, now that every unit's slots are known (automatic choice only):
//  * DELTA pays for every position gap beyond 16 bits with a bridge slot.  A graph whose gaps are heavy-tailed (R-MAT: a quarter
//    of the rows empty, hubs of 10^5 non-zeros) needs one for every 25th element although its MEAN gap looks fine: 4 % more slots
//    and still 11 % fewer bytes than PAIRS (58.5-58.9 us against 59.4-59.8; what made it 82-85 us through round 4 was the dealing of
//    the runs, see first_slot in stream_tiles.cpp: lay_out_streams, not the bridges).  More than 5 % bridge slots -> PAIRS.
//  * DELTA's 6-byte slots only pay when the stream is what bounds the kernel.  Measured over 20 shapes (tools/probe_synth.py,
//    40000^2 and 400000 x 100000 power-law matrices at mean gaps 16 ... 4096, ogbl-ppa, mouse_gene):
//    t(DELTA) - t(PAIRS) = (bytes saved) / 6.5 TB/s - c with c = 3.5 us fixed point, 6 us float (more instructions per element,
//    a head record per unit and wavefront).  So: DELTA only when it saves more than kDeltaMinSavedBytes of stream.
// (DELTA is priced at its PLAIN 768-byte record here, deliberately, also where the image will be packed into 640-byte records (stream_tiles.h:
// kRecordBytes24): the constants above were fitted on plain images, and a matrix whose plain DELTA image misses the saving but whose packed one would
// clear it -- a PAIRS image of 115 ... 140 MB -- has not been measured as a packed image against PAIRS.  Such a matrix stays PAIRS.)
// Returns kFormatDelta or kFormatPairs for a tentative DELTA plan of `num_blocks` blocks.
inline StreamFormat delta_or_pairs(const std::vector<UnitPlan>& plans, uint32_t num_blocks, uint64_t nnz, bool is_float) {
    uint64_t slots = 0, pairs_bytes = 0, delta_bytes = 0;
    for (const UnitPlan& up : plans) {
        slots += up.slots;
        const uint64_t pairs_chunks = (uint64_t(up.n) + kWaveLanes - 1) / kWaveLanes, records = (up.slots + kWaveLanes - 1) / kWaveLanes;
        pairs_bytes += pairs_chunks * kChunkBytes;
        // slots + one head per wavefront with work, in records of two slots (a run's last record is half empty every other time)
        delta_bytes += (records + std::min<uint64_t>(records, kConsumerWaves) * 3 / 2) * (kRecordBytes / 2);
    }
    // (the fixed cost c is mostly the head record per unit and wavefront: 14 units per block -> 3.5 us, but a sliced plan with one or two
    // units per block pays ~1.2 us -- gplus in 7 slices: 24 MB saved, 24.7 us in PAIRS, 21.9 in DELTA.  Fixed point only: measured there.)
    const double units_per_block = double(plans.size()) / std::max<uint32_t>(1, num_blocks);
    const uint64_t min_saved = is_float ? kDeltaMinSavedBytesFloat
                                        : std::min<uint64_t>(kDeltaMinSavedBytes, uint64_t((1.0 + 0.18 * units_per_block) * 6.5e6));
    return (double(slots) > 1.05 * double(nnz) || pairs_bytes < delta_bytes + min_saved) ? kFormatPairs : kFormatDelta;
}

// OWNER24 holds a share's rows relative to its first row in 11 bits and a wavefront's step count in 16: otherwise, or when
// the row cap has cut so many shares short that the 7-byte records are no smaller than 8-byte chunks, keep the 8-byte form
struct Owner24Fit { bool fits, smaller; };      // (smaller: only meaningful where it fits)
inline Owner24Fit owner24_fit(const std::vector<Block>& blocks, const std::vector<UnitPlan>& plans) {
    bool fits = true;
    uint64_t bytes24 = 0, bytes32 = 0;
    for (size_t bi = 0; bi < blocks.size() && fits; ++bi) {
        uint64_t steps[kConsumerWaves] = {0};
        for (uint32_t u = blocks[bi].unit_begin; u < blocks[bi].unit_end; ++u) {
            const UnitPlan& up = plans[u];
            bytes32 += (uint64_t(up.n) + kWaveLanes - 1) / kWaveLanes * kChunkBytes;
            for (uint32_t w = 0; w < kConsumerWaves; ++w) {
                steps[w] += (up.own_begin[w + 1] - up.own_begin[w] + kWaveLanes - 1) / kWaveLanes;
                if (up.own_last[w] - up.own_row[w] >= kOwnerShareRows || up.own_row[w] > 0xffffu) fits = false;
            }
        }
        for (uint32_t w = 0; w < kConsumerWaves; ++w) {
            if (steps[w] > kOwnerStepMask) fits = false;
            bytes24 += (steps[w] + kOwnerRecordSteps - 1) / kOwnerRecordSteps * kOwnerRecordBytes;
        }
    }
    return {fits, !(double(bytes24) > 0.97 * double(bytes32))};
}

// ---- PAIRS with 24-bit position words (stream_tiles.h: PAIRS24): 7 bytes per element where 11 bits of row are enough ----------
// Opt-in (HISPARSE_AUX_BITS=24): measured SLOWER than the 8-byte form although it streams 12 % fewer bytes (mouse_gene 40.8 vs
// 39.7 us): a step becomes two loads (one of them unaligned) instead of one dwordx2, and the kernels are bound by the number of
// memory requests a CU keeps in flight, not by the bytes.
// (taken last: the plan's format is final here, and the row ranges are cut)
inline bool wants_pairs24(const TilePlan& p, const PlanSwitches& sw, uint32_t max_block_rows) {
    return sw.aux24 && !p.owner() && !p.delta() && !p.light && max_block_rows <= kAux24MaxRows;
}

}  // namespace detail
}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_STREAM_PLAN_H_
