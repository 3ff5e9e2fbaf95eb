// hs_context.h — the context behind the C-ABI of include/hisparse_hip.h, shared by its implementation files:
//   hs_api.cpp     create / destroy, options, stream and binding hooks, enqueue, run / batch / partition / feedback / iterate, sync / read, timing
//   hs_load.cpp    hs_load_matrix, hs_load_matrix_csr, hs_load_matrix_csr_transposed (+ autotune), hs_update_values, the debug reads
//   hs_spmspv.cpp  the SpMSpV extension          hs_spmm.cpp  the SpMM extension
// One context owns one HIP device, one stream and the device-resident data.  There is no CPU fallback anywhere in these files: without a
// usable gfx950 device every call fails.
#ifndef HISPARSE_HS_CONTEXT_H_
#define HISPARSE_HS_CONTEXT_H_

#include "hisparse_hip.h"

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "device_buffer.h"      // DeviceBuffer, PinnedBuffer, DeviceEvent: the owners of device memory, pinned memory, events
#include "hisparse/common.h"
#include "reuse_tracker.h"
#include "spmv_kernels.h"
#include "stream_tiles.h"
#include "tiles_common.h"

// The host side of the carried combine pass (the device side: spmv_device.h, hisparse::dev::CarriedCombine).
// Column-sliced plans, hs_run after hs_run on the library's own stream: the combine pass of a step is CARRIED into the SpMV kernel of the
// next one.  This class owns everything that takes: the partial vectors (one set, or two when the plan carries), which set's sum has not
// been written to its y yet (the debt) and the turn counter.  A step either goes through step(), which pays the previous debt inside its
// own launch and leaves a new one, or runs after settle(), the stand-alone combine for what is owed.  Every entry point that could observe
// y, its target or the stream settles first (enter, below), so the stream-order contract of hisparse_hip.h holds unchanged.
class CarriedCombine {
public:
    // At load: partial vectors for `col_slices` > 1 slices of `num_rows` words, twice when the plan carries.  reset() alone: no matrix.
    void reset() { *this = CarriedCombine(); }
    hipError_t reset(bool is_float, uint32_t num_rows, uint32_t num_cols, uint32_t col_slices, bool carries) {
        reset();
        if (col_slices <= 1) return hipSuccess;
        const hipError_t e = partial_.alloc(size_t(carries ? 2 : 1) * col_slices * num_rows * 4);
        if (e != hipSuccess) return e;
        is_float_ = is_float;
        rows_ = num_rows;
        cols_ = num_cols;
        slices_ = col_slices;
        carries_ = carries;
        return hipSuccess;
    }

    bool carries() const { return carries_; }
    uint32_t* partial() const { return partial_.get(); }      // where a step that does not carry writes its partial rows

    // May this step leave its sum owed?  `plain_whole_step`: every row partition, no events around the kernel, no feedback;
    // `stream_private`: the library's own stream with no handle given out, or inside hs_run_batch.
    // x [num_cols words) must share no memory with a result vector [num_rows words): the carried combine writes y(k) from inside step k+1's
    // kernel while other workgroups of that kernel read x -- in-place y = A*y stays well defined only with the stand-alone combine.
    bool eligible(bool plain_whole_step, bool stream_private, const uint32_t* x, const uint32_t* y) const {
        return carries_ && plain_whole_step && stream_private && !aliases(x, y) && !(owed_ >= 0 && aliases(x, owed_y_));
    }

    // One eligible step: its partial rows go to the set the previous step did NOT use; the previous step's are added up by this launch's
    // workgroups before they start on their blocks; this step's own sum is owed to `y` until the next step() or settle().
    hipError_t step(hisparse::dev::SpmvLaunch& a, uint32_t* y, hipStream_t stream) {
        const uint32_t b = turn_++ & 1u;
        const size_t set = size_t(slices_) * rows_;
        a.out = partial_.get() + b * set;
        if (owed_ >= 0) {
            a.carry_partial = partial_.get() + size_t(owed_) * set;
            a.carry_y = owed_y_;
            a.carry_rows = rows_;
            a.carry_slices = slices_;
        }
        const hipError_t e = hisparse::dev::launch_spmv(is_float_, a, stream);
        if (e != hipSuccess) return e;
        owed_ = int(b);
        owed_y_ = y;
        return hipSuccess;
    }

    // The sum of the last carried step, if any, goes to its y now (one combine_slices_kernel launch); nothing is owed afterwards.
    hipError_t settle(hipStream_t stream) {
        if (owed_ < 0) return hipSuccess;
        const uint32_t* partial = partial_.get() + size_t(owed_) * slices_ * rows_;
        owed_ = -1;
        return hisparse::dev::launch_combine_slices(is_float_, partial, owed_y_, rows_, slices_, 0, rows_, stream);
    }

    // The recorded debt does not exist on the device: the steps were captured into a graph that is dropped, or a launch among them failed.
    void forget() { owed_ = -1; }

private:
    bool aliases(const uint32_t* x, const uint32_t* y) const {
        if (!x || !y) return false;
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), x1 = x0 + size_t(cols_) * 4, y0 = reinterpret_cast<uintptr_t>(y), y1 = y0 + size_t(rows_) * 4;
        return x0 < y1 && y0 < x1;
    }

    DeviceBuffer<uint32_t> partial_;      // col_slices > 1: per-slice partial results, col_slices x num_rows words per set
    bool is_float_ = false, carries_ = false;
    uint32_t rows_ = 0, cols_ = 0, slices_ = 1;
    int owed_ = -1;                       // the set whose sum has not been written yet, or -1
    uint32_t* owed_y_ = nullptr;
    uint32_t turn_ = 0;
};

// What belongs to the loaded matrix.  An empty value = no matrix: free_matrix assigns one.
struct MatrixData {
    bool loaded = false;
    uint32_t num_rows = 0, num_cols = 0, row_parts = 0;
    DeviceBuffer<uint8_t> image;
    DeviceBuffer<hisparse::dev::Block> blocks;
    DeviceBuffer<hisparse::dev::Unit> units;
    DeviceBuffer<uint32_t> part_heads;
    hisparse::dev::SpmvLaunch launch{};   // the plan as launch_spmv takes it (the pointers above, format, LDS bytes, ...): a step adds x, out, its row-partition filter
                                          // and its stream cache policy (below)
    // The stream cache policy is a launch's, not the load's (hs_api.cpp: launch_args; reuse_tracker.h): what the device's tracker knows this image by --
    // an id no other load has had, fresh again after hs_update_values -- and what the load contributes: the caller's stream_resident option (0 | 1;
    // -1: none) and whether the image's shape may be streamed resident at all (stream_tiles.h: plan_stream_resident).
    uint64_t image_id = 0, image_bytes = 0;
    int resident_forced = -1;
    bool resident_eligible = false;
    uint32_t col_slices = 1;
    bool crossing_blocks = false;   // some row block reaches over a row-partition border (tiles_common.h: Layout::cross_parts)
    uint32_t max_block_rows = 0;
    DeviceBuffer<uint32_t> y;       // library-owned packed y
    DeviceBuffer<uint32_t> partition_y;   // hs_run_partition on a one-slice plan with crossing blocks: the kernel writes here (num_rows words,
                                          // allocated on first use), the partition's own rows are then copied into y
    // SpMM over a SWEEP image planned for it (spmm_sweep.hip; option spmm_vectors = 4): X interleaved [column][4], the four result columns
    // (per column slice) before the combine pass, and after it
    uint32_t spmm_vectors = 1;
    DeviceBuffer<uint32_t> spmm_x4, spmm_partial, spmm_y;
    DeviceBuffer<uint32_t> x_interleaved;   // fused SpMM over a BITMAP image: 4 columns of X as [column][vector] words (allocated on first use)
    // SpMM on the matrix engine (float BITMAP matrices): the second image + scratch (spmm_mfma.hip).  Optional: an empty value = no second image.
    struct Mfma {
        DeviceBuffer<uint32_t> words;
        hisparse::dev::MfmaImage info;    // geometry and words_bytes only (its host and device `words` stay empty)
        DeviceBuffer<uint32_t> x;
        DeviceBuffer<float> partial;
        DeviceBuffer<uint32_t> flag;
        DeviceBuffer<uint32_t> value_map;   // hs_update_values: as `value_map` below, into `words`
    } mfma;
    // hs_update_values (option value_map, CSR loads built on the device): per non-zero in CSR order, the u32 word index of its value in
    // `image`; a staging buffer for values handed in from the host (allocated on first use); why there is no map
    DeviceBuffer<uint32_t> value_map;
    uint64_t value_map_nnz = 0;
    DeviceBuffer<float> value_stage;
    std::string value_map_why = "no matrix has been loaded";
};

// What belongs to the CSC load of the SpMSpV extension (hs_load_matrix_csc): the matrix once more, in CSC form, + scratch.
struct CscData {
    DeviceBuffer<uint32_t> indptr, rows, vals;
    DeviceBuffer<uint32_t> keys, products, bin_base, cursors, overflow;   // the product list (spmv_kernels.h: SpmspvScratch) and its counters
    uint64_t capacity = 0;
    hisparse::dev::SpmspvScratch scratch() const {
        return {keys.get(), products.get(), bin_base.get(), cursors.get(), overflow.get(), capacity};
    }
    std::vector<uint32_t> col_len;                 // host copy of the column lengths: splits a host-side x whose products exceed the list
    DeviceBuffer<uint32_t> y;                      // max(csc rows, the dense matrix's padded rows) words
    uint32_t y_words = 0;
    PinnedBuffer<hisparse::dev::hs_idx_val_dev> h_sx;   // hs_spmspv: pinned, mapped staging of the caller's IDX_VAL_T pairs (two halves of sx_capacity entries, used in turn) ...
    hisparse::dev::hs_idx_val_dev* d_sx = nullptr;      // ... = the same memory as the device sees it
    DeviceEvent sx_read[2];                        // half h's kernels have read it: the host may write it again
    uint32_t sx_turn = 0;
    std::vector<uint8_t> sx_seen;                  // one bit per column, all zero between calls (the repeat check of hs_spmspv)
    uint32_t sx_capacity = 0;
    DeviceBuffer<uint32_t> x_dense;                // dense dispatch: x scattered into a zero vector (num_cols words)
    uint32_t num_rows = 0, num_cols = 0;
};

struct hs_context {
    hisparse::dev::detail::OptionMap options;    // hs_set_option: "HISPARSE_<KEY>" -> value
    int device = -1;
    int impl = 0;
    hisparse::Geometry geom;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int compute_units = 0;
    bool in_batch = false;          // inside hs_run_batch: the batch settles its own last step before it returns, whatever stream it runs on
    bool stream_shared = false;     // hs_get_stream was called: somebody else may order work against the stream -- every step completes in itself

    MatrixData mat;
    CarriedCombine carry;
    CscData csc;
    uint32_t mfma_call = 0;                        // launch_spmm_mfma wants a number no earlier call on this context has used
    double dense_spmv_us = 0.0;                    // the dense SpMV of the loaded matrix, timed once (hs_spmspv's dispatch rule); 0: not yet
    uint64_t spmspv_dense_dispatches = 0;          // calls of hs_spmspv answered by the dense SpMV (hs_get_stats does not carry it: tests read it through hs_last_error)

    // hs_run_batch with `batch_graph`: the captured step sequence, kept while nothing it bakes in changes
    hipGraph_t batch_graph = nullptr;
    hipGraphExec_t batch_exec = nullptr;
    uint32_t batch_steps = 0;
    const void* batch_x = nullptr;
    void* batch_y = nullptr;
    hipStream_t batch_stream = nullptr;

    // The device's reuse tracker (one per device, shared by its contexts), and the copy of its state that launches decide on while this context
    // captures its stream (hs_run_batch with batch_graph, hs_iterate with iterate_graph): captured launches execute later, once per replay
    hisparse::ReuseTracker* reuse = nullptr;
    hisparse::ReuseList capture_list;
    bool capturing = false;

    bool vector_loaded = false;
    DeviceBuffer<uint32_t> d_x;    // library-owned packed x
    const uint32_t* x_bound = nullptr;
    uint32_t* y_bound = nullptr;
    uint32_t x_capacity = 0;
    uint32_t x_len = 0;            // words of the vector last given to hs_load_vector

    hs_stats stats{};
    std::string error;

    bool is_float() const { return impl != HS_IMPL_FIXED; }
    bool stream_private() const { return stream == own_stream && !stream_shared; }
    uint32_t* y_target() const { return y_bound ? y_bound : mat.y.get(); }
    const uint32_t* x_source() const { return x_bound ? x_bound : d_x.get(); }
};

int fail(hs_context* ctx, int code, const std::string& msg);      // records msg for hs_last_error (ctx == nullptr: the creating thread's), returns code
int hip_fail(hs_context* ctx, hipError_t e, const char* what);
#define HS_HIP(ctx, call)                                       \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #call);  \
    } while (0)

// a call-time switch of this context: hs_set_option first, the environment as the fallback for tools
inline const char* ctx_option(const hs_context* c, const char* name) { return hisparse::dev::detail::option_lookup(&c->options, name); }

// The way into an entry point: what the call needs, checked in this order -- a context (and its indispensable pointer arguments:
// `have_args`, reported as "null argument"), a loaded matrix, a vector for it, a CSC matrix -- then the context's device is made current
// and an owed combine pass is settled (CarriedCombine above).  kNoSettle: this call carries on from the caller's last step, or settles at
// a later point of its own; kHostOnly: the checks alone.  A call that validates arguments between the checks and its device work enters
// twice -- kHostOnly first, then for the device and the settle -- so that a rejected call launches nothing.
enum : unsigned { kMatrix = 1u, kVector = 2u, kReady = kMatrix | kVector, kCsc = 4u, kNoSettle = 8u, kHostOnly = 16u | kNoSettle };
int enter(hs_context* ctx, unsigned need);
int enter(hs_context* ctx, unsigned need, bool have_args);
int settle(hs_context* ctx);      // the stand-alone combine for what is owed, on the context's stream

// Enqueue one SpMV y = A x (filter < 0) or one row partition of it; optional events bracket the kernel.  `feedback` (hs_iterate): also
// x = scale (*) y (+) shift afterwards -- folded into the combine launch of a column-sliced matrix, its own launch otherwise.
struct Feedback { uint32_t scale, shift; };
int enqueue(hs_context* c, const uint32_t* x, uint32_t* y, int32_t filter, hipEvent_t k0, hipEvent_t k1, const Feedback* feedback = nullptr);
// `steps` whole SpMVs on vectors that are not the context's own, step i on x + i * ldx and y + i * ldy: no sum is left owed to them on any path
int run_steps(hs_context* c, const uint32_t* x, uint64_t ldx, uint32_t* y, uint64_t ldy, uint32_t steps);
// `warm` steps, then the best of `regions` regions of `runs` steps each, every region settled before its closing event: microseconds per
// step in *us, <= 0 when no time could be taken.  Nothing is owed to y afterwards.
int time_steps(hs_context* c, const uint32_t* x, uint32_t* y, int warm, int regions, int runs, double* us);

void drop_batch_graph(hs_context* c);
void free_matrix(hs_context* c);

#endif  // HISPARSE_HS_CONTEXT_H_
