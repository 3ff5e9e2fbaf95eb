// hs_api.cpp — implementation of the drop-in C-ABI (include/hisparse_hip.h) on the HIP runtime: the context's life, options, stream and
// binding hooks, and the SpMV itself.  Loads are in hs_load.cpp, the SpMSpV and SpMM extensions in hs_spmspv.cpp and hs_spmm.cpp.
//
// The reference reaches its device through OpenCL/XRT objects created in sw/benchmark.cpp:228-298 and
// launches five kernels per row partition (:318-338).  Here one context owns one HIP device, one
// stream and the device-resident data; hs_run launches the whole SpMV (all row partitions) as ONE
// kernel, spmv_rowblock_kernel<fixed|float>, which writes the packed y directly.
#include "hs_context.h"

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "gpu_tiles.h"

namespace {

thread_local std::string g_create_error;

// hs_set_option's keys (the HISPARSE_<KEY> environment switches the library understands); plan-time ones take effect at the next load
const char* const kOptionKeys[] = {
    "STREAM_FORMAT", "COL_SLICES", "MAX_ROWS", "CROSS_PARTITIONS", "SPMM_VECTORS", "ROW_RUNS", "AUX_BITS", "XCD_AFFINITY", "STREAM_RESIDENT", "RETILE", "PLAN_DEBUG",
    "BITMAP_SKEW", "BITMAP_X_LDS", "BITMAP_BUILD", "WALK_LANES", "NO_MFMA_IMAGE", "MFMA_CHUNK", "LIGHT", "LIGHT_WGS", "SWEEP",
    "DELTA_DEAL", "POW2_SLICES", "SPMM_FUSED", "SPMM_MFMA", "SPMSPV", "SPMSPV_CROSSOVER", "ITERATE_GRAPH", "BATCH_GRAPH", "CARRY_COMBINE", "AUTOTUNE", "PLAN_CENSUS",
    "VALUE_MAP",
};

static_assert(hisparse::dev::kRowblockResidentMaxImageBytes == hisparse::dev::kResidentMaxImageBytes, "one cache, one budget for the reuse tracker");

// The stream cache policy of ONE launch (reuse_tracker.h): `sc1` when the caller's option says so, or when no option is set, the image's shape is
// eligible and the device's tracker finds it warm -- the images launched since its previous launch, itself included, streamed no more than the
// Infinity Cache holds.  Every launch is recorded, of every format and under either policy; a row partition counts as its whole image (its bytes
// were last read one partition loop ago).  While the stream is capturing, nothing executes: the decision is taken on a copy of the tracker's state
// -- this context's own captures keep one copy from step to step, so a captured batch from a cold state is `nt` for step 1 and resident for the
// rest, and touch the tracker once per replay (replayed); a caller's capture of a stream it owns, whose replays the library does not see, decides
// each launch on a fresh copy.
bool launch_stream_resident(hs_context* c) {
    const MatrixData& m = c->mat;
    const uint64_t budget = hisparse::dev::kResidentMaxImageBytes;
    if (c->capturing) return hisparse::launch_resident(c->capture_list, m.resident_forced, m.resident_eligible, m.image_id, m.image_bytes, budget);
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (c->stream != c->own_stream && hipStreamIsCapturing(c->stream, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone) {
        hisparse::ReuseList copy = c->reuse->snapshot();
        return hisparse::launch_resident(copy, m.resident_forced, m.resident_eligible, m.image_id, m.image_bytes, budget);
    }
    return c->reuse->launch_resident(m.resident_forced, m.resident_eligible, m.image_id, m.image_bytes, budget);
}

// This context captures its own launches from here to the end of the scope
struct CaptureScope {
    hs_context* c;
    explicit CaptureScope(hs_context* ctx) : c(ctx) {
        c->capture_list = c->reuse->snapshot();
        c->capturing = true;
    }
    ~CaptureScope() { c->capturing = false; }
};
// one replay of a captured graph ran the loaded image
void replayed(hs_context* c) { c->reuse->touch(c->mat.image_id, c->mat.image_bytes); }

hisparse::dev::SpmvLaunch launch_args(hs_context* c, const uint32_t* x, uint32_t* y, int32_t filter) {
    hisparse::dev::SpmvLaunch a = c->mat.launch;
    a.x = x;
    a.out = c->mat.col_slices > 1 ? c->carry.partial() : y;
    a.row_part_filter = filter;
    a.stream_resident = launch_stream_resident(c);
    return a;
}

// rows [lo, hi) of row partition j
void partition_rows(const hs_context* c, uint32_t j, uint32_t& lo, uint32_t& hi) {
    const uint64_t a = uint64_t(j) * c->geom.logical_ob;
    const uint64_t b = std::min<uint64_t>(a + c->geom.logical_ob, c->mat.num_rows);
    lo = uint32_t(a);
    hi = uint32_t(b);
}

int step(hs_context* c, int32_t filter = -1, const Feedback* feedback = nullptr) { return enqueue(c, c->x_source(), c->y_target(), filter, nullptr, nullptr, feedback); }

}  // namespace

int fail(hs_context* ctx, int code, const std::string& msg) {
    if (ctx) ctx->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hs_context* ctx, hipError_t e, const char* what) {
    return fail(ctx, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int settle(hs_context* c) {
    const hipError_t e = c->carry.settle(c->stream);
    return e == hipSuccess ? HS_OK : hip_fail(c, e, "combine_slices_kernel");
}

int enter(hs_context* ctx, unsigned need) {
    if (!ctx) return HS_ERR_BAD_ARG;
    if ((need & kMatrix) && !ctx->mat.loaded) return fail(ctx, HS_ERR_NOT_LOADED, "hs_load_matrix has not been called");
    if (need & kVector) {
        if (!ctx->vector_loaded && !ctx->x_bound) return fail(ctx, HS_ERR_NOT_LOADED, "hs_load_vector has not been called");
        if (!ctx->x_bound && ctx->x_len != ctx->mat.num_cols)
            return fail(ctx, HS_ERR_NOT_LOADED, "the loaded vector does not have this matrix's padded column count: call hs_load_vector again");
    }
    if ((need & kCsc) && !ctx->csc.indptr) return fail(ctx, HS_ERR_NOT_LOADED, "hs_load_matrix_csc has not been called");
    if ((need & kHostOnly) == kHostOnly) return HS_OK;
    HS_HIP(ctx, hipSetDevice(ctx->device));
    return (need & kNoSettle) ? HS_OK : settle(ctx);
}
int enter(hs_context* ctx, unsigned need, bool have_args) {
    if (!ctx || !have_args) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    return enter(ctx, need);
}

void drop_batch_graph(hs_context* c) {
    if (c->batch_exec) (void)hipGraphExecDestroy(c->batch_exec);
    if (c->batch_graph) (void)hipGraphDestroy(c->batch_graph);
    c->batch_exec = nullptr;
    c->batch_graph = nullptr;
    c->batch_steps = 0;
}

void free_matrix(hs_context* c) {
    drop_batch_graph(c);
    c->mat = MatrixData();
    c->carry.reset();
    c->y_bound = nullptr;
}

int enqueue(hs_context* c, const uint32_t* x, uint32_t* y, int32_t filter, hipEvent_t k0, hipEvent_t k1, const Feedback* feedback) {
    if (const char* why = hisparse::dev::profiling_switch_error()) return fail(c, HS_ERR_BAD_ARG, why);
    MatrixData& m = c->mat;
    if (c->carry.eligible(filter < 0 && !k0 && !k1 && !feedback, c->stream_private() || c->in_batch, x, y)) {
        hisparse::dev::SpmvLaunch a = launch_args(c, x, y, filter);
        HS_HIP(c, c->carry.step(a, y, c->stream));
        return HS_OK;
    }
    if (int rc = settle(c)) return rc;
    hisparse::dev::SpmvLaunch args = launch_args(c, x, y, filter);
    // One partition of a plan whose row blocks reach over partition borders: the blocks that intersect the partition run (Block::next_part)
    // and compute rows of its neighbours too.  "Rows of other partitions keep their previous contents" (hisparse_hip.h): a column-sliced
    // plan combines the partition's rows only (below); a one-slice plan writes to a side buffer and the partition's rows are copied over.
    const bool side_y = filter >= 0 && m.crossing_blocks && m.col_slices == 1;
    if (side_y) {
        if (!m.partition_y) HS_HIP(c, m.partition_y.alloc(size_t(m.num_rows) * 4));
        args.out = m.partition_y.get();
    }
    if (k0) HS_HIP(c, hipEventRecord(k0, c->stream));
    HS_HIP(c, hisparse::dev::launch_spmv(c->is_float(), args, c->stream));
    if (k1) HS_HIP(c, hipEventRecord(k1, c->stream));
    if (side_y) {
        uint32_t lo = 0, hi = 0;
        partition_rows(c, uint32_t(filter), lo, hi);
        HS_HIP(c, hipMemcpyAsync(y + lo, m.partition_y.get() + lo, size_t(hi - lo) * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    uint32_t* x_fb = const_cast<uint32_t*>(x);
    const uint32_t n_fb = std::min(m.num_rows, m.num_cols);
    if (m.col_slices > 1) {
        uint32_t lo = 0, hi = m.num_rows;
        if (filter >= 0) partition_rows(c, uint32_t(filter), lo, hi);
        HS_HIP(c, hisparse::dev::launch_combine_slices(c->is_float(), c->carry.partial(), y, m.num_rows, m.col_slices, lo, hi, c->stream,
                                                       feedback ? x_fb : nullptr, n_fb, feedback ? feedback->scale : 0, feedback ? feedback->shift : 0));
    } else if (feedback) {
        HS_HIP(c, hisparse::dev::launch_feedback(c->is_float(), y, x_fb, n_fb, feedback->scale, feedback->shift, c->stream));
    }
    return HS_OK;
}

int run_steps(hs_context* c, const uint32_t* x, uint64_t ldx, uint32_t* y, uint64_t ldy, uint32_t steps) {
    int rc = HS_OK;
    for (uint32_t i = 0; i < steps && rc == HS_OK; ++i) rc = enqueue(c, x + size_t(i) * ldx, y + size_t(i) * ldy, -1, nullptr, nullptr);
    // never leave a sum owed to a transient target: an event or a device-wide synchronisation then completes y, and its owner may free it
    if (rc == HS_OK) return settle(c);
    c->carry.forget();
    return rc;
}

int time_steps(hs_context* c, const uint32_t* x, uint32_t* y, int warm, int regions, int runs, double* us) {
    *us = -1.0;
    DeviceEvent t0, t1;
    if (t0.create() != hipSuccess || t1.create() != hipSuccess) return HS_OK;
    int rc = HS_OK;
    for (int i = 0; i < warm && rc == HS_OK; ++i) rc = enqueue(c, x, y, -1, nullptr, nullptr);
    for (int rep = 0; rep < regions && rc == HS_OK; ++rep) {
        (void)hipEventRecord(t0.get(), c->stream);
        for (int i = 0; i < runs && rc == HS_OK; ++i) rc = enqueue(c, x, y, -1, nullptr, nullptr);
        // a carried plan owes the last step's sum to y here: it belongs to the region, and whatever the caller enqueues next must not be
        // overwritten by it afterwards
        if (rc == HS_OK) rc = settle(c);
        (void)hipEventRecord(t1.get(), c->stream);
        float ms = 0.0f;
        if (rc == HS_OK && hipEventSynchronize(t1.get()) == hipSuccess && hipEventElapsedTime(&ms, t0.get(), t1.get()) == hipSuccess) {
            const double one = double(ms) * 1000.0 / runs;
            *us = *us < 0.0 ? one : std::min(*us, one);
        }
    }
    if (rc != HS_OK) {
        c->carry.forget();
        *us = -1.0;
    }
    return rc;
}

extern "C" {

const char* hs_strerror(int code) {
    switch (code) {
        case HS_OK: return "ok";
        case HS_ERR_BAD_ARG: return "bad argument";
        case HS_ERR_NO_DEVICE: return "no usable gfx950 device";
        case HS_ERR_HIP: return "HIP runtime error";
        case HS_ERR_BAD_MATRIX: return "channel buffers are not a valid CPSR image";
        case HS_ERR_NOT_LOADED: return "matrix or vector not loaded";
        case HS_ERR_UNSUPPORTED: return "unsupported configuration";
        case HS_ERR_NO_MEMORY: return "out of memory";
        default: return "unknown error";
    }
}

const char* hs_last_error(const hs_context* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int hs_create(hs_context** out, int device_id, int impl, uint32_t ob_bank, uint32_t vb_bank) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null context pointer");
    *out = nullptr;
    if (!hisparse::impl_valid(impl)) return fail(nullptr, HS_ERR_BAD_ARG, "impl must be 0 (fixed), 1 (float_pob) or 2 (float_stall)");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hs_context* c = new (std::nothrow) hs_context;
    if (!c) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    c->device = device_id;
    c->reuse = &hisparse::reuse_tracker_for(device_id);
    c->impl = impl;
    c->geom = hisparse::make_geometry(impl, ob_bank ? ob_bank : hisparse::impl_default_ob_bank(impl),
                                      vb_bank ? vb_bank : hisparse::impl_default_vb_bank(impl));
    c->compute_units = prop.multiProcessorCount;
    if (c->geom.logical_ob > 0xffffffffull || c->geom.logical_vb > 0xffffffffull || c->geom.logical_ob % c->geom.row_divisor != 0) {
        delete c;
        return fail(nullptr, HS_ERR_BAD_ARG, "ob_bank must make 128*ob_bank a multiple of 128*interleave; bank sizes must fit 32 bits");
    }
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return hip_fail(nullptr, e, "hipSetDevice/hipStreamCreate");
    }
    c->stream = c->own_stream;
    // "program the device" here, not inside the first hs_load_matrix: the code objects load on first use, and the dynamic-LDS cap
    // is a property of the FUNCTION (always the full 160 KiB, so that no context can lower it under another one's launches)
    if ((e = hisparse::dev::configure_spmv_kernels(hisparse::dev::kMaxLdsBytes)) != hipSuccess || (e = hisparse::dev::warm_gpu_tiler()) != hipSuccess) {
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        return hip_fail(nullptr, e, "loading the gfx950 kernels");
    }
    // ... and the runtime's one-time set-up of its pageable-copy paths (7 ms in the first copy of a process, whatever its size:
    // tools/h2d_bench.cpp), once per process
    static std::once_flag copy_paths;
    std::call_once(copy_paths, [c] {
        std::vector<uint8_t> host(4 << 20, 0);
        DeviceBuffer<uint8_t> dev;
        if (dev.alloc(host.size()) != hipSuccess) return;
        (void)hipMemcpy(dev.get(), host.data(), host.size(), hipMemcpyHostToDevice);
        (void)hipMemcpy(host.data(), dev.get(), host.size(), hipMemcpyDeviceToHost);
        (void)hipMemcpyAsync(dev.get(), host.data(), host.size(), hipMemcpyHostToDevice, c->own_stream);      // the stream-ordered variants
        (void)hipMemcpyAsync(host.data(), dev.get(), host.size(), hipMemcpyDeviceToHost, c->own_stream);      // have their own set-up
        (void)hipStreamSynchronize(c->own_stream);
    });
    *out = c;
    return HS_OK;
}

int hs_destroy(hs_context* ctx) {
    if (!ctx) return HS_OK;
    (void)hipSetDevice(ctx->device);
    // only the library's own stream is known to be alive here; a caller-owned stream (hs_set_stream) must have been
    // synchronised by its owner before the context is destroyed (hisparse_hip.h)
    if (ctx->stream == ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    else (void)hipDeviceSynchronize();
    free_matrix(ctx);
    ctx->csc = CscData();
    ctx->d_x.reset();
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return HS_OK;
}

int hs_load_vector(hs_context* ctx, const void* packed_x, uint32_t num_cols) {
    if (!ctx || !packed_x) return fail(ctx, HS_ERR_BAD_ARG, "null argument");
    if (ctx->mat.loaded && num_cols != ctx->mat.num_cols) return fail(ctx, HS_ERR_BAD_ARG, "vector length must equal the padded column count");
    if (int rc = enter(ctx, kNoSettle)) return rc;
    if (num_cols > ctx->x_capacity) {
        HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->x_capacity = 0;
        HS_HIP(ctx, ctx->d_x.alloc(size_t(num_cols) * 4 + 64));
        ctx->x_capacity = num_cols;
    }
    HS_HIP(ctx, hipMemcpyAsync(ctx->d_x.get(), packed_x, size_t(num_cols) * 4, hipMemcpyHostToDevice, ctx->stream));
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller may reuse packed_x immediately
    ctx->vector_loaded = true;
    ctx->x_len = num_cols;
    return HS_OK;
}

int hs_run(hs_context* ctx) {
    if (int rc = enter(ctx, kReady | kNoSettle)) return rc;      // (a carried plan: this step's kernel settles the last one's sum)
    return step(ctx);
}

int hs_run_batch(hs_context* ctx, uint32_t steps) {
    int rc = enter(ctx, kReady | kNoSettle | (steps ? 0u : kHostOnly));
    if (rc != HS_OK || steps == 0) return rc;
    const char* opt = ctx_option(ctx, "HISPARSE_BATCH_GRAPH");
    // A batch is one unit in stream order: inside it the steps carry each other's combine pass (enqueue), and the last step's is launched
    // before the call returns -- also on a caller-owned stream, where single hs_run calls must each complete in themselves.
    struct InBatch {
        hs_context* c;
        const bool own;
        explicit InBatch(hs_context* ctx) : c(ctx), own(ctx->stream_private()) { c->in_batch = true; }
        ~InBatch() { c->in_batch = false; }
        int settle() { return own ? HS_OK : ::settle(c); }      // (on the library's own stream the sum may stay owed: every entry point settles it)
    } batch(ctx);
    if (!(opt && std::atoi(opt) != 0)) {      // plain: the launches of `steps` SpMVs enqueued from this C loop
        for (uint32_t i = 0; i < steps; ++i)
            if ((rc = step(ctx)) != HS_OK) {
                (void)batch.settle();      // a caller-owned stream is never left owing a sum, also not on the error path
                return rc;
            }
        return batch.settle();
    }
    // graph replay: the same launches captured once into a hipGraph (per step count, vector, result target and stream) and replayed
    // with ONE runtime call -- what the step costs when the host's enqueue rate is out of the picture
    if (const char* why = hisparse::dev::profiling_switch_error()) return fail(ctx, HS_ERR_BAD_ARG, why);
    if (!ctx->batch_exec || ctx->batch_steps != steps || ctx->batch_x != ctx->x_source() || ctx->batch_y != ctx->y_target() || ctx->batch_stream != ctx->stream) {
        drop_batch_graph(ctx);
        if ((rc = ::settle(ctx)) != HS_OK) return rc;        // the graph owes nothing when it begins ...
        hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamBeginCapture (the legacy default stream cannot be captured)");
        {
            CaptureScope capture(ctx);                       // the steps' cache policies are decided on a copy of the reuse tracker and frozen
            for (uint32_t i = 0; i < steps && rc == HS_OK; ++i) rc = step(ctx);
        }
        if (rc == HS_OK) rc = ::settle(ctx);                 // ... and nothing when it ends (a carried plan: K kernels + one combine)
        e = hipStreamEndCapture(ctx->stream, &ctx->batch_graph);
        if (rc == HS_OK && (e != hipSuccess || !ctx->batch_graph)) rc = hip_fail(ctx, e, "hipStreamEndCapture");
        if (rc == HS_OK && (e = hipGraphInstantiate(&ctx->batch_exec, ctx->batch_graph, nullptr, nullptr, 0)) != hipSuccess) rc = hip_fail(ctx, e, "hipGraphInstantiate");
        if (rc != HS_OK) {
            // nothing was EXECUTED during the capture: whatever the captured steps recorded as owed does not exist (a dropped graph must
            // not leave a stale debt for the next entry point to combine)
            ctx->carry.forget();
            drop_batch_graph(ctx);
            return rc;
        }
        ctx->batch_steps = steps;
        ctx->batch_x = ctx->x_source();
        ctx->batch_y = ctx->y_target();
        ctx->batch_stream = ctx->stream;
    }
    if ((rc = ::settle(ctx)) != HS_OK) return rc;
    HS_HIP(ctx, hipGraphLaunch(ctx->batch_exec, ctx->stream));
    replayed(ctx);
    return HS_OK;
}

int hs_run_partition(hs_context* ctx, uint32_t row_part_id, uint32_t part_len) {
    if (int rc = enter(ctx, kReady | kNoSettle)) return rc;      // (enqueue settles in front of a partition's launch)
    if (row_part_id >= ctx->mat.row_parts) return fail(ctx, HS_ERR_BAD_ARG, "row_part_id out of range");
    uint32_t lo, hi;
    partition_rows(ctx, row_part_id, lo, hi);
    if (part_len != (hi - lo) / hisparse::NUM_HBM_CHANNELS)
        return fail(ctx, HS_ERR_BAD_ARG, "part_len must be the partition's rows / 16 (sw/benchmark.cpp:301-322): expected " +
                                             std::to_string((hi - lo) / hisparse::NUM_HBM_CHANNELS));
    return step(ctx, int32_t(row_part_id));
}

int hs_feedback(hs_context* ctx, uint32_t scale_word, uint32_t shift_word) {
    if (int rc = enter(ctx, kReady)) return rc;
    HS_HIP(ctx, hisparse::dev::launch_feedback(ctx->is_float(), ctx->y_target(), const_cast<uint32_t*>(ctx->x_source()),
                                               std::min(ctx->mat.num_rows, ctx->mat.num_cols), scale_word, shift_word, ctx->stream));
    return HS_OK;
}

int hs_iterate(hs_context* ctx, uint32_t iterations, uint32_t scale_word, uint32_t shift_word) {
    int rc = enter(ctx, kReady | (iterations ? 0u : kHostOnly));
    if (rc != HS_OK || iterations == 0) return rc;
    const Feedback feedback{scale_word, shift_word};
    auto one_iteration = [&]() -> int { return step(ctx, -1, &feedback); };
    // One iteration = 2-3 small launches, enqueued from this C loop far faster than the GPU retires them, so plain
    // stream-ordered launches are the default.  HISPARSE_ITERATE_GRAPH=1 captures chunks of 32 iterations into one
    // hipGraph and replays them instead; measured on ROCm 7.2 that is no faster (1k x 1k: 8.4 vs 8.6 us per iteration)
    // and slower for large matrices (ogbl-ppa 64.7 vs 60.9 us: gaps between graph nodes), so it stays opt-in.
    const char* graph_env = ctx_option(ctx, "HISPARSE_ITERATE_GRAPH");
    const bool use_graph = graph_env && std::atoi(graph_env) != 0;
    const uint32_t chunk = use_graph ? std::min<uint32_t>(iterations, 32) : 1;
    uint32_t done = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (chunk > 1 && hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        {
            CaptureScope capture(ctx);
            for (uint32_t i = 0; i < chunk && rc == HS_OK; ++i) rc = one_iteration();
        }
        const hipError_t end = hipStreamEndCapture(ctx->stream, &graph);
        if (rc == HS_OK && end == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            hipError_t e = hipSuccess;
            for (; done + chunk <= iterations && e == hipSuccess; done += chunk) {
                e = hipGraphLaunch(exec, ctx->stream);
                replayed(ctx);
            }
            (void)hipGraphExecDestroy(exec);
            (void)hipGraphDestroy(graph);
            if (e != hipSuccess) return fail(ctx, HS_ERR_HIP, std::string("hipGraphLaunch: ") + hipGetErrorString(e));
        } else {
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();   // capture was refused (e.g. the legacy default stream): plain launches below
            if (rc != HS_OK) return rc;
        }
    } else {
        (void)hipGetLastError();
    }
    for (; done < iterations; ++done)
        if ((rc = one_iteration()) != HS_OK) return rc;
    return HS_OK;
}

int hs_sync(hs_context* ctx) {
    if (int rc = enter(ctx, 0)) return rc;
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return HS_OK;
}

int hs_read_result(hs_context* ctx, void* packed_y, uint32_t num_rows) {
    if (int rc = enter(ctx, kMatrix | kNoSettle, packed_y != nullptr)) return rc;
    if (num_rows != ctx->mat.num_rows) return fail(ctx, HS_ERR_BAD_ARG, "result length must equal the padded row count");
    if (int rc = settle(ctx)) return rc;
    HS_HIP(ctx, hipMemcpyAsync(packed_y, ctx->y_target(), size_t(num_rows) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return HS_OK;
}

int hs_set_option(hs_context* ctx, const char* key, const char* value) {
    if (int rc = enter(ctx, kHostOnly, key != nullptr)) return rc;
    std::string k(key);
    for (char& ch : k) ch = char(std::toupper(static_cast<unsigned char>(ch)));
    if (k.rfind("HISPARSE_", 0) == 0) k = k.substr(9);
    bool known = false;
    for (const char* name : kOptionKeys) known = known || k == name;
    if (k == "ABLATE" || k == "DEPTH" || k == "TIMELINE_OUT")
        return fail(ctx, HS_ERR_BAD_ARG, "'" + k + "' is a profiling switch of libhisparse_hip_prof.so (wrong results by design), not an option of this library");
    if (!known) return fail(ctx, HS_ERR_BAD_ARG, "unknown option '" + std::string(key) + "'");
    if (value && *value && k == "MFMA_CHUNK") {      // a value the kernel cannot take is refused here, not clamped at the load
        uint32_t chunk = 0;
        if (!hisparse::dev::detail::parse_mfma_chunk(value, chunk)) return fail(ctx, HS_ERR_BAD_ARG, hisparse::dev::detail::kBadMfmaChunk);
    }
    if (value && *value) ctx->options["HISPARSE_" + k] = value;
    else ctx->options.erase("HISPARSE_" + k);
    drop_batch_graph(ctx);      // the captured batch bakes in whatever enqueue() read at capture time: any option change invalidates it
    return HS_OK;
}

int hs_set_stream(hs_context* ctx, void* hip_stream) {
    if (int rc = enter(ctx, 0)) return rc;
    // work already enqueued must not be overtaken by work on the new stream; a caller-owned stream may be gone by now,
    // so only the library's own stream is synchronised by handle
    if (ctx->stream == ctx->own_stream) HS_HIP(ctx, hipStreamSynchronize(ctx->own_stream));
    else HS_HIP(ctx, hipDeviceSynchronize());
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return HS_OK;
}

int hs_get_stream(hs_context* ctx, void** hip_stream) {
    if (!hip_stream) return HS_ERR_BAD_ARG;
    if (int rc = enter(ctx, 0)) return rc;
    ctx->stream_shared = true;      // whoever holds the handle may order work against it: from now on every step completes in itself
    *hip_stream = ctx->stream;
    return HS_OK;
}

int hs_device_vector(hs_context* ctx, void** x_dev) {
    if (!x_dev) return HS_ERR_BAD_ARG;
    if (int rc = enter(ctx, kHostOnly)) return rc;
    if (!ctx->d_x) return fail(ctx, HS_ERR_NOT_LOADED, "hs_load_vector has not been called");
    *x_dev = ctx->d_x.get();
    return HS_OK;
}

int hs_device_result(hs_context* ctx, void** y_dev) {
    if (!y_dev) return HS_ERR_BAD_ARG;
    if (int rc = enter(ctx, kMatrix)) return rc;
    *y_dev = ctx->mat.y.get();
    return HS_OK;
}

int hs_bind_device_vector(hs_context* ctx, const void* x_dev) {
    if (int rc = enter(ctx, kHostOnly)) return rc;
    if (x_dev && (reinterpret_cast<uintptr_t>(x_dev) & 15u)) return fail(ctx, HS_ERR_BAD_ARG, "device vector must be 16-byte aligned");
    if (static_cast<const uint32_t*>(x_dev) != ctx->x_bound) drop_batch_graph(ctx);
    ctx->x_bound = static_cast<const uint32_t*>(x_dev);
    return HS_OK;
}

int hs_bind_device_result(hs_context* ctx, void* y_dev) {
    if (int rc = enter(ctx, kHostOnly)) return rc;
    if (y_dev && (reinterpret_cast<uintptr_t>(y_dev) & 15u)) return fail(ctx, HS_ERR_BAD_ARG, "device result must be 16-byte aligned");
    if (static_cast<uint32_t*>(y_dev) != ctx->y_bound) {
        if (int rc = enter(ctx, 0)) return rc;      // (an owed sum belongs to the old target)
        drop_batch_graph(ctx);
    }
    ctx->y_bound = static_cast<uint32_t*>(y_dev);
    return HS_OK;
}

int hs_push_result(hs_context* ctx, void* const* dst, uint32_t n_dst, uint32_t num_words) {
    if (int rc = enter(ctx, kMatrix | kHostOnly)) return rc;
    if (n_dst == 0) return HS_OK;
    if (!dst || n_dst > hisparse::dev::kMaxPushTargets) return fail(ctx, HS_ERR_BAD_ARG, "1 .. 8 destinations");
    if (num_words > ctx->mat.num_rows || (num_words & 3u)) return fail(ctx, HS_ERR_BAD_ARG, "num_words must be a multiple of 4 and at most the padded row count");
    for (uint32_t k = 0; k < n_dst; ++k)
        if (!dst[k] || (reinterpret_cast<uintptr_t>(dst[k]) & 15u)) return fail(ctx, HS_ERR_BAD_ARG, "destinations must be 16-byte aligned device pointers");
    if (int rc = enter(ctx, 0)) return rc;
    HS_HIP(ctx, hisparse::dev::launch_push_result(ctx->y_target(), dst, n_dst, num_words, ctx->stream));
    return HS_OK;
}

int hs_get_stats(const hs_context* ctx, hs_stats* stats) {
    if (!ctx || !stats) return HS_ERR_BAD_ARG;
    *stats = ctx->stats;
    return HS_OK;
}

int hs_time_runs(hs_context* ctx, int warmup, int runs, float* total_ms, float* kernel_ms) {
    int rc = enter(ctx, kReady | kNoSettle);      // (the warm-up steps carry on from the caller's last step)
    if (rc != HS_OK) return rc;
    if (warmup < 0 || runs <= 0) return fail(ctx, HS_ERR_BAD_ARG, "need warmup >= 0 and runs > 0");
    for (int i = 0; i < warmup; ++i)
        if ((rc = step(ctx)) != HS_OK) return rc;
    if ((rc = settle(ctx)) != HS_OK) return rc;
    HS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<DeviceEvent> events(2 + (kernel_ms ? size_t(runs) * 2 : 0));
    for (DeviceEvent& ev : events) HS_HIP(ctx, ev.create());
    const hipEvent_t begin = events[0].get(), end = events[1].get();
    const DeviceEvent* k = events.data() + 2;
    HS_HIP(ctx, hipEventRecord(begin, ctx->stream));
    for (int i = 0; i < runs; ++i)
        if ((rc = enqueue(ctx, ctx->x_source(), ctx->y_target(), -1, kernel_ms ? k[size_t(i) * 2].get() : nullptr, kernel_ms ? k[size_t(i) * 2 + 1].get() : nullptr)) != HS_OK) return rc;
    if ((rc = settle(ctx)) != HS_OK) return rc;        // (the last step's sum may still be owed)
    HS_HIP(ctx, hipEventRecord(end, ctx->stream));
    HS_HIP(ctx, hipEventSynchronize(end));
    float ms = 0.0f;
    HS_HIP(ctx, hipEventElapsedTime(&ms, begin, end));
    if (total_ms) *total_ms = ms;
    if (kernel_ms) {
        float sum = 0.0f;
        for (int i = 0; i < runs; ++i) {
            float one = 0.0f;
            HS_HIP(ctx, hipEventElapsedTime(&one, k[size_t(i) * 2].get(), k[size_t(i) * 2 + 1].get()));
            sum += one;
        }
        *kernel_ms = sum;
    }
    return HS_OK;
}

int hs_time_kernel(hs_context* ctx, int warmup, int runs, float* kernel_ms) {
    int rc = enter(ctx, kReady | kHostOnly);
    if (rc != HS_OK) return rc;
    if (warmup < 0 || runs <= 0 || !kernel_ms) return fail(ctx, HS_ERR_BAD_ARG, "need warmup >= 0, runs > 0 and an output pointer");
    if (const char* why = hisparse::dev::profiling_switch_error()) return fail(ctx, HS_ERR_BAD_ARG, why);
    if ((rc = enter(ctx, 0)) != HS_OK) return rc;
    // a plan whose combine pass is carried into the next step's kernel: the kernel as it runs in consecutive steps, i.e. with that work in it
    const bool carried = ctx->carry.carries() && ctx->stream_private();
    auto launch = [&]() -> int {
        if (carried) return step(ctx);
        const hisparse::dev::SpmvLaunch args = launch_args(ctx, ctx->x_source(), ctx->y_target(), -1);      // (per launch: its cache policy is the launch's)
        HS_HIP(ctx, hisparse::dev::launch_spmv(ctx->is_float(), args, ctx->stream));
        return HS_OK;
    };
    for (int i = 0; i < warmup; ++i)
        if ((rc = launch()) != HS_OK) return rc;
    DeviceEvent ev[2];
    HS_HIP(ctx, ev[0].create());
    HS_HIP(ctx, ev[1].create());
    HS_HIP(ctx, hipEventRecord(ev[0].get(), ctx->stream));
    for (int i = 0; i < runs; ++i)
        if ((rc = launch()) != HS_OK) return rc;
    HS_HIP(ctx, hipEventRecord(ev[1].get(), ctx->stream));
    HS_HIP(ctx, hipEventSynchronize(ev[1].get()));
    HS_HIP(ctx, hipEventElapsedTime(kernel_ms, ev[0].get(), ev[1].get()));
    // column-sliced plans: the launches above left partial sums only; one whole step (or the owed combine) puts y back in order
    return carried ? settle(ctx) : step(ctx);
}

}  // extern "C"
