// hsr_api.cpp — include/hisparse_rows.h on the HIP runtime: the rows object of the row softmax.  One object owns one device, one stream of
// its own and, from hsr_create on, all the device memory its _device calls will ever use (device_buffer.h): indptr, the non-empty rows
// sorted into length classes and the 16-word table that maps virtual workgroups to classes (row_softmax.h).  The schedule is built here,
// on the host, from indptr; the kernels are in row_softmax.hip.  Nothing here touches a context, a pattern or a numeric mode.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "hsr_common.h"
#include "row_softmax.h"

struct hsr_rows {
    int device = 0;
    uint32_t num_rows = 0;
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    uint32_t compute_units = 0;
    uint32_t workgroups = 0;      // virtual workgroups of the schedule
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffer<uint32_t> indptr, list, table;
    std::string error;
};

namespace {

using namespace hisparse::dev;

thread_local std::string g_create_error;

int fail(hsr_rows* r, int code, const std::string& msg) {
    if (r) r->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hsr_rows* r, hipError_t e, const char* what) { return fail(r, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define HSR_HIP(r, call)                                              \
    do {                                                              \
        const hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail((r), e_, #call);        \
    } while (0)

int enter(hsr_rows* r) {
    if (!r) return HS_ERR_BAD_ARG;
    HSR_HIP(r, hipSetDevice(r->device));
    return HS_OK;
}

// the non-empty rows class by class and the table of row_softmax.h; the long rows (class 0, started first) longest first, the others ascending
void schedule(uint32_t num_rows, const uint32_t* indptr, std::vector<uint32_t>& list, uint32_t (&table)[kRowsTableWords]) {
    uint32_t count[kRowsClasses] = {};
    for (uint32_t r = 0; r < num_rows; ++r)
        if (const uint32_t n = indptr[r + 1] - indptr[r]) ++count[rows_class_of(n)];
    std::memset(table, 0, sizeof table);
    uint32_t next[kRowsClasses];
    for (uint32_t c = 0; c < kRowsClasses; ++c) {
        const uint32_t per = rows_per_workgroup(c);
        next[c] = table[8 + c];
        table[c + 1] = table[c] + (count[c] + per - 1) / per;      // [6]: all of them
        table[8 + c + 1] = table[8 + c] + count[c];                // [14]: the non-empty rows
    }
    list.resize(table[8 + kRowsClasses]);
    for (uint32_t r = 0; r < num_rows; ++r)
        if (const uint32_t n = indptr[r + 1] - indptr[r]) list[next[rows_class_of(n)]++] = r;
    std::stable_sort(list.begin(), list.begin() + count[0], [&](uint32_t a, uint32_t b) { return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b]; });
}

// everything hsr_create does on the device; the caller destroys r when this fails
int build(hsr_rows* r, const uint32_t* indptr) {
    std::vector<uint32_t> list;
    uint32_t table[kRowsTableWords];
    schedule(r->num_rows, indptr, list, table);
    r->workgroups = table[kRowsClasses];
    HSR_HIP(r, hipSetDevice(r->device));
    HSR_HIP(r, hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking));
    r->stream = r->own_stream;
    const size_t indptr_bytes = (size_t(r->num_rows) + 1) * 4, list_bytes = std::max<size_t>(list.size(), 1) * 4, table_bytes = kRowsTableWords * 4;
    HSR_HIP(r, r->indptr.alloc(indptr_bytes));
    HSR_HIP(r, r->list.alloc(list_bytes));
    HSR_HIP(r, r->table.alloc(table_bytes));
    r->device_bytes = indptr_bytes + list_bytes + table_bytes;
    HSR_HIP(r, hipMemcpyAsync(r->indptr.get(), indptr, indptr_bytes, hipMemcpyHostToDevice, r->own_stream));
    if (!list.empty()) HSR_HIP(r, hipMemcpyAsync(r->list.get(), list.data(), list.size() * 4, hipMemcpyHostToDevice, r->own_stream));
    HSR_HIP(r, hipMemcpyAsync(r->table.get(), table, table_bytes, hipMemcpyHostToDevice, r->own_stream));
    HSR_HIP(r, hipStreamSynchronize(r->own_stream));      // the caller's array, list and table are free again
    return HS_OK;
}

RowSoftmaxLaunch launch_of(const hsr_rows* r) {
    RowSoftmaxLaunch a;
    a.indptr = r->indptr.get();
    a.list = r->list.get();
    a.table = r->table.get();
    a.workgroups = r->workgroups;
    a.compute_units = r->compute_units;
    return a;
}

// the host forms' ends: copy out when all went well, always wait before the transient buffers go
int finish(hsr_rows* r, int rc, float* host, const float* dev) {
    if (rc == HS_OK && r->nnz) {
        const hipError_t e = hipMemcpyAsync(host, dev, size_t(r->nnz) * 4, hipMemcpyDeviceToHost, r->stream);
        if (e != hipSuccess) rc = hip_fail(r, e, "hipMemcpyAsync");
    }
    const hipError_t e = hipStreamSynchronize(r->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(r, e, "hipStreamSynchronize");
    return rc;
}

}  // namespace

extern "C" {

int hsr_create(hsr_rows** out, int device_id, uint32_t num_rows, const uint32_t* indptr) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null rows pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsr::check_rows(num_rows, indptr, why)) return fail(nullptr, rc, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hsr_rows* r = new (std::nothrow) hsr_rows;
    if (!r) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    r->device = device_id;
    r->num_rows = num_rows;
    r->nnz = indptr[num_rows];
    r->compute_units = uint32_t(prop.multiProcessorCount);
    if (int rc = build(r, indptr)) {
        g_create_error = r->error;
        if (r->own_stream) (void)hipStreamDestroy(r->own_stream);
        delete r;
        return rc;
    }
    *out = r;
    return HS_OK;
}

int hsr_destroy(hsr_rows* r) {
    if (!r) return HS_OK;
    (void)hipSetDevice(r->device);
    // only the object's own stream is known to be alive; a caller-owned stream must have been synchronised by its owner
    if (r->own_stream) {
        (void)hipStreamSynchronize(r->own_stream);
        (void)hipStreamDestroy(r->own_stream);
    }
    delete r;
    return HS_OK;
}

const char* hsr_last_error(const hsr_rows* r) { return r ? r->error.c_str() : g_create_error.c_str(); }

int hsr_info(const hsr_rows* r, uint64_t* nnz, uint64_t* device_bytes) {
    if (!r) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = r->nnz;
    if (device_bytes) *device_bytes = r->device_bytes;
    return HS_OK;
}

int hsr_set_stream(hsr_rows* r, void* hip_stream) {
    if (!r) return HS_ERR_BAD_ARG;
    r->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : r->own_stream;
    return HS_OK;
}

int hsr_sync(hsr_rows* r) {
    if (int rc = enter(r)) return rc;
    HSR_HIP(r, hipStreamSynchronize(r->stream));
    return HS_OK;
}

int hsr_softmax_device(hsr_rows* r, const float* s_dev, float scale, float* p_dev) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_forward(r->nnz, s_dev, scale, p_dev, true, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    HSR_HIP(r, launch_row_softmax(launch_of(r), s_dev, scale, p_dev, r->stream));
    return HS_OK;
}

int hsr_softmax_backward_device(hsr_rows* r, const float* p_dev, const float* gp_dev, float scale, float* gs_dev) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_backward(r->nnz, p_dev, gp_dev, scale, gs_dev, true, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    HSR_HIP(r, launch_row_softmax_backward(launch_of(r), p_dev, gp_dev, scale, gs_dev, r->stream));
    return HS_OK;
}

int hsr_softmax(hsr_rows* r, const float* s, float scale, float* p) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_forward(r->nnz, s, scale, p, false, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    DeviceBuffer<float> d;      // transient (the host form is synchronous and may allocate); the kernel runs in place
    HSR_HIP(r, d.alloc_count(size_t(r->nnz), 16));
    HSR_HIP(r, hipMemcpyAsync(d.get(), s, size_t(r->nnz) * 4, hipMemcpyHostToDevice, r->stream));
    return finish(r, hsr_softmax_device(r, d.get(), scale, d.get()), p, d.get());
}

int hsr_softmax_backward(hsr_rows* r, const float* p, const float* gp, float scale, float* gs) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_backward(r->nnz, p, gp, scale, gs, false, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    DeviceBuffer<float> d_p, d_g;      // transient; the gradient is written over gp's copy
    HSR_HIP(r, d_p.alloc_count(size_t(r->nnz), 16));
    HSR_HIP(r, d_g.alloc_count(size_t(r->nnz), 16));
    HSR_HIP(r, hipMemcpyAsync(d_p.get(), p, size_t(r->nnz) * 4, hipMemcpyHostToDevice, r->stream));
    HSR_HIP(r, hipMemcpyAsync(d_g.get(), gp, size_t(r->nnz) * 4, hipMemcpyHostToDevice, r->stream));
    return finish(r, hsr_softmax_backward_device(r, d_p.get(), d_g.get(), scale, d_g.get()), gs, d_g.get());
}

}  // extern "C"
