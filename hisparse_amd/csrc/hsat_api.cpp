// hsat_api.cpp — include/hisparse_attention.h on the HIP runtime: the pattern object of the fused attention step.  As hsw_api.cpp's, one
// object owns one device, one stream of its own and, from hsat_create on, all the device memory its _device call will ever use
// (device_buffer.h): the CSR arrays and the rows sorted into the length classes of wide_products.h (wide_schedule.h).  The kernel is in
// pattern_attention.hip.  Nothing here touches a context or another pattern object.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "hsat_common.h"
#include "pattern_attention.h"
#include "wide_schedule.h"

using namespace hisparse::dev;

struct hsat_pattern {
    int device = 0;
    uint32_t num_rows = 0, num_cols = 0;
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffer<uint32_t> ptr, idx, list;
    WideSide view;
    std::string error;
};

namespace {

thread_local std::string g_create_error;

int fail(hsat_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hsat_pattern* p, hipError_t e, const char* what) { return fail(p, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define HSAT_HIP(p, call)                                             \
    do {                                                              \
        const hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail((p), e_, #call);        \
    } while (0)

int enter(hsat_pattern* p) {
    if (!p) return HS_ERR_BAD_ARG;
    HSAT_HIP(p, hipSetDevice(p->device));
    return HS_OK;
}

// everything hsat_create does on the device; the caller destroys p when this fails
int build(hsat_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    HSAT_HIP(p, hipSetDevice(p->device));
    HSAT_HIP(p, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    p->stream = p->own_stream;
    std::vector<uint32_t> list;
    schedule(p->num_rows, indptr, list, p->view.count);
    const size_t ptr_bytes = (size_t(p->num_rows) + 1) * 4, entry_bytes = std::max<size_t>(size_t(p->nnz), 1) * 4, list_bytes = size_t(p->num_rows) * 4;
    HSAT_HIP(p, p->ptr.alloc(ptr_bytes));
    HSAT_HIP(p, p->idx.alloc(entry_bytes));
    HSAT_HIP(p, p->list.alloc(list_bytes));
    p->device_bytes = ptr_bytes + entry_bytes + list_bytes;
    HSAT_HIP(p, hipMemcpyAsync(p->ptr.get(), indptr, ptr_bytes, hipMemcpyHostToDevice, p->own_stream));
    HSAT_HIP(p, hipMemcpyAsync(p->list.get(), list.data(), list_bytes, hipMemcpyHostToDevice, p->own_stream));
    if (p->nnz) HSAT_HIP(p, hipMemcpyAsync(p->idx.get(), indices, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    HSAT_HIP(p, hipStreamSynchronize(p->own_stream));      // the host arrays (the caller's, `list`) are free again
    p->view.ptr = p->ptr.get();
    p->view.idx = p->idx.get();
    p->view.list = p->list.get();
    p->view.entries = p->nnz;
    return HS_OK;
}

// A dense host operand of n rows x d words on the device with ld = d rounded up to 4 (the pad words stay as allocated: loaded, never used)
int features_in(hsat_pattern* p, DeviceBuffer<float>& dev, const float* host, uint32_t n, uint32_t d, uint64_t ld) {
    HSAT_HIP(p, dev.alloc_count(size_t(n) * ld, 16));
    HSAT_HIP(p, hipMemcpy2DAsync(dev.get(), ld * 4, host, size_t(d) * 4, size_t(d) * 4, n, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

}  // namespace

extern "C" {

int hsat_create(hsat_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsat::check_create(num_rows, num_cols, indptr, indices, why)) return fail(nullptr, rc, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hsat_pattern* p = new (std::nothrow) hsat_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->nnz = indptr[num_rows];
    p->view.compute_units = uint32_t(prop.multiProcessorCount);
    if (int rc = build(p, indptr, indices)) {
        g_create_error = p->error;
        if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
        delete p;
        return rc;
    }
    *out = p;
    return HS_OK;
}

int hsat_destroy(hsat_pattern* p) {
    if (!p) return HS_OK;
    (void)hipSetDevice(p->device);
    // only the object's own stream is known to be alive; a caller-owned stream must have been synchronised by its owner
    if (p->own_stream) {
        (void)hipStreamSynchronize(p->own_stream);
        (void)hipStreamDestroy(p->own_stream);
    }
    delete p;
    return HS_OK;
}

const char* hsat_last_error(const hsat_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsat_info(const hsat_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz;
    if (device_bytes) *device_bytes = p->device_bytes;
    return HS_OK;
}

int hsat_set_stream(hsat_pattern* p, void* hip_stream) {
    if (!p) return HS_ERR_BAD_ARG;
    p->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->own_stream;
    return HS_OK;
}

int hsat_sync(hsat_pattern* p) {
    if (int rc = enter(p)) return rc;
    HSAT_HIP(p, hipStreamSynchronize(p->stream));
    return HS_OK;
}

int hsat_forward_device(hsat_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, uint32_t d, float scale,
                        float* y_dev, uint64_t ldy, float* lse_dev) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsat::check_forward(p->num_rows, p->num_cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, d, scale, y_dev, ldy, lse_dev, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSAT_HIP(p, launch_pattern_attention(p->view, q_dev, ldq, k_dev, ldk, v_dev, ldv, d, scale, y_dev, ldy, lse_dev, p->stream));
    return HS_OK;
}

int hsat_forward(hsat_pattern* p, const float* q, const float* k, const float* v, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsat::check_forward_host(p->num_rows, p->num_cols, q, k, v, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    DeviceBuffer<float> d_q, d_k, d_v, d_y, d_lse;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, d, ld)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, d, ld)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, d, ld)) return rc;
    HSAT_HIP(p, d_y.alloc_count(size_t(p->num_rows) * ld, 16));
    HSAT_HIP(p, d_lse.alloc_count(size_t(p->num_rows), 16));
    int rc = hsat_forward_device(p, d_q.get(), ld, d_k.get(), ld, d_v.get(), ld, d, scale, d_y.get(), ld, lse ? d_lse.get() : nullptr);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpy2DAsync(y, size_t(d) * 4, d_y.get(), size_t(ld) * 4, size_t(d) * 4, p->num_rows, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

}  // extern "C"
