// hsw_api.cpp — include/hisparse_wide.h on the HIP runtime: the pattern object of the row-major feature products.  One object owns one
// device, one stream of its own and, from hsw_create on, all the device memory its _device calls will ever use (device_buffer.h): the CSR
// arrays, the rows sorted into length classes (wide_products.h) and, with HSW_TRANSPOSED, the same three for the transposed pattern plus
// the map from its entries back to CSR order.  Both schedules and the transposed pattern are built here, on the host; the kernels are in
// wide_products.hip.  Nothing here touches a context, an hsp_pattern or a numeric mode.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "hsw_common.h"
#include "wide_products.h"
#include "wide_schedule.h"

namespace {

using namespace hisparse::dev;

// one side of the pattern on the device (WideSide's arrays and their owner)
struct Side {
    DeviceBuffer<uint32_t> ptr, idx, perm, list;
    WideSide view;
};

}  // namespace

struct hsw_pattern {
    int device = 0;
    uint32_t num_rows = 0, num_cols = 0;
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    uint32_t compute_units = 0;
    bool transposed = false;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    Side rows, cols;      // cols: the transposed pattern (HSW_TRANSPOSED)
    std::string error;
};

namespace {

thread_local std::string g_create_error;

int fail(hsw_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hsw_pattern* p, hipError_t e, const char* what) { return fail(p, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define HSW_HIP(p, call)                                              \
    do {                                                              \
        const hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail((p), e_, #call);        \
    } while (0)

int enter(hsw_pattern* p) {
    if (!p) return HS_ERR_BAD_ARG;
    HSW_HIP(p, hipSetDevice(p->device));
    return HS_OK;
}

// one side's arrays onto the device; mapped: the side has a perm array (of nnz words, like idx)
int upload(hsw_pattern* p, Side& s, uint32_t rows, const uint32_t* ptr, const uint32_t* idx, bool mapped, const uint32_t* perm) {
    std::vector<uint32_t> list;
    schedule(rows, ptr, list, s.view.count);
    const size_t ptr_bytes = (size_t(rows) + 1) * 4, entry_bytes = std::max<size_t>(size_t(p->nnz), 1) * 4, list_bytes = size_t(rows) * 4;
    HSW_HIP(p, s.ptr.alloc(ptr_bytes));
    HSW_HIP(p, s.idx.alloc(entry_bytes));
    HSW_HIP(p, s.list.alloc(list_bytes));
    p->device_bytes += ptr_bytes + entry_bytes + list_bytes;
    HSW_HIP(p, hipMemcpyAsync(s.ptr.get(), ptr, ptr_bytes, hipMemcpyHostToDevice, p->own_stream));
    HSW_HIP(p, hipMemcpyAsync(s.list.get(), list.data(), list_bytes, hipMemcpyHostToDevice, p->own_stream));
    if (p->nnz) HSW_HIP(p, hipMemcpyAsync(s.idx.get(), idx, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    if (mapped) {
        HSW_HIP(p, s.perm.alloc(entry_bytes));
        p->device_bytes += entry_bytes;
        if (p->nnz) HSW_HIP(p, hipMemcpyAsync(s.perm.get(), perm, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    }
    HSW_HIP(p, hipStreamSynchronize(p->own_stream));      // the host arrays (the caller's, `list`) are free again
    s.view.ptr = s.ptr.get();
    s.view.idx = s.idx.get();
    s.view.perm = s.perm.get();
    s.view.list = s.list.get();
    s.view.entries = p->nnz;
    s.view.compute_units = p->compute_units;
    return HS_OK;
}

// everything hsw_create does on the device; the caller destroys p when this fails
int build(hsw_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    HSW_HIP(p, hipSetDevice(p->device));
    HSW_HIP(p, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    p->stream = p->own_stream;
    if (int rc = upload(p, p->rows, p->num_rows, indptr, indices, false, nullptr)) return rc;
    if (p->transposed) {
        std::vector<uint32_t> cptr, row, perm;
        hisparse::hsw::build_transposed(p->num_rows, p->num_cols, indptr, indices, cptr, row, perm);
        if (int rc = upload(p, p->cols, p->num_cols, cptr.data(), row.data(), true, perm.data())) return rc;
    }
    return HS_OK;
}

// A dense host operand of n rows x d words on the device with ld = d rounded up to 4 (the pad words stay as allocated: loaded, never used)
int features_in(hsw_pattern* p, DeviceBuffer<float>& dev, const float* host, uint32_t n, uint32_t d, uint64_t ld) {
    HSW_HIP(p, dev.alloc_count(size_t(n) * ld, 16));
    HSW_HIP(p, hipMemcpy2DAsync(dev.get(), ld * 4, host, size_t(d) * 4, size_t(d) * 4, n, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

int entries_in(hsw_pattern* p, DeviceBuffer<float>& dev, const float* host) {
    HSW_HIP(p, dev.alloc_count(size_t(p->nnz), 16));
    if (p->nnz) HSW_HIP(p, hipMemcpyAsync(dev.get(), host, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

// the host forms' ends: copy out when all went well (`rows` rows of `words` words from rows of ld), always wait before the transient buffers go
int finish(hsw_pattern* p, int rc, float* host, const float* dev, uint64_t rows, uint64_t words, uint64_t ld) {
    if (rc == HS_OK && rows && words) {
        const hipError_t e = ld == words ? hipMemcpyAsync(host, dev, size_t(rows * words) * 4, hipMemcpyDeviceToHost, p->stream)
                                         : hipMemcpy2DAsync(host, size_t(words) * 4, dev, size_t(ld) * 4, size_t(words) * 4, size_t(rows), hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// hsw_spmm (side = rows) and hsw_spmm_t (side = cols) after their checks
int spmm_host(hsw_pattern* p, bool transposed, const float* w, const float* x, uint32_t d, float* y) {
    const uint32_t y_rows = transposed ? p->num_cols : p->num_rows, x_rows = transposed ? p->num_rows : p->num_cols;
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, w, p->nnz, x, uint64_t(x_rows) * d, y, uint64_t(y_rows) * d, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    DeviceBuffer<float> d_w, d_x, d_y;      // transient (the host form is synchronous and may allocate)
    if (int rc = entries_in(p, d_w, w)) return rc;
    if (int rc = features_in(p, d_x, x, x_rows, d, ld)) return rc;
    HSW_HIP(p, d_y.alloc_count(size_t(y_rows) * ld, 16));
    const int rc = transposed ? hsw_spmm_t_device(p, d_w.get(), d_x.get(), ld, d, d_y.get(), ld) : hsw_spmm_device(p, d_w.get(), d_x.get(), ld, d, d_y.get(), ld);
    return finish(p, rc, y, d_y.get(), y_rows, d, ld);
}

}  // namespace

extern "C" {

int hsw_create(hsw_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t flags) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsw::check_create(num_rows, num_cols, indptr, indices, flags, why)) return fail(nullptr, rc, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hsw_pattern* p = new (std::nothrow) hsw_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->nnz = indptr[num_rows];
    p->compute_units = uint32_t(prop.multiProcessorCount);
    p->transposed = (flags & HSW_TRANSPOSED) != 0;
    if (int rc = build(p, indptr, indices)) {
        g_create_error = p->error;
        if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
        delete p;
        return rc;
    }
    *out = p;
    return HS_OK;
}

int hsw_destroy(hsw_pattern* p) {
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

const char* hsw_last_error(const hsw_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsw_info(const hsw_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz;
    if (device_bytes) *device_bytes = p->device_bytes;
    return HS_OK;
}

int hsw_set_stream(hsw_pattern* p, void* hip_stream) {
    if (!p) return HS_ERR_BAD_ARG;
    p->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->own_stream;
    return HS_OK;
}

int hsw_sync(hsw_pattern* p) {
    if (int rc = enter(p)) return rc;
    HSW_HIP(p, hipStreamSynchronize(p->stream));
    return HS_OK;
}

int hsw_sddmm_device(hsw_pattern* p, const float* u_dev, uint64_t ldu, const float* v_dev, uint64_t ldv, uint32_t d, float* out_dev) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_sddmm(p->num_rows, p->num_cols, p->nnz, u_dev, ldu, v_dev, ldv, d, out_dev, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSW_HIP(p, launch_wide_dot(p->rows.view, u_dev, ldu, v_dev, ldv, d, out_dev, p->stream));
    return HS_OK;
}

int hsw_spmm_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_spmm(p->num_rows, p->num_cols, p->nnz, w_dev, x_dev, ldx, d, y_dev, ldy, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSW_HIP(p, launch_wide_gather(p->rows.view, w_dev, x_dev, ldx, d, y_dev, ldy, p->stream));
    return HS_OK;
}

int hsw_spmm_t_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_spmm(p->num_cols, p->num_rows, p->nnz, w_dev, x_dev, ldx, d, y_dev, ldy, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSW_HIP(p, launch_wide_gather(p->cols.view, w_dev, x_dev, ldx, d, y_dev, ldy, p->stream));
    return HS_OK;
}

int hsw_sddmm(hsw_pattern* p, const float* u, const float* v, uint32_t d, float* out) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, u, uint64_t(p->num_rows) * d, v, uint64_t(p->num_cols) * d, out, p->nnz, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    DeviceBuffer<float> d_u, d_v, d_out;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_u, u, p->num_rows, d, ld)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, d, ld)) return rc;
    HSW_HIP(p, d_out.alloc_count(size_t(p->nnz), 16));
    return finish(p, hsw_sddmm_device(p, d_u.get(), ld, d_v.get(), ld, d, d_out.get()), out, d_out.get(), 1, p->nnz, p->nnz);
}

int hsw_spmm(hsw_pattern* p, const float* w, const float* x, uint32_t d, float* y) {
    if (!p) return HS_ERR_BAD_ARG;
    return spmm_host(p, false, w, x, d, y);
}

int hsw_spmm_t(hsw_pattern* p, const float* w, const float* x, uint32_t d, float* y) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    return spmm_host(p, true, w, x, d, y);
}

}  // extern "C"
