// hsp_api.cpp — include/hisparse_pattern.h on the HIP runtime: the pattern object of the sampled dense product.  One object owns one
// device, one stream of its own and, from hsp_create on, all the device memory it will ever use (device_buffer.h): the column and the
// row of every entry and the two staging buffers for max_k vectors.  The kernels are in sddmm.hip.  Nothing here touches a context.
#include <cstring>
#include <new>
#include <string>

#include "device_buffer.h"
#include "hsp_common.h"
#include "sddmm.h"

struct hsp_pattern {
    int device = 0;
    int impl = 0;
    uint32_t num_rows = 0, num_cols = 0, max_k = 0;
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    uint32_t compute_units = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffer<uint32_t> row, col;      // per entry, CSR order
    DeviceBuffer<uint32_t> u4, v4;        // staging: ceil(max_k / 4) groups of num_rows (num_cols) x 4 words; none when max_k = 1
    std::string error;
};

namespace {

using hisparse::hsp::round_up4;

thread_local std::string g_create_error;

int fail(hsp_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hsp_pattern* p, hipError_t e, const char* what) { return fail(p, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define HSP_HIP(p, call)                                              \
    do {                                                              \
        const hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail((p), e_, #call);        \
    } while (0)

int enter(hsp_pattern* p) {
    if (!p) return HS_ERR_BAD_ARG;
    HSP_HIP(p, hipSetDevice(p->device));
    return HS_OK;
}

// everything hsp_create does on the device; the caller destroys p when this fails
int build(hsp_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    HSP_HIP(p, hipSetDevice(p->device));
    HSP_HIP(p, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    p->stream = p->own_stream;
    const size_t entry_bytes = size_t(round_up4(p->nnz)) * 4;      // whole 16-byte words for the four-entry loads
    HSP_HIP(p, p->row.alloc(std::max<size_t>(entry_bytes, 16)));
    HSP_HIP(p, p->col.alloc(std::max<size_t>(entry_bytes, 16)));
    p->device_bytes = 2 * std::max<size_t>(entry_bytes, 16);
    if (p->max_k >= 2) {
        const size_t groups = (p->max_k + hisparse::hsp::kGroup - 1) / hisparse::hsp::kGroup;
        HSP_HIP(p, p->u4.alloc(groups * p->num_rows * 16));
        HSP_HIP(p, p->v4.alloc(groups * p->num_cols * 16));
        p->device_bytes += groups * (size_t(p->num_rows) + p->num_cols) * 16;
    }
    if (p->nnz == 0) return HS_OK;
    DeviceBuffer<uint32_t> d_indptr;      // needed by the expansion only
    HSP_HIP(p, d_indptr.alloc_count(size_t(p->num_rows) + 1));
    HSP_HIP(p, hipMemcpyAsync(d_indptr.get(), indptr, (size_t(p->num_rows) + 1) * 4, hipMemcpyHostToDevice, p->own_stream));
    HSP_HIP(p, hipMemcpyAsync(p->col.get(), indices, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    HSP_HIP(p, hisparse::dev::launch_expand_rows(d_indptr.get(), p->num_rows, p->nnz, p->row.get(), p->compute_units, p->own_stream));
    HSP_HIP(p, hipStreamSynchronize(p->own_stream));      // the caller's arrays and d_indptr are free again
    return HS_OK;
}

}  // namespace

extern "C" {

int hsp_create(hsp_pattern** out, int device_id, int impl, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices,
               uint32_t max_k) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsp::check_pattern(impl, num_rows, num_cols, indptr, indices, max_k, why)) return fail(nullptr, rc, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hsp_pattern* p = new (std::nothrow) hsp_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->impl = impl;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->max_k = max_k;
    p->nnz = indptr[num_rows];
    p->compute_units = uint32_t(prop.multiProcessorCount);
    if (int rc = build(p, indptr, indices)) {
        g_create_error = p->error;
        if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
        delete p;
        return rc;
    }
    *out = p;
    return HS_OK;
}

int hsp_destroy(hsp_pattern* p) {
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

const char* hsp_last_error(const hsp_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsp_info(const hsp_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz;
    if (device_bytes) *device_bytes = p->device_bytes;
    return HS_OK;
}

int hsp_set_stream(hsp_pattern* p, void* hip_stream) {
    if (!p) return HS_ERR_BAD_ARG;
    p->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->own_stream;
    return HS_OK;
}

int hsp_sync(hsp_pattern* p) {
    if (int rc = enter(p)) return rc;
    HSP_HIP(p, hipStreamSynchronize(p->stream));
    return HS_OK;
}

int hsp_sddmm_device(hsp_pattern* p, const void* u_dev, uint64_t ldu, const void* v_dev, uint64_t ldv, uint32_t k, void* out_dev, int accumulate) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsp::check_product(p->num_rows, p->num_cols, p->max_k, u_dev, ldu, v_dev, ldv, k, out_dev, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    hisparse::dev::SddmmLaunch a;
    a.row = p->row.get();
    a.col = p->col.get();
    a.nnz = p->nnz;
    a.num_rows = p->num_rows;
    a.num_cols = p->num_cols;
    a.u = static_cast<const uint32_t*>(u_dev);
    a.v = static_cast<const uint32_t*>(v_dev);
    a.ldu = ldu;
    a.ldv = ldv;
    a.k = k;
    a.u4 = p->u4.get();
    a.v4 = p->v4.get();
    a.out = static_cast<uint32_t*>(out_dev);
    a.accumulate = accumulate != 0;
    a.compute_units = p->compute_units;
    HSP_HIP(p, hisparse::dev::launch_sddmm(p->impl == HS_IMPL_FIXED, a, p->stream));
    return HS_OK;
}

int hsp_sddmm(hsp_pattern* p, const void* u, const void* v, uint32_t k, void* out) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!u || !v || !out) return fail(p, HS_ERR_BAD_ARG, "null argument");
    if (k < 1 || k > p->max_k) return fail(p, HS_ERR_BAD_ARG, "k must be 1 ... max_k (" + std::to_string(p->max_k) + ")");
    if (int rc = enter(p)) return rc;
    const uint64_t ldu = round_up4(p->num_rows), ldv = round_up4(p->num_cols);
    DeviceBuffer<uint32_t> d_u, d_v, d_out;      // transient: the host form is synchronous and may allocate
    HSP_HIP(p, d_u.alloc_count(size_t(k) * ldu));
    HSP_HIP(p, d_v.alloc_count(size_t(k) * ldv));
    HSP_HIP(p, d_out.alloc_count(size_t(round_up4(p->nnz)), 16));
    HSP_HIP(p, hipMemcpyAsync(d_u.get(), u, size_t(k) * ldu * 4, hipMemcpyHostToDevice, p->stream));
    HSP_HIP(p, hipMemcpyAsync(d_v.get(), v, size_t(k) * ldv * 4, hipMemcpyHostToDevice, p->stream));
    int rc = hsp_sddmm_device(p, d_u.get(), ldu, d_v.get(), ldv, k, d_out.get(), 0);
    if (rc == HS_OK && p->nnz) {
        const hipError_t e = hipMemcpyAsync(out, d_out.get(), size_t(p->nnz) * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "hipMemcpyAsync");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);      // always, before the transient buffers go
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

}  // extern "C"
