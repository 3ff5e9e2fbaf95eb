// hsab_api.cpp — include/hisparse_attention_backward.h on the HIP runtime: the pattern object of the fused attention backward step.  As
// hsat_api.cpp's, one object owns one device, one stream of its own and, from hsab_create on, all the device memory its _device call will
// ever use (device_buffer.h): the CSR arrays with the rows sorted into the length classes of wide_products.h (wide_schedule.h), the
// transposed pattern (hsw_common.h's stable counting sort, WITHOUT its CSR-index map: there is no per-entry array to index) with the
// columns sorted the same way, and one double per row, the D words the first kernel writes and the second reads.  The kernels are in
// attention_backward.hip.  Nothing here touches a context or another pattern object.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "attention_backward.h"
#include "device_buffer.h"
#include "hsab_common.h"
#include "wide_schedule.h"

using namespace hisparse::dev;

struct hsab_pattern {
    int device = 0;
    uint32_t num_rows = 0, num_cols = 0;
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffer<uint32_t> ptr, idx, list;         // the pattern and its rows by class
    DeviceBuffer<uint32_t> cptr, crow, clist;      // the transposed pattern and its columns by class
    DeviceBuffer<double> dsum;                     // D per row: one backward call in flight per object
    WideSide rows, cols;
    std::string error;
};

namespace {

thread_local std::string g_create_error;

int fail(hsab_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hsab_pattern* p, hipError_t e, const char* what) { return fail(p, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define HSAB_HIP(p, call)                                             \
    do {                                                              \
        const hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail((p), e_, #call);        \
    } while (0)

int enter(hsab_pattern* p) {
    if (!p) return HS_ERR_BAD_ARG;
    HSAB_HIP(p, hipSetDevice(p->device));
    return HS_OK;
}

// everything hsab_create does on the device; the caller destroys p when this fails
int build(hsab_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    HSAB_HIP(p, hipSetDevice(p->device));
    HSAB_HIP(p, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    p->stream = p->own_stream;
    std::vector<uint32_t> list, cptr, crow, clist;
    schedule(p->num_rows, indptr, list, p->rows.count);
    {
        std::vector<uint32_t> perm;      // the CSR index of every entry in column order: built by the shared sort, not kept
        hisparse::hsw::build_transposed(p->num_rows, p->num_cols, indptr, indices, cptr, crow, perm);
    }
    schedule(p->num_cols, cptr.data(), clist, p->cols.count);
    const size_t ptr_bytes = (size_t(p->num_rows) + 1) * 4, entry_bytes = std::max<size_t>(size_t(p->nnz), 1) * 4, list_bytes = size_t(p->num_rows) * 4;
    const size_t cptr_bytes = (size_t(p->num_cols) + 1) * 4, clist_bytes = size_t(p->num_cols) * 4, dsum_bytes = size_t(p->num_rows) * 8;
    HSAB_HIP(p, p->ptr.alloc(ptr_bytes));
    HSAB_HIP(p, p->idx.alloc(entry_bytes));
    HSAB_HIP(p, p->list.alloc(list_bytes));
    HSAB_HIP(p, p->cptr.alloc(cptr_bytes));
    HSAB_HIP(p, p->crow.alloc(entry_bytes));
    HSAB_HIP(p, p->clist.alloc(clist_bytes));
    HSAB_HIP(p, p->dsum.alloc(dsum_bytes));
    p->device_bytes = ptr_bytes + entry_bytes + list_bytes + cptr_bytes + entry_bytes + clist_bytes + dsum_bytes;
    HSAB_HIP(p, hipMemcpyAsync(p->ptr.get(), indptr, ptr_bytes, hipMemcpyHostToDevice, p->own_stream));
    HSAB_HIP(p, hipMemcpyAsync(p->list.get(), list.data(), list_bytes, hipMemcpyHostToDevice, p->own_stream));
    HSAB_HIP(p, hipMemcpyAsync(p->cptr.get(), cptr.data(), cptr_bytes, hipMemcpyHostToDevice, p->own_stream));
    HSAB_HIP(p, hipMemcpyAsync(p->clist.get(), clist.data(), clist_bytes, hipMemcpyHostToDevice, p->own_stream));
    if (p->nnz) {
        HSAB_HIP(p, hipMemcpyAsync(p->idx.get(), indices, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
        HSAB_HIP(p, hipMemcpyAsync(p->crow.get(), crow.data(), size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    }
    HSAB_HIP(p, hipStreamSynchronize(p->own_stream));      // the host arrays (the caller's and the vectors here) are free again
    p->rows.ptr = p->ptr.get();
    p->rows.idx = p->idx.get();
    p->rows.list = p->list.get();
    p->cols.ptr = p->cptr.get();
    p->cols.idx = p->crow.get();
    p->cols.list = p->clist.get();
    p->rows.entries = p->cols.entries = p->nnz;
    return HS_OK;
}

// A dense host operand of n rows x d words on the device with ld = d rounded up to 4 (the pad words stay as allocated: loaded, never used)
int features_in(hsab_pattern* p, DeviceBuffer<float>& dev, const float* host, uint32_t n, uint32_t d, uint64_t ld) {
    HSAB_HIP(p, dev.alloc_count(size_t(n) * ld, 16));
    HSAB_HIP(p, hipMemcpy2DAsync(dev.get(), ld * 4, host, size_t(d) * 4, size_t(d) * 4, n, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

}  // namespace

extern "C" {

int hsab_create(hsab_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsab::check_create(num_rows, num_cols, indptr, indices, why)) return fail(nullptr, rc, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hsab_pattern* p = new (std::nothrow) hsab_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->nnz = indptr[num_rows];
    p->rows.compute_units = p->cols.compute_units = uint32_t(prop.multiProcessorCount);
    if (int rc = build(p, indptr, indices)) {
        g_create_error = p->error;
        if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
        delete p;
        return rc;
    }
    *out = p;
    return HS_OK;
}

int hsab_destroy(hsab_pattern* p) {
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

const char* hsab_last_error(const hsab_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsab_info(const hsab_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz;
    if (device_bytes) *device_bytes = p->device_bytes;
    return HS_OK;
}

int hsab_set_stream(hsab_pattern* p, void* hip_stream) {
    if (!p) return HS_ERR_BAD_ARG;
    p->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->own_stream;
    return HS_OK;
}

int hsab_sync(hsab_pattern* p) {
    if (int rc = enter(p)) return rc;
    HSAB_HIP(p, hipStreamSynchronize(p->stream));
    return HS_OK;
}

int hsab_backward_device(hsab_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                         const float* lse_dev, uint32_t d, float scale, float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsab::check_backward(p->num_rows, p->num_cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv,
                                                why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSAB_HIP(p, launch_attention_backward_rows(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, d, scale, gq_dev, ldgq, p->dsum.get(), p->stream));
    HSAB_HIP(p, launch_attention_backward_cols(p->cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, p->dsum.get(), d, scale, gk_dev, ldgk, gv_dev, ldgv, p->stream));
    return HS_OK;
}

int hsab_backward(hsab_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t d, float scale, float* gq, float* gk, float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsab::check_backward_host(p->num_rows, p->num_cols, q, k, v, gy, lse, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    DeviceBuffer<float> d_q, d_k, d_v, d_gy, d_lse, d_gq, d_gk, d_gv;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, d, ld)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, d, ld)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, d, ld)) return rc;
    if (int rc = features_in(p, d_gy, gy, p->num_rows, d, ld)) return rc;
    HSAB_HIP(p, d_lse.alloc_count(size_t(p->num_rows), 16));
    HSAB_HIP(p, hipMemcpyAsync(d_lse.get(), lse, size_t(p->num_rows) * 4, hipMemcpyHostToDevice, p->stream));
    HSAB_HIP(p, d_gq.alloc_count(size_t(p->num_rows) * ld, 16));
    HSAB_HIP(p, d_gk.alloc_count(size_t(p->num_cols) * ld, 16));
    HSAB_HIP(p, d_gv.alloc_count(size_t(p->num_cols) * ld, 16));
    int rc = hsab_backward_device(p, d_q.get(), ld, d_k.get(), ld, d_v.get(), ld, d_gy.get(), ld, d_lse.get(), d, scale, d_gq.get(), ld, d_gk.get(), ld, d_gv.get(), ld);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpy2DAsync(gq, size_t(d) * 4, d_gq.get(), size_t(ld) * 4, size_t(d) * 4, p->num_rows, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpy2DAsync(gk, size_t(d) * 4, d_gk.get(), size_t(ld) * 4, size_t(d) * 4, p->num_cols, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpy2DAsync(gv, size_t(d) * 4, d_gv.get(), size_t(ld) * 4, size_t(d) * 4, p->num_cols, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

}  // extern "C"
