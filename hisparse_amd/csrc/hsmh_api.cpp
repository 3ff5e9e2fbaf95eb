// hsmh_api.cpp — include/hisparse_heads.h on the HIP runtime: the pattern object of the multi-head attention step, forward and backward.
// As hsat_api.cpp's and hsab_api.cpp's, one object owns one device, one stream of its own and, from hsmh_create on, all the device
// memory its _device calls will ever use (device_buffer.h): the CSR arrays with the rows sorted into the length classes of
// wide_products.h (wide_schedule.h) and, with HSMH_BACKWARD, the transposed pattern (hsw_common.h's stable counting sort, without its
// CSR-index map) with the columns sorted the same way and max_heads doubles per row, the D words the row kernel writes and the column
// kernel reads.  The kernels are in heads_attention.hip.  Nothing here touches a context or another pattern object.
// The four hsmh16_* calls of include/hisparse_heads_bf16.h work on the same object with bf16 operands (heads16_attention.hip): the same
// pattern, transposed pattern, D words and stream, nothing held twice.
// The five hsmhb_* calls of include/hisparse_heads_bias.h add a per-entry, per-head bias (heads_bias_attention.hip).  hsmhb_create is
// hsmh_create that, with HSMH_BACKWARD, also keeps the shared sort's CSR-index map on the device (4 max(nnz, 1) bytes more): the column
// side of the backward finds an entry's bias words and stores its gbias words through it.  hsmh_create builds the map and drops it.
// The five hsmhd_* calls of include/hisparse_heads_dropout.h add dropout on the attention weights, with or without a bias
// (heads_dropout_attention.hip): no new object and no memory; the backward keys its column side's draws through the same map.
// The four hsgat_* calls of include/hisparse_gat.h run the graph attention (GAT) step on the same object (gat_attention.hip): additive
// scores from one word per node and head, the same pattern, transposed pattern, D words and stream, no map and no memory of their own.
// The six hsgat2_* calls of include/hisparse_gatv2.h run the GATv2 step on the same object (gatv2_attention.hip): the score is
// a . LeakyReLU(XD[row] + XS[col]); the backward's third launch adds the row side's per-workgroup vectors of ga, which live in a
// workspace the CALLER owns (hsgat2_work_bytes), so the object still allocates nothing outside create.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "gat_attention.h"
#include "gatv2_attention.h"
#include "heads16_attention.h"
#include "heads_attention.h"
#include "heads_bias_attention.h"
#include "heads_dropout_attention.h"
#include "hisparse_gat.h"
#include "hisparse_gatv2.h"
#include "hisparse_heads_bf16.h"
#include "hisparse_heads_bias.h"
#include "hisparse_heads_dropout.h"
#include "hsmh_common.h"
#include "wide_schedule.h"

using namespace hisparse::dev;

struct hsmh_pattern {
    int device = 0;
    uint32_t num_rows = 0, num_cols = 0, max_heads = 0;
    bool backward = false;
    bool map = false;      // hsmhb_create with HSMH_BACKWARD: perm is kept
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DeviceBuffer<uint32_t> ptr, idx, list;         // the pattern and its rows by class
    DeviceBuffer<uint32_t> cptr, crow, clist;      // with HSMH_BACKWARD: the transposed pattern and its columns by class
    DeviceBuffer<uint32_t> perm;                   // with the map: the CSR index of every entry of the transposed pattern
    DeviceBuffer<double> dsum;                     // with HSMH_BACKWARD: D per row and head, [row][max_heads]: one backward call in flight per object
    WideSide rows, cols;
    std::string error;
};

namespace {

thread_local std::string g_create_error;

int fail(hsmh_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}
int hip_fail(hsmh_pattern* p, hipError_t e, const char* what) { return fail(p, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

#define HSMH_HIP(p, call)                                             \
    do {                                                              \
        const hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail((p), e_, #call);        \
    } while (0)

int enter(hsmh_pattern* p) {
    if (!p) return HS_ERR_BAD_ARG;
    HSMH_HIP(p, hipSetDevice(p->device));
    return HS_OK;
}

// everything hsmh_create does on the device; the caller destroys p when this fails
int build(hsmh_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    HSMH_HIP(p, hipSetDevice(p->device));
    HSMH_HIP(p, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    p->stream = p->own_stream;
    std::vector<uint32_t> list;
    schedule(p->num_rows, indptr, list, p->rows.count);
    const size_t ptr_bytes = (size_t(p->num_rows) + 1) * 4, entry_bytes = std::max<size_t>(size_t(p->nnz), 1) * 4, list_bytes = size_t(p->num_rows) * 4;
    HSMH_HIP(p, p->ptr.alloc(ptr_bytes));
    HSMH_HIP(p, p->idx.alloc(entry_bytes));
    HSMH_HIP(p, p->list.alloc(list_bytes));
    p->device_bytes = ptr_bytes + entry_bytes + list_bytes;
    HSMH_HIP(p, hipMemcpyAsync(p->ptr.get(), indptr, ptr_bytes, hipMemcpyHostToDevice, p->own_stream));
    HSMH_HIP(p, hipMemcpyAsync(p->list.get(), list.data(), list_bytes, hipMemcpyHostToDevice, p->own_stream));
    if (p->nnz) HSMH_HIP(p, hipMemcpyAsync(p->idx.get(), indices, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    std::vector<uint32_t> cptr, crow, clist, perm;      // alive until the synchronisation below
    if (p->backward) {
        hisparse::hsw::build_transposed(p->num_rows, p->num_cols, indptr, indices, cptr, crow, perm);      // perm: the CSR index of every entry in column order
        if (!p->map) std::vector<uint32_t>().swap(perm);                                                      // built by the shared sort, kept for hsmhb_create only
        schedule(p->num_cols, cptr.data(), clist, p->cols.count);
        const size_t cptr_bytes = (size_t(p->num_cols) + 1) * 4, clist_bytes = size_t(p->num_cols) * 4, dsum_bytes = size_t(p->num_rows) * p->max_heads * 8;
        HSMH_HIP(p, p->cptr.alloc(cptr_bytes));
        HSMH_HIP(p, p->crow.alloc(entry_bytes));
        HSMH_HIP(p, p->clist.alloc(clist_bytes));
        HSMH_HIP(p, p->dsum.alloc(dsum_bytes));
        p->device_bytes += cptr_bytes + entry_bytes + clist_bytes + dsum_bytes;
        HSMH_HIP(p, hipMemcpyAsync(p->cptr.get(), cptr.data(), cptr_bytes, hipMemcpyHostToDevice, p->own_stream));
        HSMH_HIP(p, hipMemcpyAsync(p->clist.get(), clist.data(), clist_bytes, hipMemcpyHostToDevice, p->own_stream));
        if (p->nnz) HSMH_HIP(p, hipMemcpyAsync(p->crow.get(), crow.data(), size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
        if (p->map) {
            HSMH_HIP(p, p->perm.alloc(entry_bytes));
            p->device_bytes += entry_bytes;
            if (p->nnz) HSMH_HIP(p, hipMemcpyAsync(p->perm.get(), perm.data(), size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
        }
    }
    HSMH_HIP(p, hipStreamSynchronize(p->own_stream));      // the host arrays (the caller's and the vectors here) are free again
    p->rows.ptr = p->ptr.get();
    p->rows.idx = p->idx.get();
    p->rows.list = p->list.get();
    p->cols.ptr = p->cptr.get();
    p->cols.idx = p->crow.get();
    p->cols.list = p->clist.get();
    p->cols.perm = p->map ? p->perm.get() : nullptr;      // read by the kernels of heads_bias_attention.hip only
    p->rows.entries = p->cols.entries = p->nnz;
    return HS_OK;
}

// A dense host operand of n rows x w words on the device, ld = w (a multiple of 4)
int features_in(hsmh_pattern* p, DeviceBuffer<float>& dev, const float* host, uint32_t n, uint32_t w) {
    HSMH_HIP(p, dev.alloc_count(size_t(n) * w, 16));
    HSMH_HIP(p, hipMemcpyAsync(dev.get(), host, size_t(n) * w * 4, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

// The same for bf16 elements, ld = w (a multiple of 8)
int features16_in(hsmh_pattern* p, DeviceBuffer<uint16_t>& dev, const uint16_t* host, uint32_t n, uint32_t w) {
    HSMH_HIP(p, dev.alloc_count(size_t(n) * w, 16));
    HSMH_HIP(p, hipMemcpyAsync(dev.get(), host, size_t(n) * w * 2, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

// A per-entry host array of nnz x heads words on the device, ld = heads (a word at least, so that the pointer is never null)
int entries_in(hsmh_pattern* p, DeviceBuffer<float>& dev, const float* host, uint32_t heads) {
    HSMH_HIP(p, dev.alloc_count(std::max<size_t>(size_t(p->nnz) * heads, 1), 16));
    if (p->nnz) HSMH_HIP(p, hipMemcpyAsync(dev.get(), host, size_t(p->nnz) * heads * 4, hipMemcpyHostToDevice, p->stream));
    return HS_OK;
}

// hsmh_create and hsmhb_create: keep_map asks for the entry map beside the transposed pattern
int create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags, bool keep_map) {
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsmh::check_create(num_rows, num_cols, indptr, indices, max_heads, flags, why)) return fail(nullptr, rc, why);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(nullptr, HS_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, HS_ERR_BAD_ARG, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    hsmh_pattern* p = new (std::nothrow) hsmh_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->max_heads = max_heads;
    p->backward = (flags & HSMH_BACKWARD) != 0;
    p->map = keep_map && p->backward;
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

}  // namespace

extern "C" {

int hsmh_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags) {
    return create(out, device_id, num_rows, num_cols, indptr, indices, max_heads, flags, false);
}

int hsmh_destroy(hsmh_pattern* p) {
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

const char* hsmh_last_error(const hsmh_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsmh_info(const hsmh_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz;
    if (device_bytes) *device_bytes = p->device_bytes;
    return HS_OK;
}

int hsmh_set_stream(hsmh_pattern* p, void* hip_stream) {
    if (!p) return HS_ERR_BAD_ARG;
    p->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->own_stream;
    return HS_OK;
}

int hsmh_sync(hsmh_pattern* p) {
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, hipStreamSynchronize(p->stream));
    return HS_OK;
}

int hsmh_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d, float scale,
                        float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward(p->num_rows, p->num_cols, p->max_heads, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_heads_forward(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmh_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, uint32_t heads, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_host(p->num_rows, p->num_cols, p->max_heads, q, k, v, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_q, d_k, d_v, d_y, d_lse;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    HSMH_HIP(p, d_y.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_lse.alloc_count(size_t(p->num_rows) * heads, 16));
    int rc = hsmh_forward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, heads, d, scale, d_y.get(), w, lse ? d_lse.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(y, d_y.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

int hsmh_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                         const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float scale, float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev,
                         uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward(p->num_rows, p->num_cols, p->max_heads, p->backward, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale,
                                                gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_heads_backward_rows(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                           p->stream));
    HSMH_HIP(p, launch_heads_backward_cols(p->cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, scale, gk_dev, ldgk, gv_dev,
                                           ldgv, p->stream));
    return HS_OK;
}

int hsmh_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t heads, uint32_t d, float scale, float* gq, float* gk,
                  float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_host(p->num_rows, p->num_cols, p->max_heads, p->backward, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_q, d_k, d_v, d_gy, d_lse, d_gq, d_gk, d_gv;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_gy, gy, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_lse, lse, p->num_rows, heads)) return rc;
    HSMH_HIP(p, d_gq.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_gk.alloc_count(size_t(p->num_cols) * w, 16));
    HSMH_HIP(p, d_gv.alloc_count(size_t(p->num_cols) * w, 16));
    int rc = hsmh_backward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, d_gy.get(), w, d_lse.get(), heads, heads, d, scale, d_gq.get(), w, d_gk.get(), w, d_gv.get(), w);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(gq, d_gq.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gk, d_gk.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gv, d_gv.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// ---- include/hisparse_heads_bf16.h: the same object, bf16 operands ----------------------------------------------------------------------
int hsmh16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                          float scale, uint16_t* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward16(p->num_rows, p->num_cols, p->max_heads, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_heads16_forward(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmh16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint32_t heads, uint32_t d, float scale, uint16_t* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward16_host(p->num_rows, p->num_cols, p->max_heads, q, k, v, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<uint16_t> d_q, d_k, d_v, d_y;      // transient (the host form is synchronous and may allocate)
    DeviceBuffer<float> d_lse;
    if (int rc = features16_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features16_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features16_in(p, d_v, v, p->num_cols, w)) return rc;
    HSMH_HIP(p, d_y.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_lse.alloc_count(size_t(p->num_rows) * heads, 16));
    int rc = hsmh16_forward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, heads, d, scale, d_y.get(), w, lse ? d_lse.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(y, d_y.get(), size_t(p->num_rows) * w * 2, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

int hsmh16_backward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const uint16_t* gy_dev,
                           uint64_t ldgy, const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float scale, uint16_t* gq_dev, uint64_t ldgq, uint16_t* gk_dev, uint64_t ldgk,
                           uint16_t* gv_dev, uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward16(p->num_rows, p->num_cols, p->max_heads, p->backward, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale,
                                                  gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_heads16_backward_rows(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                             p->stream));
    HSMH_HIP(p, launch_heads16_backward_cols(p->cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, scale, gk_dev, ldgk,
                                             gv_dev, ldgv, p->stream));
    return HS_OK;
}

int hsmh16_backward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy, const float* lse, uint32_t heads, uint32_t d, float scale,
                    uint16_t* gq, uint16_t* gk, uint16_t* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward16_host(p->num_rows, p->num_cols, p->max_heads, p->backward, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<uint16_t> d_q, d_k, d_v, d_gy, d_gq, d_gk, d_gv;      // transient (the host form is synchronous and may allocate)
    DeviceBuffer<float> d_lse;
    if (int rc = features16_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features16_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features16_in(p, d_v, v, p->num_cols, w)) return rc;
    if (int rc = features16_in(p, d_gy, gy, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_lse, lse, p->num_rows, heads)) return rc;
    HSMH_HIP(p, d_gq.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_gk.alloc_count(size_t(p->num_cols) * w, 16));
    HSMH_HIP(p, d_gv.alloc_count(size_t(p->num_cols) * w, 16));
    int rc = hsmh16_backward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, d_gy.get(), w, d_lse.get(), heads, heads, d, scale, d_gq.get(), w, d_gk.get(), w, d_gv.get(), w);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(gq, d_gq.get(), size_t(p->num_rows) * w * 2, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gk, d_gk.get(), size_t(p->num_cols) * w * 2, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gv, d_gv.get(), size_t(p->num_cols) * w * 2, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// ---- include/hisparse_heads_bias.h: the same object, a bias per entry and head ----------------------------------------------------------
int hsmhb_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags) {
    return create(out, device_id, num_rows, num_cols, indptr, indices, max_heads, flags, true);
}

int hsmhb_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* bias_dev, uint64_t ldb,
                         uint32_t heads, uint32_t d, float scale, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_bias(p->num_rows, p->num_cols, p->max_heads, p->nnz, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, y_dev, ldy,
                                                    lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_biased_forward(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmhb_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias, uint32_t heads, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_bias_host(p->num_rows, p->num_cols, p->max_heads, p->nnz, q, k, v, bias, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_q, d_k, d_v, d_b, d_y, d_lse;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    if (int rc = entries_in(p, d_b, bias, heads)) return rc;
    HSMH_HIP(p, d_y.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_lse.alloc_count(size_t(p->num_rows) * heads, 16));
    int rc = hsmhb_forward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, d_b.get(), heads, heads, d, scale, d_y.get(), w, lse ? d_lse.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(y, d_y.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

int hsmhb_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float* gq_dev, uint64_t ldgq,
                          float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv, float* gbias_dev, uint64_t ldgb) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_bias(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev, ldb,
                                                     heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, gbias_dev, ldgb, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_biased_rows(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev, ldb, heads, d, scale, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                   p->stream));
    HSMH_HIP(p, launch_biased_cols(p->cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, bias_dev, ldb, heads, d, scale, gk_dev, ldgk,
                                   gv_dev, ldgv, gbias_dev, ldgb, p->stream));
    return HS_OK;
}

int hsmhb_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale,
                   float* gq, float* gk, float* gv, float* gbias) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_bias_host(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz, q, k, v, gy, lse, bias, heads, d, scale, gq, gk, gv, gbias, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_q, d_k, d_v, d_gy, d_lse, d_b, d_gq, d_gk, d_gv, d_gb;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_gy, gy, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_lse, lse, p->num_rows, heads)) return rc;
    if (int rc = entries_in(p, d_b, bias, heads)) return rc;
    HSMH_HIP(p, d_gq.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_gk.alloc_count(size_t(p->num_cols) * w, 16));
    HSMH_HIP(p, d_gv.alloc_count(size_t(p->num_cols) * w, 16));
    if (gbias) HSMH_HIP(p, d_gb.alloc_count(std::max<size_t>(size_t(p->nnz) * heads, 1), 16));
    int rc = hsmhb_backward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, d_gy.get(), w, d_lse.get(), heads, d_b.get(), heads, heads, d, scale, d_gq.get(), w, d_gk.get(), w,
                                   d_gv.get(), w, gbias ? d_gb.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(gq, d_gq.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gk, d_gk.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gv, d_gv.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && gbias && p->nnz) e = hipMemcpyAsync(gbias, d_gb.get(), size_t(p->nnz) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// ---- include/hisparse_heads_dropout.h: the same object, dropout on the attention weights, a bias or none ----------------------------------
int hsmhd_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* bias_dev, uint64_t ldb,
                         uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout(p->num_rows, p->num_cols, p->max_heads, p->nnz, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, drop_p, y_dev,
                                                       ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_dropout_forward(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, hisparse::philox::dropout_of(drop_p, seed, offset), y_dev, ldy,
                                       lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmhd_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed,
                  uint64_t offset, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout_host(p->num_rows, p->num_cols, p->max_heads, p->nnz, q, k, v, bias, heads, d, scale, drop_p, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_q, d_k, d_v, d_b, d_y, d_lse;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    if (bias)
        if (int rc = entries_in(p, d_b, bias, heads)) return rc;
    HSMH_HIP(p, d_y.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_lse.alloc_count(size_t(p->num_rows) * heads, 16));
    int rc = hsmhd_forward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, bias ? d_b.get() : nullptr, heads, heads, d, scale, drop_p, seed, offset, d_y.get(), w,
                                  lse ? d_lse.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(y, d_y.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

int hsmhd_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset,
                          float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv, float* gbias_dev, uint64_t ldgb) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev,
                                                        ldb, heads, d, scale, drop_p, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, gbias_dev, ldgb, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    HSMH_HIP(p, launch_dropout_rows(p->rows, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev, ldb, heads, d, scale, dr, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                    p->stream));
    HSMH_HIP(p, launch_dropout_cols(p->cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, bias_dev, ldb, heads, d, scale, dr, gk_dev, ldgk,
                                    gv_dev, ldgv, gbias_dev, ldgb, p->stream));
    return HS_OK;
}

int hsmhd_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale,
                   float drop_p, uint64_t seed, uint64_t offset, float* gq, float* gk, float* gv, float* gbias) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout_host(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz, q, k, v, gy, lse, bias, heads, d, scale, drop_p, gq, gk, gv, gbias,
                                                             why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_q, d_k, d_v, d_gy, d_lse, d_b, d_gq, d_gk, d_gv, d_gb;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_q, q, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_k, k, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_gy, gy, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_lse, lse, p->num_rows, heads)) return rc;
    if (bias)
        if (int rc = entries_in(p, d_b, bias, heads)) return rc;
    HSMH_HIP(p, d_gq.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_gk.alloc_count(size_t(p->num_cols) * w, 16));
    HSMH_HIP(p, d_gv.alloc_count(size_t(p->num_cols) * w, 16));
    if (gbias) HSMH_HIP(p, d_gb.alloc_count(std::max<size_t>(size_t(p->nnz) * heads, 1), 16));
    int rc = hsmhd_backward_device(p, d_q.get(), w, d_k.get(), w, d_v.get(), w, d_gy.get(), w, d_lse.get(), heads, bias ? d_b.get() : nullptr, heads, heads, d, scale, drop_p, seed, offset,
                                   d_gq.get(), w, d_gk.get(), w, d_gv.get(), w, gbias ? d_gb.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(gq, d_gq.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gk, d_gk.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gv, d_gv.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && gbias && p->nnz) e = hipMemcpyAsync(gbias, d_gb.get(), size_t(p->nnz) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// host code: no object, no device
int hsmhd_keep_mask(uint64_t nnz, uint32_t heads, float drop_p, uint64_t seed, uint64_t offset, uint8_t* keep) { return hisparse::hsmh::keep_mask(nnz, heads, drop_p, seed, offset, keep); }

// ---- include/hisparse_gat.h: the same object, additive (GAT) scores from one word per node and head ---------------------------------------
int hsgat_forward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                         float slope, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_forward(p->num_rows, p->num_cols, p->max_heads, el_dev, ldel, er_dev, lder, v_dev, ldv, heads, d, slope, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_gat_forward(p->rows, el_dev, ldel, er_dev, lder, v_dev, ldv, heads, d, slope, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsgat_forward(hsmh_pattern* p, const float* el, const float* er, const float* v, uint32_t heads, uint32_t d, float slope, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_forward_host(p->num_rows, p->num_cols, p->max_heads, el, er, v, heads, d, slope, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_el, d_er, d_v, d_y, d_lse;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_el, el, p->num_rows, heads)) return rc;
    if (int rc = features_in(p, d_er, er, p->num_cols, heads)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    HSMH_HIP(p, d_y.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_lse.alloc_count(size_t(p->num_rows) * heads, 16));
    int rc = hsgat_forward_device(p, d_el.get(), heads, d_er.get(), heads, d_v.get(), w, heads, d, slope, d_y.get(), w, lse ? d_lse.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(y, d_y.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

int hsgat_backward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gel_dev, uint64_t ldgel, float* ger_dev, uint64_t ldger, float* gv_dev,
                          uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_backward(p->num_rows, p->num_cols, p->max_heads, p->backward, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d,
                                                    slope, gel_dev, ldgel, ger_dev, ldger, gv_dev, ldgv, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_gat_backward_rows(p->rows, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, slope, gel_dev, ldgel, p->dsum.get(), p->max_heads,
                                         p->stream));
    HSMH_HIP(p, launch_gat_backward_cols(p->cols, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, slope, ger_dev, ldger,
                                         gv_dev, ldgv, p->stream));
    return HS_OK;
}

int hsgat_backward(hsmh_pattern* p, const float* el, const float* er, const float* v, const float* gy, const float* lse, uint32_t heads, uint32_t d, float slope, float* gel,
                   float* ger, float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_backward_host(p->num_rows, p->num_cols, p->max_heads, p->backward, el, er, v, gy, lse, heads, d, slope, gel, ger, gv, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_el, d_er, d_v, d_gy, d_lse, d_gel, d_ger, d_gv;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_el, el, p->num_rows, heads)) return rc;
    if (int rc = features_in(p, d_er, er, p->num_cols, heads)) return rc;
    if (int rc = features_in(p, d_v, v, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_gy, gy, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_lse, lse, p->num_rows, heads)) return rc;
    HSMH_HIP(p, d_gel.alloc_count(size_t(p->num_rows) * heads, 16));
    HSMH_HIP(p, d_ger.alloc_count(size_t(p->num_cols) * heads, 16));
    HSMH_HIP(p, d_gv.alloc_count(size_t(p->num_cols) * w, 16));
    int rc = hsgat_backward_device(p, d_el.get(), heads, d_er.get(), heads, d_v.get(), w, d_gy.get(), w, d_lse.get(), heads, heads, d, slope, d_gel.get(), heads, d_ger.get(), heads,
                                   d_gv.get(), w);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(gel, d_gel.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ger, d_ger.get(), size_t(p->num_cols) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gv, d_gv.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// ---- include/hisparse_gatv2.h: the same object, the score a . LeakyReLU(XD[row] + XS[col]) and the gradient of a ---------------------------
int hsgat2_forward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev, uint32_t heads, uint32_t d, float slope,
                          float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_forward(p->num_rows, p->num_cols, p->max_heads, xd_dev, ldxd, xs_dev, ldxs, a_dev, heads, d, slope, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HSMH_HIP(p, launch_gatv2_forward(p->rows, xd_dev, ldxd, xs_dev, ldxs, a_dev, heads, d, slope, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsgat2_forward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, uint32_t heads, uint32_t d, float slope, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_forward_host(p->num_rows, p->num_cols, p->max_heads, xd, xs, a, heads, d, slope, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    DeviceBuffer<float> d_xd, d_xs, d_a, d_y, d_lse;      // transient (the host form is synchronous and may allocate)
    if (int rc = features_in(p, d_xd, xd, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_xs, xs, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_a, a, 1, w)) return rc;
    HSMH_HIP(p, d_y.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_lse.alloc_count(size_t(p->num_rows) * heads, 16));
    int rc = hsgat2_forward_device(p, d_xd.get(), w, d_xs.get(), w, d_a.get(), heads, d, slope, d_y.get(), w, lse ? d_lse.get() : nullptr, heads);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(y, d_y.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess && lse) e = hipMemcpyAsync(lse, d_lse.get(), size_t(p->num_rows) * heads * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

// one vector of heads * d doubles per physical workgroup of the row side's launch
int hsgat2_work_bytes(const hsmh_pattern* p, uint32_t heads, uint32_t d, uint64_t* bytes) {
    if (!p || !bytes) return HS_ERR_BAD_ARG;
    std::string why;
    if (hisparse::hsmh::check_shape(heads, d, p->max_heads, why)) return HS_ERR_BAD_ARG;      // p is const: the reason is check_shape's, as the calls report it
    *bytes = uint64_t(gatv2_row_vectors(p->rows, heads, d)) * heads * d * 8;
    return HS_OK;
}

int hsgat2_backward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev, const float* gy_dev, uint64_t ldgy,
                           const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gxd_dev, uint64_t ldgxd, float* gxs_dev, uint64_t ldgxs, float* ga_dev,
                           void* work_dev, uint64_t work_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    uint64_t need = 0;
    (void)hsgat2_work_bytes(p, heads, d, &need);      // a bad shape leaves 0 and is refused by the checks below, with its reason
    if (int rc = hisparse::hsmh::check_gat2_backward(p->num_rows, p->num_cols, p->max_heads, p->backward, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, heads, d, slope,
                                                     gxd_dev, ldgxd, gxs_dev, ldgxs, ga_dev, work_dev, work_bytes, need, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    double* work = static_cast<double*>(work_dev);
    HSMH_HIP(p, launch_gatv2_backward_rows(p->rows, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, heads, d, slope, gxd_dev, ldgxd, p->dsum.get(), p->max_heads, work,
                                           p->stream));
    HSMH_HIP(p, launch_gatv2_backward_cols(p->cols, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, slope, gxs_dev, ldgxs,
                                           p->stream));
    HSMH_HIP(p, launch_gatv2_reduce(work, gatv2_row_vectors(p->rows, heads, d), heads * d, ga_dev, p->stream));
    return HS_OK;
}

int hsgat2_backward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, const float* gy, const float* lse, uint32_t heads, uint32_t d, float slope, float* gxd,
                    float* gxs, float* ga) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_backward_host(p->num_rows, p->num_cols, p->max_heads, p->backward, xd, xs, a, gy, lse, heads, d, slope, gxd, gxs, ga, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    uint64_t work_bytes = 0;
    if (hsgat2_work_bytes(p, heads, d, &work_bytes)) return fail(p, HS_ERR_BAD_ARG, "hsgat2_work_bytes refused a shape the checks accepted");
    DeviceBuffer<float> d_xd, d_xs, d_a, d_gy, d_lse, d_gxd, d_gxs, d_ga;      // transient (the host form is synchronous and may allocate)
    DeviceBuffer<double> d_work;
    if (int rc = features_in(p, d_xd, xd, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_xs, xs, p->num_cols, w)) return rc;
    if (int rc = features_in(p, d_a, a, 1, w)) return rc;
    if (int rc = features_in(p, d_gy, gy, p->num_rows, w)) return rc;
    if (int rc = features_in(p, d_lse, lse, p->num_rows, heads)) return rc;
    HSMH_HIP(p, d_gxd.alloc_count(size_t(p->num_rows) * w, 16));
    HSMH_HIP(p, d_gxs.alloc_count(size_t(p->num_cols) * w, 16));
    HSMH_HIP(p, d_ga.alloc_count(w, 16));
    HSMH_HIP(p, d_work.alloc_count(size_t(work_bytes / 8), 16));
    int rc = hsgat2_backward_device(p, d_xd.get(), w, d_xs.get(), w, d_a.get(), d_gy.get(), w, d_lse.get(), heads, heads, d, slope, d_gxd.get(), w, d_gxs.get(), w, d_ga.get(),
                                    d_work.get(), work_bytes);
    // copy out when all went well, always wait before the transient buffers go
    if (rc == HS_OK) {
        hipError_t e = hipMemcpyAsync(gxd, d_gxd.get(), size_t(p->num_rows) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gxs, d_gxs.get(), size_t(p->num_cols) * w * 4, hipMemcpyDeviceToHost, p->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ga, d_ga.get(), size_t(w) * 4, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) rc = hip_fail(p, e, "copying the result out");
    }
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p, e, "hipStreamSynchronize");
    return rc;
}

}  // extern "C"
