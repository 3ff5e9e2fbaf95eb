// hsp_api.cpp — include/hisparse_pattern.h on the HIP runtime: the pattern object of the sampled dense product.  One object owns one
// device, one stream of its own and, from hsp_create on, all the device memory it will ever use (device_buffer.h): the column and the
// row of every entry and the two staging buffers for max_k vectors.  The kernels are in sddmm.hip; what the object shares with the other
// pattern objects, and the host form's transient buffers, are pattern_object.h's.  Nothing here touches a context.
#include <new>
#include <string>

#include "hsp_common.h"
#include "pattern_object.h"
#include "sddmm.h"

using namespace hisparse::obj;

struct hsp_pattern : PatternObject {
    int impl = 0;
    uint32_t num_rows = 0, num_cols = 0, max_k = 0;
    uint32_t compute_units = 0;
    DeviceBuffer<uint32_t> row, col;      // per entry, CSR order
    DeviceBuffer<uint32_t> u4, v4;        // staging: ceil(max_k / 4) groups of num_rows (num_cols) x 4 words; none when max_k = 1
};

namespace {

using hisparse::hsp::round_up4;

// everything hsp_create does on the device; the caller destroys p when this fails
int build(hsp_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    if (int rc = open_stream(p)) return rc;
    const size_t entry_bytes = size_t(round_up4(p->nnz)) * 4;      // whole 16-byte words for the four-entry loads
    HS_HIP(p, p->row.alloc(std::max<size_t>(entry_bytes, 16)));
    HS_HIP(p, p->col.alloc(std::max<size_t>(entry_bytes, 16)));
    p->device_bytes = 2 * std::max<size_t>(entry_bytes, 16);
    if (p->max_k >= 2) {
        const size_t groups = (p->max_k + hisparse::hsp::kGroup - 1) / hisparse::hsp::kGroup;
        HS_HIP(p, p->u4.alloc(groups * p->num_rows * 16));
        HS_HIP(p, p->v4.alloc(groups * p->num_cols * 16));
        p->device_bytes += groups * (size_t(p->num_rows) + p->num_cols) * 16;
    }
    if (p->nnz == 0) return HS_OK;
    DeviceBuffer<uint32_t> d_indptr;      // needed by the expansion only
    HS_HIP(p, d_indptr.alloc_count(size_t(p->num_rows) + 1));
    HS_HIP(p, hipMemcpyAsync(d_indptr.get(), indptr, (size_t(p->num_rows) + 1) * 4, hipMemcpyHostToDevice, p->own_stream));
    HS_HIP(p, hipMemcpyAsync(p->col.get(), indices, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    HS_HIP(p, hisparse::dev::launch_expand_rows(d_indptr.get(), p->num_rows, p->nnz, p->row.get(), p->compute_units, p->own_stream));
    HS_HIP(p, hipStreamSynchronize(p->own_stream));      // the caller's arrays and d_indptr are free again
    return HS_OK;
}

}  // namespace

extern "C" {

int hsp_create(hsp_pattern** out, int device_id, int impl, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices,
               uint32_t max_k) {
    if (!out) return fail<hsp_pattern>(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    hipDeviceProp_t prop;
    if (int rc = hisparse::hsp::check_pattern(impl, num_rows, num_cols, indptr, indices, max_k, why)) return fail<hsp_pattern>(nullptr, rc, why);
    if (int rc = probe_device(device_id, prop, why)) return fail<hsp_pattern>(nullptr, rc, why);
    hsp_pattern* p = new (std::nothrow) hsp_pattern;
    if (!p) return fail<hsp_pattern>(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->impl = impl;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->max_k = max_k;
    p->nnz = indptr[num_rows];
    p->compute_units = uint32_t(prop.multiProcessorCount);
    return finish_create(out, p, build(p, indptr, indices));
}

int hsp_destroy(hsp_pattern* p) { return destroy(p); }
const char* hsp_last_error(const hsp_pattern* p) { return last_error(p); }
int hsp_info(const hsp_pattern* p, uint64_t* nnz, uint64_t* device_bytes) { return info(p, nnz, device_bytes); }
int hsp_set_stream(hsp_pattern* p, void* hip_stream) { return set_stream(p, hip_stream); }
int hsp_sync(hsp_pattern* p) { return sync(p); }

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
    HS_HIP(p, hisparse::dev::launch_sddmm(p->impl == HS_IMPL_FIXED, a, p->stream));
    return HS_OK;
}

int hsp_sddmm(hsp_pattern* p, const void* u, const void* v, uint32_t k, void* out) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!u || !v || !out) return fail(p, HS_ERR_BAD_ARG, "null argument");
    if (k < 1 || k > p->max_k) return fail(p, HS_ERR_BAD_ARG, "k must be 1 ... max_k (" + std::to_string(p->max_k) + ")");
    if (int rc = enter(p)) return rc;
    const uint64_t ldu = round_up4(p->num_rows), ldv = round_up4(p->num_cols);
    Staging st(p);      // u and v: k vectors of ld words, as large as they are; out: whole 16-byte words, nnz of them copied out
    const uint32_t* d_u = st.in(static_cast<const uint32_t*>(u), k, ldu, ldu, 0);
    const uint32_t* d_v = st.in(static_cast<const uint32_t*>(v), k, ldv, ldv, 0);
    uint32_t* d_out = st.out(static_cast<uint32_t*>(out), 1, p->nnz, round_up4(p->nnz));
    return st.finish(st.failed() ? st.failed() : hsp_sddmm_device(p, d_u, ldu, d_v, ldv, k, d_out, 0));
}

}  // extern "C"
