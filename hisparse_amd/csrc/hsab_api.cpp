// hsab_api.cpp — include/hisparse_attention_backward.h on the HIP runtime: the pattern object of the fused attention backward step.  As
// hsat_api.cpp's, one object owns one device, one stream of its own and, from hsab_create on, all the device memory its _device call will
// ever use (device_buffer.h): the CSR arrays with the rows sorted into the length classes of wide_products.h (wide_schedule.h, which
// sorts and uploads a side), the transposed pattern (hsw_common.h's stable counting sort, WITHOUT its CSR-index map: there is no
// per-entry array to index) with the columns sorted the same way, and one double per row, the D words the first kernel writes and the
// second reads.  The kernels are in attention_backward.hip; what the object shares with the other pattern objects, and the host form's
// transient buffers, are pattern_object.h's.  Nothing here touches a context or another pattern object.
#include <new>
#include <string>
#include <vector>

#include "attention_backward.h"
#include "hsab_common.h"
#include "wide_schedule.h"

using namespace hisparse::dev;
using namespace hisparse::obj;

struct hsab_pattern : PatternObject {
    uint32_t num_rows = 0, num_cols = 0;
    WideSideBuffers rows, cols;      // the pattern and its rows by class; the transposed pattern and its columns by class
    DeviceBuffer<double> dsum;       // D per row: one backward call in flight per object
};

namespace {

// everything hsab_create does on the device; the caller destroys p when this fails
int build(hsab_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    if (int rc = open_stream(p)) return rc;
    if (int rc = upload_side(p, p->rows, p->num_rows, indptr, indices, false, nullptr)) return rc;
    std::vector<uint32_t> cptr, crow;
    {
        std::vector<uint32_t> perm;      // the CSR index of every entry in column order: built by the shared sort, not kept
        hisparse::hsw::build_transposed(p->num_rows, p->num_cols, indptr, indices, cptr, crow, perm);
    }
    if (int rc = upload_side(p, p->cols, p->num_cols, cptr.data(), crow.data(), false, nullptr)) return rc;
    const size_t dsum_bytes = size_t(p->num_rows) * 8;
    HS_HIP(p, p->dsum.alloc(dsum_bytes));
    p->device_bytes += dsum_bytes;
    return HS_OK;
}

}  // namespace

extern "C" {

int hsab_create(hsab_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices) {
    if (!out) return fail<hsab_pattern>(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    hipDeviceProp_t prop;
    if (int rc = hisparse::hsab::check_create(num_rows, num_cols, indptr, indices, why)) return fail<hsab_pattern>(nullptr, rc, why);
    if (int rc = probe_device(device_id, prop, why)) return fail<hsab_pattern>(nullptr, rc, why);
    hsab_pattern* p = new (std::nothrow) hsab_pattern;
    if (!p) return fail<hsab_pattern>(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->nnz = indptr[num_rows];
    p->rows.view.compute_units = p->cols.view.compute_units = uint32_t(prop.multiProcessorCount);
    return finish_create(out, p, build(p, indptr, indices));
}

int hsab_destroy(hsab_pattern* p) { return destroy(p); }
const char* hsab_last_error(const hsab_pattern* p) { return last_error(p); }
int hsab_info(const hsab_pattern* p, uint64_t* nnz, uint64_t* device_bytes) { return info(p, nnz, device_bytes); }
int hsab_set_stream(hsab_pattern* p, void* hip_stream) { return set_stream(p, hip_stream); }
int hsab_sync(hsab_pattern* p) { return sync(p); }

int hsab_backward_device(hsab_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                         const float* lse_dev, uint32_t d, float scale, float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsab::check_backward(p->num_rows, p->num_cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv,
                                                why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_attention_backward_rows(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, d, scale, gq_dev, ldgq, p->dsum.get(), p->stream));
    HS_HIP(p, launch_attention_backward_cols(p->cols.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, p->dsum.get(), d, scale, gk_dev, ldgk, gv_dev, ldgv, p->stream));
    return HS_OK;
}

int hsab_backward(hsab_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t d, float scale, float* gq, float* gk, float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsab::check_backward_host(p->num_rows, p->num_cols, q, k, v, gy, lse, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    Staging st(p);      // dense operands with ld = d rounded up to 4 (the pad words stay as allocated: loaded, never used)
    const float* d_q = st.in(q, p->num_rows, d, ld);
    const float* d_k = st.in(k, p->num_cols, d, ld);
    const float* d_v = st.in(v, p->num_cols, d, ld);
    const float* d_gy = st.in(gy, p->num_rows, d, ld);
    const float* d_lse = st.in(lse, p->num_rows, 1, 1);
    float* d_gq = st.out(gq, p->num_rows, d, ld);
    float* d_gk = st.out(gk, p->num_cols, d, ld);
    float* d_gv = st.out(gv, p->num_cols, d, ld);
    return st.finish(st.failed() ? st.failed() : hsab_backward_device(p, d_q, ld, d_k, ld, d_v, ld, d_gy, ld, d_lse, d, scale, d_gq, ld, d_gk, ld, d_gv, ld));
}

}  // extern "C"
