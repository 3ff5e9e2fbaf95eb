// hsat_api.cpp — include/hisparse_attention.h on the HIP runtime: the pattern object of the fused attention step.  As hsw_api.cpp's, one
// object owns one device, one stream of its own and, from hsat_create on, all the device memory its _device call will ever use
// (device_buffer.h): the CSR arrays and the rows sorted into the length classes of wide_products.h (wide_schedule.h, which sorts and
// uploads them).  The kernel is in pattern_attention.hip; what the object shares with the other pattern objects, and the host form's
// transient buffers, are pattern_object.h's.  Nothing here touches a context or another pattern object.
#include <new>
#include <string>

#include "hsat_common.h"
#include "pattern_attention.h"
#include "wide_schedule.h"

using namespace hisparse::dev;
using namespace hisparse::obj;

struct hsat_pattern : PatternObject {
    uint32_t num_rows = 0, num_cols = 0;
    WideSideBuffers rows;
};

namespace {

// everything hsat_create does on the device; the caller destroys p when this fails
int build(hsat_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    if (int rc = open_stream(p)) return rc;
    return upload_side(p, p->rows, p->num_rows, indptr, indices, false, nullptr);
}

}  // namespace

extern "C" {

int hsat_create(hsat_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices) {
    if (!out) return fail<hsat_pattern>(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    hipDeviceProp_t prop;
    if (int rc = hisparse::hsat::check_create(num_rows, num_cols, indptr, indices, why)) return fail<hsat_pattern>(nullptr, rc, why);
    if (int rc = probe_device(device_id, prop, why)) return fail<hsat_pattern>(nullptr, rc, why);
    hsat_pattern* p = new (std::nothrow) hsat_pattern;
    if (!p) return fail<hsat_pattern>(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->nnz = indptr[num_rows];
    p->rows.view.compute_units = uint32_t(prop.multiProcessorCount);
    return finish_create(out, p, build(p, indptr, indices));
}

int hsat_destroy(hsat_pattern* p) { return destroy(p); }
const char* hsat_last_error(const hsat_pattern* p) { return last_error(p); }
int hsat_info(const hsat_pattern* p, uint64_t* nnz, uint64_t* device_bytes) { return info(p, nnz, device_bytes); }
int hsat_set_stream(hsat_pattern* p, void* hip_stream) { return set_stream(p, hip_stream); }
int hsat_sync(hsat_pattern* p) { return sync(p); }

int hsat_forward_device(hsat_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, uint32_t d, float scale,
                        float* y_dev, uint64_t ldy, float* lse_dev) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsat::check_forward(p->num_rows, p->num_cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, d, scale, y_dev, ldy, lse_dev, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_pattern_attention(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, d, scale, y_dev, ldy, lse_dev, p->stream));
    return HS_OK;
}

int hsat_forward(hsat_pattern* p, const float* q, const float* k, const float* v, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsat::check_forward_host(p->num_rows, p->num_cols, q, k, v, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    Staging st(p);      // dense operands with ld = d rounded up to 4 (the pad words stay as allocated: loaded, never used)
    const float* d_q = st.in(q, p->num_rows, d, ld);
    const float* d_k = st.in(k, p->num_cols, d, ld);
    const float* d_v = st.in(v, p->num_cols, d, ld);
    float* d_y = st.out(y, p->num_rows, d, ld);
    float* d_lse = st.out(lse, p->num_rows, 1, 1);
    return st.finish(st.failed() ? st.failed() : hsat_forward_device(p, d_q, ld, d_k, ld, d_v, ld, d, scale, d_y, ld, d_lse));
}

}  // extern "C"
