// hsw_api.cpp — include/hisparse_wide.h on the HIP runtime: the pattern object of the row-major feature products.  One object owns one
// device, one stream of its own and, from hsw_create on, all the device memory its _device calls will ever use (device_buffer.h): the CSR
// arrays, the rows sorted into length classes (wide_products.h) and, with HSW_TRANSPOSED, the same three for the transposed pattern plus
// the map from its entries back to CSR order.  Both schedules and the transposed pattern are built on the host (wide_schedule.h, which
// also uploads a side; hsw_common.h); the kernels are in wide_products.hip; what the object shares with the other pattern objects, and
// the host forms' transient buffers, are pattern_object.h's.  Nothing here touches a context, an hsp_pattern or a numeric mode.
// The four calls of include/hisparse_aggregate.h (hsagg_*: sum, mean, max and min of the neighbours' rows, and their backward) work on
// the same object and are at the end of this file; their kernels are in neighbor_aggregate.hip.
#include <new>
#include <string>
#include <vector>

#include "hsw_common.h"
#include "neighbor_aggregate.h"
#include "wide_products.h"
#include "wide_schedule.h"

using namespace hisparse::dev;
using namespace hisparse::obj;

struct hsw_pattern : PatternObject {
    uint32_t num_rows = 0, num_cols = 0;
    bool transposed = false;
    WideSideBuffers rows, cols;      // cols: the transposed pattern (HSW_TRANSPOSED)
};

namespace {

// everything hsw_create does on the device; the caller destroys p when this fails
int build(hsw_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    if (int rc = open_stream(p)) return rc;
    if (int rc = upload_side(p, p->rows, p->num_rows, indptr, indices, false, nullptr)) return rc;
    if (p->transposed) {
        std::vector<uint32_t> cptr, row, perm;
        hisparse::hsw::build_transposed(p->num_rows, p->num_cols, indptr, indices, cptr, row, perm);
        if (int rc = upload_side(p, p->cols, p->num_cols, cptr.data(), row.data(), true, perm.data())) return rc;
    }
    return HS_OK;
}

// hsw_spmm (side = rows) and hsw_spmm_t (side = cols) after their checks
int spmm_host(hsw_pattern* p, bool transposed, const float* w, const float* x, uint32_t d, float* y) {
    const uint32_t y_rows = transposed ? p->num_cols : p->num_rows, x_rows = transposed ? p->num_rows : p->num_cols;
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, w, p->nnz, x, uint64_t(x_rows) * d, y, uint64_t(y_rows) * d, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    Staging st(p);      // dense operands with ld = d rounded up to 4 (the pad words stay as allocated: loaded, never used)
    const float* d_w = st.in(w, 1, p->nnz, p->nnz);
    const float* d_x = st.in(x, x_rows, d, ld);
    float* d_y = st.out(y, y_rows, d, ld);
    return st.finish(st.failed() ? st.failed() : transposed ? hsw_spmm_t_device(p, d_w, d_x, ld, d, d_y, ld) : hsw_spmm_device(p, d_w, d_x, ld, d, d_y, ld));
}

// the bits of a checked `ops` word (hisparse_aggregate.h) as the launchers take them
AggregateOps aggregators(uint32_t ops) {
    AggregateOps a;
    a.sum = (ops & HSAGG_SUM) != 0;
    a.mean = (ops & HSAGG_MEAN) != 0;
    a.max = (ops & HSAGG_MAX) != 0;
    a.min = (ops & HSAGG_MIN) != 0;
    return a;
}

}  // namespace

extern "C" {

int hsw_create(hsw_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t flags) {
    if (!out) return fail<hsw_pattern>(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    hipDeviceProp_t prop;
    if (int rc = hisparse::hsw::check_create(num_rows, num_cols, indptr, indices, flags, why)) return fail<hsw_pattern>(nullptr, rc, why);
    if (int rc = probe_device(device_id, prop, why)) return fail<hsw_pattern>(nullptr, rc, why);
    hsw_pattern* p = new (std::nothrow) hsw_pattern;
    if (!p) return fail<hsw_pattern>(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->nnz = indptr[num_rows];
    p->rows.view.compute_units = p->cols.view.compute_units = uint32_t(prop.multiProcessorCount);
    p->transposed = (flags & HSW_TRANSPOSED) != 0;
    return finish_create(out, p, build(p, indptr, indices));
}

int hsw_destroy(hsw_pattern* p) { return destroy(p); }
const char* hsw_last_error(const hsw_pattern* p) { return last_error(p); }
int hsw_info(const hsw_pattern* p, uint64_t* nnz, uint64_t* device_bytes) { return info(p, nnz, device_bytes); }
int hsw_set_stream(hsw_pattern* p, void* hip_stream) { return set_stream(p, hip_stream); }
int hsw_sync(hsw_pattern* p) { return sync(p); }

int hsw_sddmm_device(hsw_pattern* p, const float* u_dev, uint64_t ldu, const float* v_dev, uint64_t ldv, uint32_t d, float* out_dev) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_sddmm(p->num_rows, p->num_cols, p->nnz, u_dev, ldu, v_dev, ldv, d, out_dev, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_wide_dot(p->rows.view, u_dev, ldu, v_dev, ldv, d, out_dev, p->stream));
    return HS_OK;
}

int hsw_spmm_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_spmm(p->num_rows, p->num_cols, p->nnz, w_dev, x_dev, ldx, d, y_dev, ldy, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_wide_gather(p->rows.view, w_dev, x_dev, ldx, d, y_dev, ldy, p->stream));
    return HS_OK;
}

int hsw_spmm_t_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_spmm(p->num_cols, p->num_rows, p->nnz, w_dev, x_dev, ldx, d, y_dev, ldy, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_wide_gather(p->cols.view, w_dev, x_dev, ldx, d, y_dev, ldy, p->stream));
    return HS_OK;
}

int hsw_sddmm(hsw_pattern* p, const float* u, const float* v, uint32_t d, float* out) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, u, uint64_t(p->num_rows) * d, v, uint64_t(p->num_cols) * d, out, p->nnz, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint64_t ld = hisparse::hsp::round_up4(d);
    Staging st(p);
    const float* d_u = st.in(u, p->num_rows, d, ld);
    const float* d_v = st.in(v, p->num_cols, d, ld);
    float* d_out = st.out(out, 1, p->nnz, p->nnz);
    return st.finish(st.failed() ? st.failed() : hsw_sddmm_device(p, d_u, ld, d_v, ld, d, d_out));
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

// ---- include/hisparse_aggregate.h: sum / mean / max / min of the neighbours' rows, on the same object ------------------------------------
int hsagg_forward_device(hsw_pattern* p, uint32_t ops, const float* x_dev, uint64_t ldx, uint32_t d, float* ysum_dev, float* ymax_dev, uint32_t* amax_dev, float* ymin_dev,
                         uint32_t* amin_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_agg_forward(p->num_rows, p->num_cols, ops, x_dev, ldx, d, ysum_dev, ymax_dev, amax_dev, ymin_dev, amin_dev, ldy, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_neighbor_forward(p->rows.view, aggregators(ops), x_dev, ldx, d, ysum_dev, ymax_dev, amax_dev, ymin_dev, amin_dev, ldy, p->stream));
    return HS_OK;
}

int hsagg_backward_device(hsw_pattern* p, uint32_t ops, const float* gsum_dev, const float* gmax_dev, const uint32_t* amax_dev, const float* gmin_dev, const uint32_t* amin_dev,
                          uint64_t ldg, uint32_t d, float* gx_dev, uint64_t ldgx) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_agg_backward(p->num_rows, p->num_cols, ops, gsum_dev, gmax_dev, amax_dev, gmin_dev, amin_dev, ldg, d, gx_dev, ldgx, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_neighbor_backward(p->cols.view, p->rows.view.ptr, aggregators(ops), gsum_dev, gmax_dev, amax_dev, gmin_dev, amin_dev, ldg, d, gx_dev, ldgx, p->stream));
    return HS_OK;
}

int hsagg_forward(hsw_pattern* p, uint32_t ops, const float* x, uint32_t d, float* ysum, float* ymax, uint32_t* amax, float* ymin, uint32_t* amin) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_agg_forward_host(p->num_rows, p->num_cols, ops, x, d, ysum, ymax, amax, ymin, amin, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const AggregateOps a = aggregators(ops);
    const uint64_t ld = hisparse::hsp::round_up4(d);
    Staging st(p);      // an output the call does not write is left out: a null host pointer is a null device pointer and no memory
    const float* d_x = st.in(x, p->num_cols, d, ld);
    float* d_sum = st.out(a.sum || a.mean ? ysum : nullptr, p->num_rows, d, ld);
    float* d_max = st.out(a.max ? ymax : nullptr, p->num_rows, d, ld);
    uint32_t* d_amax = st.out(a.max ? amax : nullptr, p->num_rows, d, ld);
    float* d_min = st.out(a.min ? ymin : nullptr, p->num_rows, d, ld);
    uint32_t* d_amin = st.out(a.min ? amin : nullptr, p->num_rows, d, ld);
    return st.finish(st.failed() ? st.failed() : hsagg_forward_device(p, ops, d_x, ld, d, d_sum, d_max, d_amax, d_min, d_amin, ld));
}

int hsagg_backward(hsw_pattern* p, uint32_t ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin, const uint32_t* amin, uint32_t d, float* gx) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_agg_backward_host(p->num_rows, p->num_cols, ops, gsum, gmax, amax, gmin, amin, d, gx, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const AggregateOps a = aggregators(ops);
    const uint64_t ld = hisparse::hsp::round_up4(d);
    Staging st(p);
    const float* d_sum = st.in(a.sum || a.mean ? gsum : nullptr, p->num_rows, d, ld);
    const float* d_max = st.in(a.max ? gmax : nullptr, p->num_rows, d, ld);
    const uint32_t* d_amax = st.in(a.max ? amax : nullptr, p->num_rows, d, ld);
    const float* d_min = st.in(a.min ? gmin : nullptr, p->num_rows, d, ld);
    const uint32_t* d_amin = st.in(a.min ? amin : nullptr, p->num_rows, d, ld);
    float* d_gx = st.out(gx, p->num_cols, d, ld);
    return st.finish(st.failed() ? st.failed() : hsagg_backward_device(p, ops, d_sum, d_max, d_amax, d_min, d_amin, ld, d, d_gx, ld));
}

}  // extern "C"
