// hsmh_api.cpp — include/hisparse_heads.h on the HIP runtime: the pattern object of the multi-head attention step, forward and backward.
// As hsat_api.cpp's and hsab_api.cpp's, one object owns one device, one stream of its own and, from hsmh_create on, all the device
// memory its _device calls will ever use (device_buffer.h): the CSR arrays with the rows sorted into the length classes of
// wide_products.h (wide_schedule.h, which sorts and uploads a side) and, with HSMH_BACKWARD, the transposed pattern (hsw_common.h's
// stable counting sort, without its CSR-index map) with the columns sorted the same way and max_heads doubles per row, the D words the
// row kernel writes and the column kernel reads.  The kernels are in heads_attention.hip; what the object shares with the other pattern
// objects, and the host forms' transient buffers (Staging: every host form below is its operands, the _device call and finish), are
// pattern_object.h's.  Nothing here touches a context or another pattern object.
// The four hsmh16_* calls of include/hisparse_heads_bf16.h work on the same object with bf16 operands (heads16_attention.hip): the same
// pattern, transposed pattern, D words and stream, nothing held twice.
// The five hsmhb_* calls of include/hisparse_heads_bias.h add a per-entry, per-head bias (heads_bias_attention.hip).  hsmhb_create is
// hsmh_create that, with HSMH_BACKWARD, also keeps the shared sort's CSR-index map on the device (4 max(nnz, 1) bytes more): the column
// side of the backward finds an entry's bias words and stores its gbias words through it.  hsmh_create builds the map and drops it.
// The five hsmhd_* calls of include/hisparse_heads_dropout.h add dropout on the attention weights, with or without a bias
// (heads_dropout_attention.hip): no new object and no memory; the backward keys its column side's draws through the same map.
// The four hsmhd16_* calls of include/hisparse_heads_dropout_bf16.h are those calls with bf16 operands (heads16_dropout_attention.hip).
// The four hsgat_* calls of include/hisparse_gat.h run the graph attention (GAT) step on the same object (gat_attention.hip): additive
// scores from one word per node and head, the same pattern, transposed pattern, D words and stream, no map and no memory of their own.
// The six hsgat2_* calls of include/hisparse_gatv2.h run the GATv2 step on the same object (gatv2_attention.hip): the score is
// a . LeakyReLU(XD[row] + XS[col]); the backward's third launch adds the row side's per-workgroup vectors of ga, which live in a
// workspace the CALLER owns (hsgat2_work_bytes), so the object still allocates nothing outside create.
#include <new>
#include <string>
#include <vector>

#include "gat_attention.h"
#include "gatv2_attention.h"
#include "heads16_attention.h"
#include "heads16_dropout_attention.h"
#include "heads_attention.h"
#include "heads_bias_attention.h"
#include "heads_dropout_attention.h"
#include "hisparse_gat.h"
#include "hisparse_gatv2.h"
#include "hisparse_heads_bf16.h"
#include "hisparse_heads_bias.h"
#include "hisparse_heads_dropout.h"
#include "hisparse_heads_dropout_bf16.h"
#include "hsmh_common.h"
#include "wide_schedule.h"

using namespace hisparse::dev;
using namespace hisparse::obj;

struct hsmh_pattern : PatternObject {
    uint32_t num_rows = 0, num_cols = 0, max_heads = 0;
    bool backward = false;
    bool map = false;                // hsmhb_create with HSMH_BACKWARD: cols.perm is kept
    WideSideBuffers rows, cols;      // the pattern and its rows by class; with HSMH_BACKWARD: the transposed pattern and its columns by class
                                     // and, with the map, the CSR index of every entry of the transposed pattern (read by the kernels of
                                     // heads_bias_attention.hip, heads_dropout_attention.hip and heads16_dropout_attention.hip only)
    DeviceBuffer<double> dsum;       // with HSMH_BACKWARD: D per row and head, [row][max_heads]: one backward call in flight per object
};

namespace {

// everything hsmh_create does on the device; the caller destroys p when this fails
int build(hsmh_pattern* p, const uint32_t* indptr, const uint32_t* indices) {
    if (int rc = open_stream(p)) return rc;
    if (int rc = upload_side(p, p->rows, p->num_rows, indptr, indices, false, nullptr)) return rc;
    if (!p->backward) return HS_OK;
    std::vector<uint32_t> cptr, crow, perm;      // perm, the CSR index of every entry in column order: built by the shared sort, kept for hsmhb_create only
    hisparse::hsw::build_transposed(p->num_rows, p->num_cols, indptr, indices, cptr, crow, perm);
    if (!p->map) std::vector<uint32_t>().swap(perm);
    if (int rc = upload_side(p, p->cols, p->num_cols, cptr.data(), crow.data(), p->map, perm.data())) return rc;
    const size_t dsum_bytes = size_t(p->num_rows) * p->max_heads * 8;
    HS_HIP(p, p->dsum.alloc(dsum_bytes));
    p->device_bytes += dsum_bytes;
    return HS_OK;
}

// hsmh_create and hsmhb_create: keep_map asks for the entry map beside the transposed pattern
int create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags, bool keep_map) {
    if (!out) return fail<hsmh_pattern>(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    hipDeviceProp_t prop;
    if (int rc = hisparse::hsmh::check_create(num_rows, num_cols, indptr, indices, max_heads, flags, why)) return fail<hsmh_pattern>(nullptr, rc, why);
    if (int rc = probe_device(device_id, prop, why)) return fail<hsmh_pattern>(nullptr, rc, why);
    hsmh_pattern* p = new (std::nothrow) hsmh_pattern;
    if (!p) return fail<hsmh_pattern>(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->device = device_id;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->max_heads = max_heads;
    p->backward = (flags & HSMH_BACKWARD) != 0;
    p->map = keep_map && p->backward;
    p->nnz = indptr[num_rows];
    p->rows.view.compute_units = p->cols.view.compute_units = uint32_t(prop.multiProcessorCount);
    return finish_create(out, p, build(p, indptr, indices));
}

}  // namespace

extern "C" {

int hsmh_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags) {
    return create(out, device_id, num_rows, num_cols, indptr, indices, max_heads, flags, false);
}

int hsmh_destroy(hsmh_pattern* p) { return destroy(p); }
const char* hsmh_last_error(const hsmh_pattern* p) { return last_error(p); }
int hsmh_info(const hsmh_pattern* p, uint64_t* nnz, uint64_t* device_bytes) { return info(p, nnz, device_bytes); }
int hsmh_set_stream(hsmh_pattern* p, void* hip_stream) { return set_stream(p, hip_stream); }
int hsmh_sync(hsmh_pattern* p) { return sync(p); }

int hsmh_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d, float scale,
                        float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward(p->num_rows, p->num_cols, p->max_heads, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_heads_forward(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmh_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, uint32_t heads, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_host(p->num_rows, p->num_cols, p->max_heads, q, k, v, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const float* d_q = st.in(q, p->num_rows, w, w);
    const float* d_k = st.in(k, p->num_cols, w, w);
    const float* d_v = st.in(v, p->num_cols, w, w);
    float* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmh_forward_device(p, d_q, w, d_k, w, d_v, w, heads, d, scale, d_y, w, d_lse, heads));
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
    HS_HIP(p, launch_heads_backward_rows(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                           p->stream));
    HS_HIP(p, launch_heads_backward_cols(p->cols.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, scale, gk_dev, ldgk, gv_dev,
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
    Staging st(p);
    const float* d_q = st.in(q, p->num_rows, w, w);
    const float* d_k = st.in(k, p->num_cols, w, w);
    const float* d_v = st.in(v, p->num_cols, w, w);
    const float* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    float* d_gq = st.out(gq, p->num_rows, w, w);
    float* d_gk = st.out(gk, p->num_cols, w, w);
    float* d_gv = st.out(gv, p->num_cols, w, w);
    return st.finish(st.failed() ? st.failed() : hsmh_backward_device(p, d_q, w, d_k, w, d_v, w, d_gy, w, d_lse, heads, heads, d, scale, d_gq, w, d_gk, w, d_gv, w));
}

// ---- include/hisparse_heads_bf16.h: the same object, bf16 operands ----------------------------------------------------------------------
int hsmh16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                          float scale, uint16_t* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward16(p->num_rows, p->num_cols, p->max_heads, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_heads16_forward(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmh16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint32_t heads, uint32_t d, float scale, uint16_t* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward16_host(p->num_rows, p->num_cols, p->max_heads, q, k, v, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const uint16_t* d_q = st.in(q, p->num_rows, w, w);
    const uint16_t* d_k = st.in(k, p->num_cols, w, w);
    const uint16_t* d_v = st.in(v, p->num_cols, w, w);
    uint16_t* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmh16_forward_device(p, d_q, w, d_k, w, d_v, w, heads, d, scale, d_y, w, d_lse, heads));
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
    HS_HIP(p, launch_heads16_backward_rows(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                             p->stream));
    HS_HIP(p, launch_heads16_backward_cols(p->cols.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, scale, gk_dev, ldgk,
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
    Staging st(p);
    const uint16_t* d_q = st.in(q, p->num_rows, w, w);
    const uint16_t* d_k = st.in(k, p->num_cols, w, w);
    const uint16_t* d_v = st.in(v, p->num_cols, w, w);
    const uint16_t* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    uint16_t* d_gq = st.out(gq, p->num_rows, w, w);
    uint16_t* d_gk = st.out(gk, p->num_cols, w, w);
    uint16_t* d_gv = st.out(gv, p->num_cols, w, w);
    return st.finish(st.failed() ? st.failed() : hsmh16_backward_device(p, d_q, w, d_k, w, d_v, w, d_gy, w, d_lse, heads, heads, d, scale, d_gq, w, d_gk, w, d_gv, w));
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
    HS_HIP(p, launch_biased_forward(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmhb_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias, uint32_t heads, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_bias_host(p->num_rows, p->num_cols, p->max_heads, p->nnz, q, k, v, bias, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const float* d_q = st.in(q, p->num_rows, w, w);
    const float* d_k = st.in(k, p->num_cols, w, w);
    const float* d_v = st.in(v, p->num_cols, w, w);
    const float* d_b = st.in(bias, p->nnz, heads, heads);
    float* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmhb_forward_device(p, d_q, w, d_k, w, d_v, w, d_b, heads, heads, d, scale, d_y, w, d_lse, heads));
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
    HS_HIP(p, launch_biased_rows(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev, ldb, heads, d, scale, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                   p->stream));
    HS_HIP(p, launch_biased_cols(p->cols.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, bias_dev, ldb, heads, d, scale, gk_dev, ldgk,
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
    Staging st(p);
    const float* d_q = st.in(q, p->num_rows, w, w);
    const float* d_k = st.in(k, p->num_cols, w, w);
    const float* d_v = st.in(v, p->num_cols, w, w);
    const float* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    const float* d_b = st.in(bias, p->nnz, heads, heads);
    float* d_gq = st.out(gq, p->num_rows, w, w);
    float* d_gk = st.out(gk, p->num_cols, w, w);
    float* d_gv = st.out(gv, p->num_cols, w, w);
    float* d_gb = st.out(gbias, p->nnz, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmhb_backward_device(p, d_q, w, d_k, w, d_v, w, d_gy, w, d_lse, heads, d_b, heads, heads, d, scale, d_gq, w, d_gk, w,
                                                                      d_gv, w, d_gb, heads));
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
    HS_HIP(p, launch_dropout_forward(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, hisparse::philox::dropout_of(drop_p, seed, offset), y_dev, ldy,
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
    Staging st(p);
    const float* d_q = st.in(q, p->num_rows, w, w);
    const float* d_k = st.in(k, p->num_cols, w, w);
    const float* d_v = st.in(v, p->num_cols, w, w);
    const float* d_b = st.in(bias, p->nnz, heads, heads);
    float* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmhd_forward_device(p, d_q, w, d_k, w, d_v, w, d_b, heads, heads, d, scale, drop_p, seed, offset, d_y, w, d_lse,
                                                                     heads));
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
    HS_HIP(p, launch_dropout_rows(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev, ldb, heads, d, scale, dr, gq_dev, ldgq, p->dsum.get(), p->max_heads,
                                    p->stream));
    HS_HIP(p, launch_dropout_cols(p->cols.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, bias_dev, ldb, heads, d, scale, dr, gk_dev, ldgk,
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
    Staging st(p);
    const float* d_q = st.in(q, p->num_rows, w, w);
    const float* d_k = st.in(k, p->num_cols, w, w);
    const float* d_v = st.in(v, p->num_cols, w, w);
    const float* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    const float* d_b = st.in(bias, p->nnz, heads, heads);
    float* d_gq = st.out(gq, p->num_rows, w, w);
    float* d_gk = st.out(gk, p->num_cols, w, w);
    float* d_gv = st.out(gv, p->num_cols, w, w);
    float* d_gb = st.out(gbias, p->nnz, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmhd_backward_device(p, d_q, w, d_k, w, d_v, w, d_gy, w, d_lse, heads, d_b, heads, heads, d, scale, drop_p, seed, offset,
                                                                      d_gq, w, d_gk, w, d_gv, w, d_gb, heads));
}

// host code: no object, no device
int hsmhd_keep_mask(uint64_t nnz, uint32_t heads, float drop_p, uint64_t seed, uint64_t offset, uint8_t* keep) { return hisparse::hsmh::keep_mask(nnz, heads, drop_p, seed, offset, keep); }

// ---- include/hisparse_heads_dropout_bf16.h: the same object, bf16 operands, dropout on the attention weights, a bias or none ---------------
int hsmhd16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const float* bias_dev,
                           uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, uint16_t* y_dev, uint64_t ldy, float* lse_dev,
                           uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout16(p->num_rows, p->num_cols, p->max_heads, p->nnz, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, drop_p, y_dev,
                                                         ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_bf16_drop_forward(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, hisparse::philox::dropout_of(drop_p, seed, offset), y_dev, ldy,
                                         lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsmhd16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed,
                    uint64_t offset, uint16_t* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout16_host(p->num_rows, p->num_cols, p->max_heads, p->nnz, q, k, v, bias, heads, d, scale, drop_p, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const uint16_t* d_q = st.in(q, p->num_rows, w, w);
    const uint16_t* d_k = st.in(k, p->num_cols, w, w);
    const uint16_t* d_v = st.in(v, p->num_cols, w, w);
    const float* d_b = st.in(bias, p->nnz, heads, heads);
    uint16_t* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmhd16_forward_device(p, d_q, w, d_k, w, d_v, w, d_b, heads, heads, d, scale, drop_p, seed, offset, d_y, w, d_lse,
                                                                       heads));
}

int hsmhd16_backward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const uint16_t* gy_dev,
                            uint64_t ldgy, const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed,
                            uint64_t offset, uint16_t* gq_dev, uint64_t ldgq, uint16_t* gk_dev, uint64_t ldgk, uint16_t* gv_dev, uint64_t ldgv, float* gbias_dev, uint64_t ldgb) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout16(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev,
                                                          ldb, heads, d, scale, drop_p, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, gbias_dev, ldgb, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    HS_HIP(p, launch_bf16_drop_rows(p->rows.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev, ldb, heads, d, scale, dr, gq_dev, ldgq, p->dsum.get(),
                                      p->max_heads, p->stream));
    HS_HIP(p, launch_bf16_drop_cols(p->cols.view, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, bias_dev, ldb, heads, d, scale, dr, gk_dev,
                                      ldgk, gv_dev, ldgv, gbias_dev, ldgb, p->stream));
    return HS_OK;
}

int hsmhd16_backward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d,
                     float scale, float drop_p, uint64_t seed, uint64_t offset, uint16_t* gq, uint16_t* gk, uint16_t* gv, float* gbias) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout16_host(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz, q, k, v, gy, lse, bias, heads, d, scale, drop_p, gq, gk, gv, gbias,
                                                               why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const uint16_t* d_q = st.in(q, p->num_rows, w, w);
    const uint16_t* d_k = st.in(k, p->num_cols, w, w);
    const uint16_t* d_v = st.in(v, p->num_cols, w, w);
    const uint16_t* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    const float* d_b = st.in(bias, p->nnz, heads, heads);
    uint16_t* d_gq = st.out(gq, p->num_rows, w, w);
    uint16_t* d_gk = st.out(gk, p->num_cols, w, w);
    uint16_t* d_gv = st.out(gv, p->num_cols, w, w);
    float* d_gb = st.out(gbias, p->nnz, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsmhd16_backward_device(p, d_q, w, d_k, w, d_v, w, d_gy, w, d_lse, heads, d_b, heads, heads, d, scale, drop_p, seed, offset,
                                                                        d_gq, w, d_gk, w, d_gv, w, d_gb, heads));
}

// ---- include/hisparse_gat.h: the same object, additive (GAT) scores from one word per node and head ---------------------------------------
int hsgat_forward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                         float slope, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_forward(p->num_rows, p->num_cols, p->max_heads, el_dev, ldel, er_dev, lder, v_dev, ldv, heads, d, slope, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_gat_forward(p->rows.view, el_dev, ldel, er_dev, lder, v_dev, ldv, heads, d, slope, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsgat_forward(hsmh_pattern* p, const float* el, const float* er, const float* v, uint32_t heads, uint32_t d, float slope, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_forward_host(p->num_rows, p->num_cols, p->max_heads, el, er, v, heads, d, slope, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const float* d_el = st.in(el, p->num_rows, heads, heads);
    const float* d_er = st.in(er, p->num_cols, heads, heads);
    const float* d_v = st.in(v, p->num_cols, w, w);
    float* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsgat_forward_device(p, d_el, heads, d_er, heads, d_v, w, heads, d, slope, d_y, w, d_lse, heads));
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
    HS_HIP(p, launch_gat_backward_rows(p->rows.view, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, slope, gel_dev, ldgel, p->dsum.get(), p->max_heads,
                                         p->stream));
    HS_HIP(p, launch_gat_backward_cols(p->cols.view, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, slope, ger_dev, ldger,
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
    Staging st(p);
    const float* d_el = st.in(el, p->num_rows, heads, heads);
    const float* d_er = st.in(er, p->num_cols, heads, heads);
    const float* d_v = st.in(v, p->num_cols, w, w);
    const float* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    float* d_gel = st.out(gel, p->num_rows, heads, heads);
    float* d_ger = st.out(ger, p->num_cols, heads, heads);
    float* d_gv = st.out(gv, p->num_cols, w, w);
    return st.finish(st.failed() ? st.failed() : hsgat_backward_device(p, d_el, heads, d_er, heads, d_v, w, d_gy, w, d_lse, heads, heads, d, slope, d_gel, heads, d_ger, heads,
                                                                      d_gv, w));
}

// ---- include/hisparse_gatv2.h: the same object, the score a . LeakyReLU(XD[row] + XS[col]) and the gradient of a ---------------------------
int hsgat2_forward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev, uint32_t heads, uint32_t d, float slope,
                          float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_forward(p->num_rows, p->num_cols, p->max_heads, xd_dev, ldxd, xs_dev, ldxs, a_dev, heads, d, slope, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    HS_HIP(p, launch_gatv2_forward(p->rows.view, xd_dev, ldxd, xs_dev, ldxs, a_dev, heads, d, slope, y_dev, ldy, lse_dev, ldl, p->stream));
    return HS_OK;
}

int hsgat2_forward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, uint32_t heads, uint32_t d, float slope, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_forward_host(p->num_rows, p->num_cols, p->max_heads, xd, xs, a, heads, d, slope, y, lse, why)) return fail(p, rc, why);
    if (int rc = enter(p)) return rc;
    const uint32_t w = heads * d;
    Staging st(p);
    const float* d_xd = st.in(xd, p->num_rows, w, w);
    const float* d_xs = st.in(xs, p->num_cols, w, w);
    const float* d_a = st.in(a, 1, w, w);
    float* d_y = st.out(y, p->num_rows, w, w);
    float* d_lse = st.out(lse, p->num_rows, heads, heads);
    return st.finish(st.failed() ? st.failed() : hsgat2_forward_device(p, d_xd, w, d_xs, w, d_a, heads, d, slope, d_y, w, d_lse, heads));
}

// one vector of heads * d doubles per physical workgroup of the row side's launch
int hsgat2_work_bytes(const hsmh_pattern* p, uint32_t heads, uint32_t d, uint64_t* bytes) {
    if (!p || !bytes) return HS_ERR_BAD_ARG;
    std::string why;
    if (hisparse::hsmh::check_shape(heads, d, p->max_heads, why)) return HS_ERR_BAD_ARG;      // p is const: the reason is check_shape's, as the calls report it
    *bytes = uint64_t(gatv2_row_vectors(p->rows.view, heads, d)) * heads * d * 8;
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
    HS_HIP(p, launch_gatv2_backward_rows(p->rows.view, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, heads, d, slope, gxd_dev, ldgxd, p->dsum.get(), p->max_heads, work,
                                           p->stream));
    HS_HIP(p, launch_gatv2_backward_cols(p->cols.view, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, p->dsum.get(), p->max_heads, heads, d, slope, gxs_dev, ldgxs,
                                           p->stream));
    HS_HIP(p, launch_gatv2_reduce(work, gatv2_row_vectors(p->rows.view, heads, d), heads * d, ga_dev, p->stream));
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
    Staging st(p);
    const float* d_xd = st.in(xd, p->num_rows, w, w);
    const float* d_xs = st.in(xs, p->num_cols, w, w);
    const float* d_a = st.in(a, 1, w, w);
    const float* d_gy = st.in(gy, p->num_rows, w, w);
    const float* d_lse = st.in(lse, p->num_rows, heads, heads);
    float* d_gxd = st.out(gxd, p->num_rows, w, w);
    float* d_gxs = st.out(gxs, p->num_cols, w, w);
    float* d_ga = st.out(ga, 1, w, w);
    void* d_work = st.scratch(work_bytes);
    return st.finish(st.failed() ? st.failed() : hsgat2_backward_device(p, d_xd, w, d_xs, w, d_a, d_gy, w, d_lse, heads, heads, d, slope, d_gxd, w, d_gxs, w, d_ga, d_work,
                                                                       work_bytes));
}

}  // extern "C"
