// hsab_cpu.cpp — include/hisparse_attention_backward.h in libhisparse_cpu.so: the fused attention backward step on the host, for machines
// WITHOUT a GPU.  Like hsat_cpu.cpp a second implementation that a driver loads INSTEAD of libhisparse_hip.so, never a fallback of it.
// "Device" pointers are host pointers here, hsab_set_stream accepts and ignores, hsab_sync is a no-op.  Single-threaded: plain loops on
// the calling thread, two passes per row (the weights, the dots of gY and V and their sum D, then the three gradients); gK and gV are
// summed in double over all rows and rounded at the end, so a column's entries are added in ascending CSR order.
//
// Arithmetic = the kernels' (attention_backward.hip), the header's ARITHMETIC block: one fp32 multiply per product of Q and K and of gY
// and V (built with -ffp-contract=off), added in double, s rounded once; t = scale * s in fp32; gp kept double; weights, D, gs and the
// sums in double, one rounding per output word.
// No dependency beyond the headers and hsab_common.h: tests/cpp/test_attention_backward_cpu.cpp compiles this file alone under the
// sanitizers.
#include <cmath>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "hsab_common.h"

struct hsab_pattern {
    uint32_t num_rows = 0, num_cols = 0;
    std::vector<uint32_t> indptr, indices;
    std::string error;
    uint64_t nnz() const { return indptr.back(); }
};

namespace {

thread_local std::string g_create_error;

int fail(hsab_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}

void backward(const hsab_pattern* p, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy, const float* lse,
              uint32_t d, float scale, float* gq, uint64_t ldgq, float* gk, uint64_t ldgk, float* gv, uint64_t ldgv) {
    std::vector<double> w, gp, row(d);
    std::vector<double> sum_k(size_t(p->num_cols) * d, 0.0), sum_v(size_t(p->num_cols) * d, 0.0);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        float* dst = gq + uint64_t(r) * ldgq;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = 0.0f;
            continue;
        }
        const float* a = q + uint64_t(r) * ldq;
        const float* g = gy + uint64_t(r) * ldgy;
        // a word that is not finite (a dead or bad row of the forward) makes every weight of the row NaN
        const double l = std::isfinite(lse[r]) ? double(lse[r]) : std::numeric_limits<double>::quiet_NaN();
        w.resize(hi - lo);
        gp.resize(hi - lo);
        double dsum = 0.0;
        for (uint64_t e = lo; e < hi; ++e) {
            const float* b = k + uint64_t(p->indices[e]) * ldk;
            const float* c = v + uint64_t(p->indices[e]) * ldv;
            double s = 0.0, x = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(a[j] * b[j]);
            for (uint32_t j = 0; j < d; ++j) x += double(g[j] * c[j]);
            w[e - lo] = std::exp(double(scale * float(s)) - l);      // a -inf score under a finite lse weighs exactly 0
            gp[e - lo] = x;
            dsum += w[e - lo] * x;
        }
        row.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            const uint32_t c = p->indices[e];
            const double pe = w[e - lo], gs = double(scale) * (pe * (gp[e - lo] - dsum));
            const float* b = k + uint64_t(c) * ldk;
            double* to_k = sum_k.data() + size_t(c) * d;
            double* to_v = sum_v.data() + size_t(c) * d;
            for (uint32_t j = 0; j < d; ++j) {
                row[j] += gs * double(b[j]);
                to_k[j] += gs * double(a[j]);
                to_v[j] += pe * double(g[j]);
            }
        }
        for (uint32_t j = 0; j < d; ++j) dst[j] = float(row[j]);
    }
    for (uint32_t c = 0; c < p->num_cols; ++c) {
        for (uint32_t j = 0; j < d; ++j) {
            gk[uint64_t(c) * ldgk + j] = float(sum_k[size_t(c) * d + j]);
            gv[uint64_t(c) * ldgv + j] = float(sum_v[size_t(c) * d + j]);
        }
    }
}

}  // namespace

extern "C" {

int hsab_create(hsab_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices) {
    (void)device_id;
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsab::check_create(num_rows, num_cols, indptr, indices, why)) return fail(nullptr, rc, why);
    hsab_pattern* p = new (std::nothrow) hsab_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->indptr.assign(indptr, indptr + size_t(num_rows) + 1);
    if (p->nnz()) p->indices.assign(indices, indices + p->nnz());
    *out = p;
    return HS_OK;
}

int hsab_destroy(hsab_pattern* p) {
    delete p;
    return HS_OK;
}

const char* hsab_last_error(const hsab_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsab_info(const hsab_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz();
    if (device_bytes) *device_bytes = 0;      // nothing lives on a device
    return HS_OK;
}

int hsab_set_stream(hsab_pattern* p, void* hip_stream) {
    (void)hip_stream;
    return p ? HS_OK : HS_ERR_BAD_ARG;
}

int hsab_sync(hsab_pattern* p) { return p ? HS_OK : HS_ERR_BAD_ARG; }

int hsab_backward_device(hsab_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                         const float* lse_dev, uint32_t d, float scale, float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsab::check_backward(p->num_rows, p->num_cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv,
                                                why))
        return fail(p, rc, why);
    backward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv);
    return HS_OK;
}

// the host form: ld = d and no alignment rule, so the loops walk the caller's arrays as they are
int hsab_backward(hsab_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t d, float scale, float* gq, float* gk, float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsab::check_backward_host(p->num_rows, p->num_cols, q, k, v, gy, lse, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    backward(p, q, d, k, d, v, d, gy, d, lse, d, scale, gq, d, gk, d, gv, d);
    return HS_OK;
}

}  // extern "C"
