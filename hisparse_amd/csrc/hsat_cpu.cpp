// hsat_cpu.cpp — include/hisparse_attention.h in libhisparse_cpu.so: the fused attention step on the host, for machines WITHOUT a GPU.
// Like hsw_cpu.cpp a second implementation that a driver loads INSTEAD of libhisparse_hip.so, never a fallback of it.  "Device" pointers
// are host pointers here, hsat_set_stream accepts and ignores, hsat_sync is a no-op.  Single-threaded: plain loops on the calling
// thread, two passes per row (the scores and their maximum, then the weights and the sums).
//
// Arithmetic = the kernel's (pattern_attention.hip), the header's ARITHMETIC block: one fp32 multiply per product of Q and K (built with
// -ffp-contract=off), added in double, s rounded once; t = scale * s in fp32; weights, sums, quotient and log-sum-exp in double, one
// rounding per output word.
// No dependency beyond the headers and hsat_common.h: tests/cpp/test_attention_cpu.cpp compiles this file alone under the sanitizers.
#include <cmath>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "hsat_common.h"

struct hsat_pattern {
    uint32_t num_rows = 0, num_cols = 0;
    std::vector<uint32_t> indptr, indices;
    std::string error;
    uint64_t nnz() const { return indptr.back(); }
};

namespace {

thread_local std::string g_create_error;

int fail(hsat_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}

void forward(const hsat_pattern* p, const float* q, uint64_t ldq, const float* k, uint64_t ldk, const float* v, uint64_t ldv, uint32_t d, float scale, float* y, uint64_t ldy,
             float* lse) {
    const float ninf = -std::numeric_limits<float>::infinity();
    std::vector<float> t;
    std::vector<double> acc(d);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        float* dst = y + uint64_t(r) * ldy;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = 0.0f;
            if (lse) lse[r] = ninf;
            continue;
        }
        const float* a = q + uint64_t(r) * ldq;
        t.resize(hi - lo);
        float m = ninf;      // one of the t words; a NaN is never the maximum
        for (uint64_t e = lo; e < hi; ++e) {
            const float* b = k + uint64_t(p->indices[e]) * ldk;
            double s = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(a[j] * b[j]);
            t[e - lo] = scale * float(s);
            m = std::fmax(m, t[e - lo]);
        }
        double l = 0.0;
        acc.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            // a -inf score weighs exactly 0, also while the maximum is -inf itself; a NaN, or +inf under a maximum of +inf, gives NaN
            const double w = t[e - lo] == ninf ? 0.0 : std::exp(double(t[e - lo]) - double(m));
            const float* b = v + uint64_t(p->indices[e]) * ldv;
            l += w;
            for (uint32_t j = 0; j < d; ++j) acc[j] += w * double(b[j]);
        }
        for (uint32_t j = 0; j < d; ++j) dst[j] = float(acc[j] / l);
        if (lse) lse[r] = float(double(m) + std::log(l));
    }
}

}  // namespace

extern "C" {

int hsat_create(hsat_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices) {
    (void)device_id;
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsat::check_create(num_rows, num_cols, indptr, indices, why)) return fail(nullptr, rc, why);
    hsat_pattern* p = new (std::nothrow) hsat_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->indptr.assign(indptr, indptr + size_t(num_rows) + 1);
    if (p->nnz()) p->indices.assign(indices, indices + p->nnz());
    *out = p;
    return HS_OK;
}

int hsat_destroy(hsat_pattern* p) {
    delete p;
    return HS_OK;
}

const char* hsat_last_error(const hsat_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsat_info(const hsat_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz();
    if (device_bytes) *device_bytes = 0;      // nothing lives on a device
    return HS_OK;
}

int hsat_set_stream(hsat_pattern* p, void* hip_stream) {
    (void)hip_stream;
    return p ? HS_OK : HS_ERR_BAD_ARG;
}

int hsat_sync(hsat_pattern* p) { return p ? HS_OK : HS_ERR_BAD_ARG; }

int hsat_forward_device(hsat_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, uint32_t d, float scale,
                        float* y_dev, uint64_t ldy, float* lse_dev) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsat::check_forward(p->num_rows, p->num_cols, q_dev, ldq, k_dev, ldk, v_dev, ldv, d, scale, y_dev, ldy, lse_dev, why)) return fail(p, rc, why);
    forward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, d, scale, y_dev, ldy, lse_dev);
    return HS_OK;
}

// the host form: ld = d and no alignment rule, so the loops walk the caller's arrays as they are
int hsat_forward(hsat_pattern* p, const float* q, const float* k, const float* v, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsat::check_forward_host(p->num_rows, p->num_cols, q, k, v, d, scale, y, lse, why)) return fail(p, rc, why);
    forward(p, q, d, k, d, v, d, d, scale, y, d, lse);
    return HS_OK;
}

}  // extern "C"
