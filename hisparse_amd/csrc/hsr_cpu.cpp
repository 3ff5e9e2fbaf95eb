// hsr_cpu.cpp — include/hisparse_rows.h in libhisparse_cpu.so: the row softmax and its backward on the host, for machines WITHOUT a GPU.
// Like hsp_cpu.cpp a second implementation that a driver loads INSTEAD of libhisparse_hip.so, never a fallback of it.  "Device" pointers
// are host pointers here, hsr_set_stream accepts and ignores, hsr_sync is a no-op.  Single-threaded: one loop over the rows on the calling
// thread (the operation is a few flops per entry; the reference implementation stays as plain as it can be).
//
// Arithmetic = the kernels' (row_softmax.hip), the header's ARITHMETIC block: one fp32 multiply and one fp32 subtract per score (built
// with -ffp-contract=off), libm's expf widened to double, the row sum and the quotient in double, one rounding; backward: products and
// their sum in double, (scale * p) * (gp - D) in double, one rounding.
// No dependency beyond the two headers and hsr_common.h: tests/cpp/test_rows_cpu.cpp compiles this file alone under the sanitizers.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "hsr_common.h"

struct hsr_rows {
    std::vector<uint32_t> indptr;
    std::string error;
    uint64_t nnz() const { return indptr.back(); }
};

namespace {

thread_local std::string g_create_error;

int fail(hsr_rows* r, int code, const std::string& msg) {
    if (r) r->error = msg; else g_create_error = msg;
    return code;
}

}  // namespace

extern "C" {

int hsr_create(hsr_rows** out, int device_id, uint32_t num_rows, const uint32_t* indptr) {
    (void)device_id;
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null rows pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsr::check_rows(num_rows, indptr, why)) return fail(nullptr, rc, why);
    hsr_rows* r = new (std::nothrow) hsr_rows;
    if (!r) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    r->indptr.assign(indptr, indptr + size_t(num_rows) + 1);
    *out = r;
    return HS_OK;
}

int hsr_destroy(hsr_rows* r) {
    delete r;
    return HS_OK;
}

const char* hsr_last_error(const hsr_rows* r) { return r ? r->error.c_str() : g_create_error.c_str(); }

int hsr_info(const hsr_rows* r, uint64_t* nnz, uint64_t* device_bytes) {
    if (!r) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = r->nnz();
    if (device_bytes) *device_bytes = 0;      // nothing lives on a device
    return HS_OK;
}

int hsr_set_stream(hsr_rows* r, void* hip_stream) {
    (void)hip_stream;
    return r ? HS_OK : HS_ERR_BAD_ARG;
}

int hsr_sync(hsr_rows* r) { return r ? HS_OK : HS_ERR_BAD_ARG; }

int hsr_softmax_device(hsr_rows* r, const float* s_dev, float scale, float* p_dev) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_forward(r->nnz(), s_dev, scale, p_dev, true, why)) return fail(r, rc, why);
    std::vector<float> e;
    for (size_t i = 0; i + 1 < r->indptr.size(); ++i) {
        const size_t lo = r->indptr[i], n = r->indptr[i + 1] - lo;
        if (n == 0) continue;
        e.resize(n);
        float m = -INFINITY;
        for (size_t k = 0; k < n; ++k) {
            e[k] = scale * s_dev[lo + k];
            m = std::fmax(m, e[k]);            // a NaN never becomes the maximum: it reaches the sum instead
        }
        double sum = 0.0;
        for (size_t k = 0; k < n; ++k) {
            e[k] = std::exp(e[k] - m);         // float overload: expf
            sum += double(e[k]);
        }
        for (size_t k = 0; k < n; ++k) p_dev[lo + k] = float(double(e[k]) / sum);
    }
    return HS_OK;
}

int hsr_softmax_backward_device(hsr_rows* r, const float* p_dev, const float* gp_dev, float scale, float* gs_dev) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_backward(r->nnz(), p_dev, gp_dev, scale, gs_dev, true, why)) return fail(r, rc, why);
    for (size_t i = 0; i + 1 < r->indptr.size(); ++i) {
        const size_t lo = r->indptr[i], hi = r->indptr[i + 1];
        double D = 0.0;
        for (size_t e = lo; e < hi; ++e) D += double(p_dev[e]) * double(gp_dev[e]);
        for (size_t e = lo; e < hi; ++e) gs_dev[e] = float((double(scale) * double(p_dev[e])) * (double(gp_dev[e]) - D));
    }
    return HS_OK;
}

// the host forms: the caller's arrays need no alignment, so they are copied as the HIP library copies them, and the row loops run in place
int hsr_softmax(hsr_rows* r, const float* s, float scale, float* p) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_forward(r->nnz(), s, scale, p, false, why)) return fail(r, rc, why);
    std::vector<float> d(r->nnz() + 1);
    std::memcpy(d.data(), s, r->nnz() * 4);
    if (int rc = hsr_softmax_device(r, d.data(), scale, d.data())) return rc;
    std::memcpy(p, d.data(), r->nnz() * 4);
    return HS_OK;
}

int hsr_softmax_backward(hsr_rows* r, const float* p, const float* gp, float scale, float* gs) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_backward(r->nnz(), p, gp, scale, gs, false, why)) return fail(r, rc, why);
    std::vector<float> dp(r->nnz() + 1), dg(r->nnz() + 1);
    std::memcpy(dp.data(), p, r->nnz() * 4);
    std::memcpy(dg.data(), gp, r->nnz() * 4);
    if (int rc = hsr_softmax_backward_device(r, dp.data(), dg.data(), scale, dg.data())) return rc;
    std::memcpy(gs, dg.data(), r->nnz() * 4);
    return HS_OK;
}

}  // extern "C"
