// hsp_cpu.cpp — include/hisparse_pattern.h in libhisparse_cpu.so: the sampled dense product on the host, for machines WITHOUT a GPU.
// Like cpu_backend.cpp a second implementation that a driver loads INSTEAD of libhisparse_hip.so, never a fallback of it.  "Device"
// pointers are host pointers here, hsp_set_stream accepts and ignores, hsp_sync is a no-op.
//
// Arithmetic = the kernels' (sddmm.hip), written with hisparse/q8_24.h and plain doubles:
//   fixed: every product narrowed to Q8.24 (AP_RND, AP_SAT), summed in 64 bits, clamped once; accumulate is a saturating add;
//   float: one fp32 multiply per (entry, j) (built with -ffp-contract=off), added in double from +0.0 in ascending j, rounded once;
//          accumulate adds the rounded partial to the old word in fp32.
// No dependency beyond the two headers and hsp_common.h: tests/cpp/test_pattern_cpu.cpp compiles this file alone under the sanitizers.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "hisparse/q8_24.h"
#include "hsp_common.h"

struct hsp_pattern {
    int impl = 0;
    uint32_t num_rows = 0, num_cols = 0, max_k = 0;
    std::vector<uint32_t> row, col;      // per entry, CSR order
    std::string error;
};

namespace {

thread_local std::string g_create_error;

int fail(hsp_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}

}  // namespace

extern "C" {

int hsp_create(hsp_pattern** out, int device_id, int impl, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices,
               uint32_t max_k) {
    (void)device_id;
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsp::check_pattern(impl, num_rows, num_cols, indptr, indices, max_k, why)) return fail(nullptr, rc, why);
    hsp_pattern* p = new (std::nothrow) hsp_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->impl = impl;
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->max_k = max_k;
    const uint64_t nnz = indptr[num_rows];
    p->col.assign(indices, indices + nnz);
    p->row.resize(nnz);
    for (uint32_t r = 0; r < num_rows; ++r)
        for (uint64_t e = indptr[r]; e < indptr[r + 1]; ++e) p->row[e] = r;
    *out = p;
    return HS_OK;
}

int hsp_destroy(hsp_pattern* p) {
    delete p;
    return HS_OK;
}

const char* hsp_last_error(const hsp_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsp_info(const hsp_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->row.size();
    if (device_bytes) *device_bytes = 0;      // nothing lives on a device
    return HS_OK;
}

int hsp_set_stream(hsp_pattern* p, void* hip_stream) {
    (void)hip_stream;
    return p ? HS_OK : HS_ERR_BAD_ARG;
}

int hsp_sync(hsp_pattern* p) { return p ? HS_OK : HS_ERR_BAD_ARG; }

int hsp_sddmm_device(hsp_pattern* p, const void* u_dev, uint64_t ldu, const void* v_dev, uint64_t ldv, uint32_t k, void* out_dev, int accumulate) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsp::check_product(p->num_rows, p->num_cols, p->max_k, u_dev, ldu, v_dev, ldv, k, out_dev, why)) return fail(p, rc, why);
    const uint32_t* u = static_cast<const uint32_t*>(u_dev);
    const uint32_t* v = static_cast<const uint32_t*>(v_dev);
    uint32_t* out = static_cast<uint32_t*>(out_dev);
    const bool fixed = p->impl == HS_IMPL_FIXED;
    for (size_t e = 0; e < p->row.size(); ++e) {
        const uint32_t r = p->row[e], c = p->col[e];
        if (fixed) {
            uint64_t sum = 0;
            for (uint32_t j = 0; j < k; ++j) sum += hisparse::q8_24_mul_raw(u[j * ldu + r], v[j * ldv + c]);
            if (accumulate) sum += out[e];
            out[e] = sum > hisparse::Q8_24_MAX_RAW ? hisparse::Q8_24_MAX_RAW : uint32_t(sum);
        } else {
            double sum = 0.0;
            for (uint32_t j = 0; j < k; ++j) {
                float a, b;
                std::memcpy(&a, &u[j * ldu + r], 4);
                std::memcpy(&b, &v[j * ldv + c], 4);
                const float prod = a * b;          // -ffp-contract=off: a multiply, then the add
                sum += double(prod);
            }
            float res = float(sum);
            if (accumulate) {
                float old;
                std::memcpy(&old, &out[e], 4);
                res = old + res;
            }
            std::memcpy(&out[e], &res, 4);
        }
    }
    return HS_OK;
}

int hsp_sddmm(hsp_pattern* p, const void* u, const void* v, uint32_t k, void* out) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!u || !v || !out) return fail(p, HS_ERR_BAD_ARG, "null argument");
    if (k < 1 || k > p->max_k) return fail(p, HS_ERR_BAD_ARG, "k must be 1 ... max_k (" + std::to_string(p->max_k) + ")");
    // the caller's arrays need not be 16-byte aligned: the device form's rule is for device memory, so copy as the HIP library does
    const uint64_t ldu = hisparse::hsp::round_up4(p->num_rows), ldv = hisparse::hsp::round_up4(p->num_cols);
    struct alignas(16) Quad { uint32_t w[4]; };
    std::vector<Quad> us(k * ldu / 4), vs(k * ldv / 4), os(p->row.size() / 4 + 1);
    std::memcpy(us.data(), u, k * ldu * 4);
    std::memcpy(vs.data(), v, k * ldv * 4);
    if (int rc = hsp_sddmm_device(p, us.data(), ldu, vs.data(), ldv, k, os.data(), 0)) return rc;
    std::memcpy(out, os.data(), p->row.size() * 4);
    return HS_OK;
}

}  // extern "C"
