// hsw_cpu.cpp — include/hisparse_wide.h in libhisparse_cpu.so: the row-major feature products on the host, for machines WITHOUT a GPU.
// Like hsp_cpu.cpp and hsr_cpu.cpp a second implementation that a driver loads INSTEAD of libhisparse_hip.so, never a fallback of it.
// "Device" pointers are host pointers here, hsw_set_stream accepts and ignores, hsw_sync is a no-op.  Single-threaded: plain loops on
// the calling thread (the reference implementation stays as plain as it can be).
//
// Arithmetic = the kernels' (wide_products.hip), the header's ARITHMETIC block: one fp32 multiply per product (built with
// -ffp-contract=off), the products of an output word added in double from +0.0, one rounding.  The transposed pattern is the one the HIP
// library builds (hsw_common.h): a column's entries in ascending CSR index.
// No dependency beyond the headers and hsw_common.h: tests/cpp/test_wide_cpu.cpp compiles this file alone under the sanitizers.
#include <new>
#include <string>
#include <vector>

#include "hsw_common.h"

struct hsw_pattern {
    uint32_t num_rows = 0, num_cols = 0;
    bool transposed = false;
    std::vector<uint32_t> indptr, indices;
    std::vector<uint32_t> cptr, trow, perm;      // HSW_TRANSPOSED
    std::string error;
    uint64_t nnz() const { return indptr.back(); }
};

namespace {

thread_local std::string g_create_error;

int fail(hsw_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}

void sddmm(const hsw_pattern* p, const float* u, uint64_t ldu, const float* v, uint64_t ldv, uint32_t d, float* out) {
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const float* a = u + uint64_t(r) * ldu;
        for (uint64_t e = p->indptr[r]; e < p->indptr[r + 1]; ++e) {
            const float* b = v + uint64_t(p->indices[e]) * ldv;
            double s = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(a[j] * b[j]);
            out[e] = float(s);
        }
    }
}

// Y[r] = sum over the entries k of row r of w[perm ? perm[k] : k] * X[idx[k]]
void spmm(uint32_t rows, const uint32_t* ptr, const uint32_t* idx, const uint32_t* perm, const float* w, const float* x, uint64_t ldx, uint32_t d, float* y, uint64_t ldy) {
    std::vector<double> s(d);
    for (uint32_t r = 0; r < rows; ++r) {
        s.assign(d, 0.0);
        for (uint64_t k = ptr[r]; k < ptr[r + 1]; ++k) {
            const float wk = w[perm ? perm[k] : k];
            const float* b = x + uint64_t(idx[k]) * ldx;
            for (uint32_t j = 0; j < d; ++j) s[j] += double(wk * b[j]);
        }
        float* dst = y + uint64_t(r) * ldy;
        for (uint32_t j = 0; j < d; ++j) dst[j] = float(s[j]);
    }
}

}  // namespace

extern "C" {

int hsw_create(hsw_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t flags) {
    (void)device_id;
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsw::check_create(num_rows, num_cols, indptr, indices, flags, why)) return fail(nullptr, rc, why);
    hsw_pattern* p = new (std::nothrow) hsw_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->transposed = (flags & HSW_TRANSPOSED) != 0;
    p->indptr.assign(indptr, indptr + size_t(num_rows) + 1);
    if (p->nnz()) p->indices.assign(indices, indices + p->nnz());
    if (p->transposed) hisparse::hsw::build_transposed(num_rows, num_cols, p->indptr.data(), p->indices.data(), p->cptr, p->trow, p->perm);
    *out = p;
    return HS_OK;
}

int hsw_destroy(hsw_pattern* p) {
    delete p;
    return HS_OK;
}

const char* hsw_last_error(const hsw_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsw_info(const hsw_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz();
    if (device_bytes) *device_bytes = 0;      // nothing lives on a device
    return HS_OK;
}

int hsw_set_stream(hsw_pattern* p, void* hip_stream) {
    (void)hip_stream;
    return p ? HS_OK : HS_ERR_BAD_ARG;
}

int hsw_sync(hsw_pattern* p) { return p ? HS_OK : HS_ERR_BAD_ARG; }

int hsw_sddmm_device(hsw_pattern* p, const float* u_dev, uint64_t ldu, const float* v_dev, uint64_t ldv, uint32_t d, float* out_dev) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_sddmm(p->num_rows, p->num_cols, p->nnz(), u_dev, ldu, v_dev, ldv, d, out_dev, why)) return fail(p, rc, why);
    sddmm(p, u_dev, ldu, v_dev, ldv, d, out_dev);
    return HS_OK;
}

int hsw_spmm_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_spmm(p->num_rows, p->num_cols, p->nnz(), w_dev, x_dev, ldx, d, y_dev, ldy, why)) return fail(p, rc, why);
    spmm(p->num_rows, p->indptr.data(), p->indices.data(), nullptr, w_dev, x_dev, ldx, d, y_dev, ldy);
    return HS_OK;
}

int hsw_spmm_t_device(hsw_pattern* p, const float* w_dev, const float* x_dev, uint64_t ldx, uint32_t d, float* y_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_spmm(p->num_cols, p->num_rows, p->nnz(), w_dev, x_dev, ldx, d, y_dev, ldy, why)) return fail(p, rc, why);
    spmm(p->num_cols, p->cptr.data(), p->trow.data(), p->perm.data(), w_dev, x_dev, ldx, d, y_dev, ldy);
    return HS_OK;
}

// the host forms: ld = d and no alignment rule, so the loops walk the caller's arrays as they are
int hsw_sddmm(hsw_pattern* p, const float* u, const float* v, uint32_t d, float* out) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, u, uint64_t(p->num_rows) * d, v, uint64_t(p->num_cols) * d, out, p->nnz(), why)) return fail(p, rc, why);
    sddmm(p, u, d, v, d, d, out);
    return HS_OK;
}

int hsw_spmm(hsw_pattern* p, const float* w, const float* x, uint32_t d, float* y) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, w, p->nnz(), x, uint64_t(p->num_cols) * d, y, uint64_t(p->num_rows) * d, why)) return fail(p, rc, why);
    spmm(p->num_rows, p->indptr.data(), p->indices.data(), nullptr, w, x, d, d, y, d);
    return HS_OK;
}

int hsw_spmm_t(hsw_pattern* p, const float* w, const float* x, uint32_t d, float* y) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_host(d, w, p->nnz(), x, uint64_t(p->num_rows) * d, y, uint64_t(p->num_cols) * d, why)) return fail(p, rc, why);
    spmm(p->num_cols, p->cptr.data(), p->trow.data(), p->perm.data(), w, x, d, d, y, d);
    return HS_OK;
}

}  // extern "C"
