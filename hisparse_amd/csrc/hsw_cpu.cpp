// hsw_cpu.cpp — include/hisparse_wide.h in libhisparse_cpu.so: the row-major feature products on the host, for machines WITHOUT a GPU.
// Like hsp_cpu.cpp and hsr_cpu.cpp a second implementation that a driver loads INSTEAD of libhisparse_hip.so, never a fallback of it.
// "Device" pointers are host pointers here, hsw_set_stream accepts and ignores, hsw_sync is a no-op.  Single-threaded: plain loops on
// the calling thread (the reference implementation stays as plain as it can be).
//
// Arithmetic = the kernels' (wide_products.hip), the header's ARITHMETIC block: one fp32 multiply per product (built with
// -ffp-contract=off), the products of an output word added in double from +0.0, one rounding.  The transposed pattern is the one the HIP
// library builds (hsw_common.h): a column's entries in ascending CSR index.
// The four calls of include/hisparse_aggregate.h (the twin of neighbor_aggregate.hip) are here too, on the same object: the winner rule is
// written as the header defines it, a walk over the row's entries, not as the kernels merge.
// No dependency beyond the headers and hsw_common.h: tests/cpp/test_wide_cpu.cpp compiles this file alone under the sanitizers.
#include <cmath>
#include <cstring>
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

// ---- include/hisparse_aggregate.h ---------------------------------------------------------------------------------------------------------
// the rank of the header's winner rule: v outranks b when it is a NaN against a non-NaN, else when the IEEE comparison says so; words
// that are equal (== or both NaN) do not outrank each other, and the smaller index then wins
bool outranks(float v, float b, bool max) {
    if (std::isnan(v) != std::isnan(b)) return std::isnan(v);
    if (std::isnan(v)) return false;
    return max ? v > b : v < b;
}

// the CSR index of the winner of feature j among row r's entries, HSAGG_NONE for a row without entries: the entries are walked in
// ascending index and only a word that outranks the best so far replaces it, so among equals the smallest index stays
uint32_t winner(const hsw_pattern* p, uint32_t r, const float* x, uint64_t ldx, uint32_t j, bool max) {
    uint32_t best = HSAGG_NONE;
    for (uint32_t e = p->indptr[r]; e < p->indptr[r + 1]; ++e)
        if (best == HSAGG_NONE || outranks(x[uint64_t(p->indices[e]) * ldx + j], x[uint64_t(p->indices[best]) * ldx + j], max)) best = e;
    return best;
}

// an extreme's word: the winner's word of X as it is, +0.0f for a row without entries
void copy_word(float* dst, const hsw_pattern* p, uint32_t e, const float* x, uint64_t ldx, uint32_t j) {
    const float zero = 0.0f;
    std::memcpy(dst, e == HSAGG_NONE ? &zero : &x[uint64_t(p->indices[e]) * ldx + j], sizeof(float));
}

void aggregate(const hsw_pattern* p, uint32_t ops, const float* x, uint64_t ldx, uint32_t d, float* ysum, float* ymax, uint32_t* amax, float* ymin, uint32_t* amin, uint64_t ldy) {
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint32_t lo = p->indptr[r], hi = p->indptr[r + 1];
        for (uint32_t j = 0; j < d; ++j) {
            const uint64_t at = uint64_t(r) * ldy + j;
            if (ops & (HSAGG_SUM | HSAGG_MEAN)) {
                double s = 0.0;
                for (uint32_t e = lo; e < hi; ++e) s += double(x[uint64_t(p->indices[e]) * ldx + j]);
                if ((ops & HSAGG_MEAN) && hi > lo) s /= double(hi - lo);
                ysum[at] = float(s);
            }
            if (ops & HSAGG_MAX) {
                const uint32_t e = winner(p, r, x, ldx, j, true);
                copy_word(ymax + at, p, e, x, ldx, j);
                if (amax) amax[at] = e;
            }
            if (ops & HSAGG_MIN) {
                const uint32_t e = winner(p, r, x, ldx, j, false);
                copy_word(ymin + at, p, e, x, ldx, j);
                if (amin) amin[at] = e;
            }
        }
    }
}

// gx[c][j]: over the entries k of column c, the gradient words of row(k) -- the sum's (the mean's: over the row's length, one double
// division) and an extreme's where the row's arg word names k's CSR index
void aggregate_backward(const hsw_pattern* p, uint32_t ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin, const uint32_t* amin, uint64_t ldg,
                        uint32_t d, float* gx, uint64_t ldgx) {
    for (uint32_t c = 0; c < p->num_cols; ++c) {
        for (uint32_t j = 0; j < d; ++j) {
            double s = 0.0;
            for (uint32_t k = p->cptr[c]; k < p->cptr[c + 1]; ++k) {
                const uint32_t r = p->trow[k], e = p->perm[k];
                const uint64_t at = uint64_t(r) * ldg + j;
                if (ops & HSAGG_SUM) s += double(gsum[at]);
                if (ops & HSAGG_MEAN) s += double(gsum[at]) / double(p->indptr[r + 1] - p->indptr[r]);
                if ((ops & HSAGG_MAX) && amax[at] == e) s += double(gmax[at]);
                if ((ops & HSAGG_MIN) && amin[at] == e) s += double(gmin[at]);
            }
            gx[uint64_t(c) * ldgx + j] = float(s);
        }
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

int hsagg_forward_device(hsw_pattern* p, uint32_t ops, const float* x_dev, uint64_t ldx, uint32_t d, float* ysum_dev, float* ymax_dev, uint32_t* amax_dev, float* ymin_dev,
                         uint32_t* amin_dev, uint64_t ldy) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_agg_forward(p->num_rows, p->num_cols, ops, x_dev, ldx, d, ysum_dev, ymax_dev, amax_dev, ymin_dev, amin_dev, ldy, why)) return fail(p, rc, why);
    aggregate(p, ops, x_dev, ldx, d, ysum_dev, ymax_dev, amax_dev, ymin_dev, amin_dev, ldy);
    return HS_OK;
}

int hsagg_backward_device(hsw_pattern* p, uint32_t ops, const float* gsum_dev, const float* gmax_dev, const uint32_t* amax_dev, const float* gmin_dev, const uint32_t* amin_dev,
                          uint64_t ldg, uint32_t d, float* gx_dev, uint64_t ldgx) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_agg_backward(p->num_rows, p->num_cols, ops, gsum_dev, gmax_dev, amax_dev, gmin_dev, amin_dev, ldg, d, gx_dev, ldgx, why)) return fail(p, rc, why);
    aggregate_backward(p, ops, gsum_dev, gmax_dev, amax_dev, gmin_dev, amin_dev, ldg, d, gx_dev, ldgx);
    return HS_OK;
}

int hsagg_forward(hsw_pattern* p, uint32_t ops, const float* x, uint32_t d, float* ysum, float* ymax, uint32_t* amax, float* ymin, uint32_t* amin) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsw::check_agg_forward_host(p->num_rows, p->num_cols, ops, x, d, ysum, ymax, amax, ymin, amin, why)) return fail(p, rc, why);
    aggregate(p, ops, x, d, d, ysum, ymax, amax, ymin, amin, d);
    return HS_OK;
}

int hsagg_backward(hsw_pattern* p, uint32_t ops, const float* gsum, const float* gmax, const uint32_t* amax, const float* gmin, const uint32_t* amin, uint32_t d, float* gx) {
    if (!p) return HS_ERR_BAD_ARG;
    if (!p->transposed) return fail(p, HS_ERR_UNSUPPORTED, "the object was created without HSW_TRANSPOSED");
    std::string why;
    if (int rc = hisparse::hsw::check_agg_backward_host(p->num_rows, p->num_cols, ops, gsum, gmax, amax, gmin, amin, d, gx, why)) return fail(p, rc, why);
    aggregate_backward(p, ops, gsum, gmax, amax, gmin, amin, d, d, gx, d);
    return HS_OK;
}

}  // extern "C"
