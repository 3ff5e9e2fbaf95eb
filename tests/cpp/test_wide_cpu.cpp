// test_wide_cpu.cpp — the CPU twin of include/hisparse_wide.h (hisparse_amd/csrc/hsw_cpu.cpp) through its C boundary, as a program of its
// own: tests/test_wide_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge patterns and the
// refusals of the header; buffers are exactly as large as the contract says, so a read or write past them is the sanitizer's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_hip.h"
#include "hisparse_wide.h"

namespace {

int g_failures = 0;
#define EXPECT(cond, what)                                                        \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, std::string(what).c_str()); \
            ++g_failures;                                                         \
        }                                                                         \
    } while (0)

uint64_t g_seed = 0x9E3779B97F4A7C15ull;
uint32_t next_word() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return uint32_t(g_seed >> 32);
}
float next_float(float magnitude) { return (float(next_word() >> 8) / float(1 << 24) - 0.5f) * 2.0f * magnitude; }

// n floats, 16-byte aligned, that end at most three floats before the end of their allocation (n = 0: never touched by a correct callee)
struct Floats {
    std::vector<float> raw;
    float* base;
    size_t n;
    explicit Floats(size_t count, float fill = 0.0f) : raw((count ? count : 1) + 4, fill), n(count) {
        uintptr_t p = reinterpret_cast<uintptr_t>(raw.data() + 4);
        base = reinterpret_cast<float*>(p - p % 16);
    }
    float* p() { return base; }
    float& operator[](size_t i) { return base[i]; }
};

struct Pattern {
    std::string name;
    uint32_t rows, cols;
    std::vector<uint32_t> indptr, indices;
    uint64_t nnz() const { return indptr.back(); }
};

Pattern from_lengths(const std::string& name, uint32_t cols, const std::vector<uint32_t>& lengths, bool sorted) {
    Pattern p{name, uint32_t(lengths.size()), cols, {0}, {}};
    for (uint32_t n : lengths) {
        std::vector<uint32_t> c(n);
        for (uint32_t k = 0; k < n; ++k) c[k] = sorted ? uint32_t(uint64_t(k) * cols / n) : next_word() % cols;
        p.indices.insert(p.indices.end(), c.begin(), c.end());
        p.indptr.push_back(uint32_t(p.indices.size()));
    }
    return p;
}

const double kU = std::ldexp(1.0, -24);

// |got - E| <= u |E| + n 2^-52 A + 2^-149 for the sum of the fp32 products `terms` (long double sums stand for E: their error is below the
// middle term's)
void check_word(float got, const std::vector<float>& terms, const std::string& what) {
    long double E = 0, A = 0;
    for (float t : terms) E += t, A += std::fabs((long double)t);
    const long double bound = kU * std::fabs(E) + (long double)terms.size() * std::ldexp(1.0L, -52) * A + std::ldexp(1.0L, -149);
    EXPECT(std::fabs((long double)got - E) <= bound, what);
}

void check_pattern(const Pattern& pt, uint32_t d, uint32_t pad) {
    const std::string what = pt.name + ", d " + std::to_string(d) + ", pad " + std::to_string(pad);
    hsw_pattern* h = nullptr;
    EXPECT(hsw_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr, HSW_TRANSPOSED) == HS_OK && h, what);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsw_info(h, &nnz, &bytes) == HS_OK && nnz == pt.nnz() && bytes == 0 && hsw_info(h, nullptr, nullptr) == HS_OK, what);
    const uint64_t ld = (d + 3) / 4 * 4 + pad;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f;
    Floats U(pt.rows * ld, nan), V(pt.cols * ld, nan), w(nnz), out(nnz, mark), Y(pt.rows * ld, mark), Yt(pt.cols * ld, mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < d; ++j) U[r * ld + j] = next_float(2.0f);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < d; ++j) V[c * ld + j] = next_float(2.0f);
    for (uint64_t e = 0; e < nnz; ++e) w[e] = next_float(3.0f);
    EXPECT(hsw_sddmm_device(h, U.p(), ld, V.p(), ld, d, out.p()) == HS_OK, what);
    EXPECT(hsw_spmm_device(h, w.p(), V.p(), ld, d, Y.p(), ld) == HS_OK, what);
    EXPECT(hsw_spmm_t_device(h, w.p(), U.p(), ld, d, Yt.p(), ld) == HS_OK, what);
    EXPECT(hsw_sync(h) == HS_OK && hsw_set_stream(h, nullptr) == HS_OK, what);
    std::vector<std::vector<std::vector<float>>> col_terms(pt.cols, std::vector<std::vector<float>>(d));
    for (uint32_t r = 0; r < pt.rows; ++r) {
        std::vector<std::vector<float>> row_terms(d);
        for (uint64_t e = pt.indptr[r]; e < pt.indptr[r + 1]; ++e) {
            const uint32_t c = pt.indices[e];
            std::vector<float> dot;
            for (uint32_t j = 0; j < d; ++j) {
                volatile float p = U[r * ld + j] * V[c * ld + j], q = w[e] * V[c * ld + j], t = w[e] * U[r * ld + j];
                dot.push_back(float(p));
                row_terms[j].push_back(float(q));
                col_terms[c][j].push_back(float(t));
            }
            check_word(out[e], dot, what + ", sddmm entry " + std::to_string(e));
        }
        for (uint32_t j = 0; j < d; ++j) {
            check_word(Y[r * ld + j], row_terms[j], what + ", spmm row " + std::to_string(r));
            if (row_terms[j].empty()) EXPECT(Y[r * ld + j] == 0.0f && !std::signbit(Y[r * ld + j]), what + ", an empty row");
        }
        for (uint64_t j = d; j < ld; ++j) EXPECT(Y[r * ld + j] == mark, what + ", spmm wrote a pad word");
    }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t j = 0; j < d; ++j) {
            check_word(Yt[c * ld + j], col_terms[c][j], what + ", spmm_t column " + std::to_string(c));
            if (col_terms[c][j].empty()) EXPECT(Yt[c * ld + j] == 0.0f && !std::signbit(Yt[c * ld + j]), what + ", an empty column");
        }
        for (uint64_t j = d; j < ld; ++j) EXPECT(Yt[c * ld + j] == mark, what + ", spmm_t wrote a pad word");
    }
    // the host forms (ld = d) give the words of the device forms
    Floats hu(size_t(pt.rows) * d), hv(size_t(pt.cols) * d), ho(nnz, mark), hy(size_t(pt.rows) * d, mark), hyt(size_t(pt.cols) * d, mark);
    for (uint32_t r = 0; r < pt.rows; ++r) std::memcpy(&hu[size_t(r) * d], &U[r * ld], d * 4);
    for (uint32_t c = 0; c < pt.cols; ++c) std::memcpy(&hv[size_t(c) * d], &V[c * ld], d * 4);
    EXPECT(hsw_sddmm(h, hu.p(), hv.p(), d, ho.p()) == HS_OK && hsw_spmm(h, w.p(), hv.p(), d, hy.p()) == HS_OK && hsw_spmm_t(h, w.p(), hu.p(), d, hyt.p()) == HS_OK, what);
    EXPECT(nnz == 0 || std::memcmp(ho.p(), out.p(), nnz * 4) == 0, what + ": hsw_sddmm differs");
    for (uint32_t r = 0; r < pt.rows; ++r) EXPECT(std::memcmp(&hy[size_t(r) * d], &Y[r * ld], d * 4) == 0, what + ": hsw_spmm differs");
    for (uint32_t c = 0; c < pt.cols; ++c) EXPECT(std::memcmp(&hyt[size_t(c) * d], &Yt[c * ld], d * 4) == 0, what + ": hsw_spmm_t differs");
    EXPECT(hsw_destroy(h) == HS_OK, what);
}

void refusals() {
    const std::vector<uint32_t> ip = {0, 3, 3, 8, 9}, ix = {0, 2, 4, 1, 1, 2, 3, 4, 0};
    std::vector<uint32_t> bad;
    hsw_pattern* h = reinterpret_cast<hsw_pattern*>(16);
    auto refused = [&](int rc, int code, const char* what) {
        EXPECT(rc == code && h == nullptr && std::strlen(hsw_last_error(nullptr)) > 0, what);
        h = reinterpret_cast<hsw_pattern*>(16);
    };
    refused(hsw_create(&h, 0, 0, 5, ip.data(), ix.data(), 1), HS_ERR_BAD_ARG, "no rows");
    refused(hsw_create(&h, 0, 4, 0, ip.data(), ix.data(), 1), HS_ERR_BAD_ARG, "no columns");
    refused(hsw_create(&h, 0, 4, 5, nullptr, ix.data(), 1), HS_ERR_BAD_ARG, "null indptr");
    refused(hsw_create(&h, 0, 4, 5, ip.data(), nullptr, 1), HS_ERR_BAD_ARG, "null indices");
    refused(hsw_create(&h, 0, 4, 5, ip.data(), ix.data(), 2), HS_ERR_BAD_ARG, "unknown flag");
    refused(hsw_create(&h, 0, 4, 5, ip.data(), ix.data(), 0x80000001u), HS_ERR_BAD_ARG, "unknown flag beside the known one");
    bad = {0, 3, 2, 8, 9};
    refused(hsw_create(&h, 0, 4, 5, bad.data(), ix.data(), 1), HS_ERR_BAD_MATRIX, "indptr decreases");
    bad = {1, 3, 3, 8, 9};
    refused(hsw_create(&h, 0, 4, 5, bad.data(), ix.data(), 1), HS_ERR_BAD_MATRIX, "indptr[0] = 1");
    refused(hsw_create(&h, 0, 4, 4, ip.data(), ix.data(), 1), HS_ERR_BAD_MATRIX, "index = num_cols");
    EXPECT(hsw_create(nullptr, 0, 4, 5, ip.data(), ix.data(), 1) == HS_ERR_BAD_ARG, "null out");
    Floats one(4);
    EXPECT(hsw_info(nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG && hsw_sync(nullptr) == HS_ERR_BAD_ARG && hsw_set_stream(nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsw_sddmm_device(nullptr, one.p(), 4, one.p(), 4, 1, one.p()) == HS_ERR_BAD_ARG && hsw_sddmm(nullptr, one.p(), one.p(), 1, one.p()) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsw_spmm_device(nullptr, one.p(), one.p(), 4, 1, one.p(), 4) == HS_ERR_BAD_ARG && hsw_spmm(nullptr, one.p(), one.p(), 1, one.p()) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsw_spmm_t_device(nullptr, one.p(), one.p(), 4, 1, one.p(), 4) == HS_ERR_BAD_ARG && hsw_spmm_t(nullptr, one.p(), one.p(), 1, one.p()) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsw_destroy(nullptr) == HS_OK, "destroy(NULL)");

    h = nullptr;
    hsw_pattern* plain = nullptr;
    EXPECT(hsw_create(&h, 0, 4, 5, ip.data(), ix.data(), HSW_TRANSPOSED) == HS_OK && h, "create");
    EXPECT(hsw_create(&plain, 0, 4, 5, ip.data(), ix.data(), 0) == HS_OK && plain, "create without the flag");
    if (!h || !plain) return;
    const uint32_t d = 5;
    const uint64_t ld = 8, n = 9;
    Floats u(5 * ld), v(5 * ld), w(n), y(5 * ld), e(n), want(4 * ld), got(4 * ld);
    for (size_t i = 0; i < 5 * ld; ++i) u[i] = next_float(2.0f), v[i] = next_float(2.0f);
    for (size_t i = 0; i < n; ++i) w[i] = next_float(3.0f);
    EXPECT(hsw_spmm_device(h, w.p(), v.p(), ld, d, want.p(), ld) == HS_OK, "reference call");
    auto still_usable = [&](int rc, const char* what, int code = HS_ERR_BAD_ARG, hsw_pattern* obj = nullptr) {
        obj = obj ? obj : h;
        EXPECT(rc == code && std::strlen(hsw_last_error(obj)) > 0, what);
        EXPECT(hsw_spmm_device(obj, w.p(), v.p(), ld, d, got.p(), ld) == HS_OK && std::memcmp(got.p(), want.p(), 4 * ld * 4) == 0, what);
    };
    float* odd16 = u.p() + 1;                                                          // 4-byte aligned only
    float* odd4 = reinterpret_cast<float*>(reinterpret_cast<char*>(w.p()) + 2);        // not even that
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p(), ld, 0, e.p()), "sddmm d = 0");
    still_usable(hsw_sddmm_device(h, u.p(), 260, v.p(), 260, 257, e.p()), "sddmm d = 257");
    still_usable(hsw_sddmm_device(h, nullptr, ld, v.p(), ld, d, e.p()), "sddmm null u");
    still_usable(hsw_sddmm_device(h, u.p(), ld, nullptr, ld, d, e.p()), "sddmm null v");
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p(), ld, d, nullptr), "sddmm null out");
    still_usable(hsw_sddmm_device(h, odd16, ld, v.p(), ld, d, e.p()), "sddmm misaligned u");
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p() + 2, ld, d, e.p()), "sddmm misaligned v");
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p(), ld, d, odd4), "sddmm misaligned out");
    still_usable(hsw_sddmm_device(h, u.p(), 6, v.p(), ld, d, e.p()), "sddmm ldu % 4");
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p(), 4, d, e.p()), "sddmm ldv < d");
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p(), ld, d, u.p() + 4), "sddmm out inside u");
    still_usable(hsw_sddmm_device(h, u.p(), ld, v.p(), ld, d, v.p()), "sddmm out is v");
    for (int t = 0; t < 2; ++t) {
        auto f = t ? hsw_spmm_t_device : hsw_spmm_device;
        const std::string name = t ? "spmm_t " : "spmm ";
        still_usable(f(h, w.p(), v.p(), ld, 0, y.p(), ld), (name + "d = 0").c_str());
        still_usable(f(h, w.p(), v.p(), 260, 257, y.p(), 260), (name + "d = 257").c_str());
        still_usable(f(h, nullptr, v.p(), ld, d, y.p(), ld), (name + "null w").c_str());
        still_usable(f(h, w.p(), nullptr, ld, d, y.p(), ld), (name + "null x").c_str());
        still_usable(f(h, w.p(), v.p(), ld, d, nullptr, ld), (name + "null y").c_str());
        still_usable(f(h, odd4, v.p(), ld, d, y.p(), ld), (name + "misaligned w").c_str());
        still_usable(f(h, w.p(), odd16, ld, d, y.p(), ld), (name + "misaligned x").c_str());
        still_usable(f(h, w.p(), v.p(), ld, d, y.p() + 1, ld), (name + "misaligned y").c_str());
        still_usable(f(h, w.p(), v.p(), 7, d, y.p(), ld), (name + "ldx % 4").c_str());
        still_usable(f(h, w.p(), v.p(), ld, d, y.p(), 4), (name + "ldy < d").c_str());
        still_usable(f(h, w.p(), v.p(), ld, d, v.p(), ld), (name + "y is x").c_str());
        still_usable(f(h, w.p(), v.p(), ld, d, w.p(), ld), (name + "y holds w").c_str());
    }
    still_usable(hsw_sddmm(h, nullptr, v.p(), d, e.p()), "host sddmm null u");
    still_usable(hsw_sddmm(h, u.p(), v.p(), 0, e.p()), "host sddmm d = 0");
    still_usable(hsw_sddmm(h, u.p(), v.p(), d, nullptr), "host sddmm null out");
    still_usable(hsw_spmm(h, w.p(), nullptr, d, y.p()), "host spmm null x");
    still_usable(hsw_spmm(h, w.p(), v.p(), 257, y.p()), "host spmm d = 257");
    still_usable(hsw_spmm_t(h, nullptr, u.p(), d, y.p()), "host spmm_t null w");
    still_usable(hsw_spmm_t(h, w.p(), u.p(), d, u.p()), "host spmm_t y is x");
    still_usable(hsw_spmm_t_device(plain, w.p(), u.p(), ld, d, y.p(), ld), "spmm_t_device without the flag", HS_ERR_UNSUPPORTED, plain);
    still_usable(hsw_spmm_t(plain, w.p(), u.p(), d, y.p()), "spmm_t without the flag", HS_ERR_UNSUPPORTED, plain);
    EXPECT(hsw_destroy(h) == HS_OK && hsw_destroy(plain) == HS_OK, "destroy");
}

}  // namespace

int main() {
    std::vector<Pattern> patterns;
    patterns.push_back(from_lengths("nnz = 0", 7, {0, 0, 0, 0, 0}, true));
    patterns.push_back(from_lengths("one entry", 1, {1}, true));
    patterns.push_back(from_lengths("runs of empty rows", 11, {0, 0, 0, 3, 1, 0, 0, 0, 0, 6, 0, 2, 0, 0}, false));
    patterns.push_back(from_lengths("one row holds every entry", 301, {0, 0, 301, 0}, true));
    patterns.push_back(from_lengths("one column holds every entry", 1, {1, 1, 0, 1, 1, 1, 0, 1}, true));
    patterns.push_back(from_lengths("unsorted columns, pairs held twice", 6, {9, 0, 14, 3}, false));
    patterns.push_back(Pattern{"an entry in the last row and column", 7, 13, {0, 1, 1, 1, 1, 1, 1, 2}, {0, 12}});
    for (const Pattern& p : patterns)
        for (uint32_t d : {1u, 5u, 64u})
            for (uint32_t pad : {0u, 8u}) check_pattern(p, d, pad);
    refusals();
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("WIDE CPU OK\n");
    return 0;
}
