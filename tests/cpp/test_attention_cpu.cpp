// test_attention_cpu.cpp — the CPU twin of include/hisparse_attention.h (hisparse_amd/csrc/hsat_cpu.cpp) through its C boundary, as a
// program of its own: tests/test_attention_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge
// patterns and the refusals of the header; buffers are exactly as large as the contract says, so a read or write past them is the
// sanitizer's.  Values are checked against a long double softmax with a tolerance far above the contract's bound and far below any
// mistake of indexing (the bound itself is tests/attention_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_attention.h"
#include "hisparse_hip.h"

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

bool close_to(float got, long double want) { return std::fabs((long double)got - want) <= 1e-5L * (1.0L + std::fabs(want)); }

void check_pattern(const Pattern& pt, uint32_t d, uint32_t pad, float scale) {
    const std::string what = pt.name + ", d " + std::to_string(d) + ", pad " + std::to_string(pad);
    hsat_pattern* h = nullptr;
    EXPECT(hsat_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr) == HS_OK && h, what);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsat_info(h, &nnz, &bytes) == HS_OK && nnz == pt.nnz() && bytes == 0 && hsat_info(h, nullptr, nullptr) == HS_OK, what);
    const uint64_t ld = (d + 3) / 4 * 4 + pad;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f;
    // the last row of an operand ends with the 16-byte chunk of its word d - 1: the buffers are that short
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + (d + 3) / 4 * 4 : 0; };
    Floats Q(reach(pt.rows), nan), K(reach(pt.cols), nan), V(reach(pt.cols), nan), Y(reach(pt.rows), mark), Y2(reach(pt.rows), mark), lse(pt.rows, mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < d; ++j) Q[r * ld + j] = next_float(2.0f);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < d; ++j) K[c * ld + j] = next_float(2.0f), V[c * ld + j] = next_float(3.0f);
    EXPECT(hsat_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, d, scale, Y.p(), ld, lse.p()) == HS_OK, what);
    EXPECT(hsat_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, d, scale, Y2.p(), ld, nullptr) == HS_OK, what + ", lse NULL");
    EXPECT(hsat_sync(h) == HS_OK && hsat_set_stream(h, nullptr) == HS_OK, what);
    EXPECT(reach(pt.rows) == 0 || std::memcmp(Y.p(), Y2.p(), reach(pt.rows) * 4) == 0, what + ": y differs when lse is NULL");
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const uint64_t lo = pt.indptr[r], hi = pt.indptr[r + 1];
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) EXPECT(Y[r * ld + j] == 0.0f && !std::signbit(Y[r * ld + j]), what + ", an empty row");
            EXPECT(std::isinf(lse[r]) && lse[r] < 0, what + ", an empty row's lse");
        } else {
            std::vector<long double> t(hi - lo);
            long double m = -std::numeric_limits<long double>::infinity(), l = 0;
            for (uint64_t e = lo; e < hi; ++e) {
                long double s = 0;
                for (uint32_t j = 0; j < d; ++j) s += (long double)Q[r * ld + j] * K[pt.indices[e] * ld + j];
                t[e - lo] = scale * s;
                m = std::fmax(m, t[e - lo]);
            }
            for (long double& x : t) x = std::exp(x - m), l += x;
            for (uint32_t j = 0; j < d; ++j) {
                long double acc = 0;
                for (uint64_t e = lo; e < hi; ++e) acc += t[e - lo] * V[pt.indices[e] * ld + j];
                EXPECT(close_to(Y[r * ld + j], acc / l), what + ", row " + std::to_string(r));
            }
            EXPECT(close_to(lse[r], m + std::log(l)), what + ", lse of row " + std::to_string(r));
        }
        for (uint64_t j = d; j < (r + 1 < pt.rows ? ld : (d + 3) / 4 * 4); ++j) EXPECT(Y[r * ld + j] == mark, what + ", a pad word of y was written");
    }
    // the host form (ld = d) gives the words of the device form
    Floats hq(size_t(pt.rows) * d), hk(size_t(pt.cols) * d), hv(size_t(pt.cols) * d), hy(size_t(pt.rows) * d, mark), hl(pt.rows, mark);
    for (uint32_t r = 0; r < pt.rows; ++r) std::memcpy(&hq[size_t(r) * d], &Q[r * ld], d * 4);
    for (uint32_t c = 0; c < pt.cols; ++c) std::memcpy(&hk[size_t(c) * d], &K[c * ld], d * 4), std::memcpy(&hv[size_t(c) * d], &V[c * ld], d * 4);
    EXPECT(hsat_forward(h, hq.p(), hk.p(), hv.p(), d, scale, hy.p(), hl.p()) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) EXPECT(std::memcmp(&hy[size_t(r) * d], &Y[r * ld], d * 4) == 0, what + ": hsat_forward differs");
    EXPECT(std::memcmp(hl.p(), lse.p(), pt.rows * 4) == 0, what + ": hsat_forward's lse differs");
    EXPECT(hsat_forward(h, hq.p(), hk.p(), hv.p(), d, scale, hy.p(), nullptr) == HS_OK, what + ", host form, lse NULL");
    EXPECT(hsat_destroy(h) == HS_OK, what);
}

// the header's table of special rows, through K: -inf, +inf and NaN features against a positive word of Q
void special_rows() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    //   columns 0 ... 3 finite, 4 and 5 score -inf, 6 +inf, 7 NaN
    const std::vector<uint32_t> ip = {0, 0, 5, 7, 10, 13}, ix = {4, 5, 4, 0, 1, 4, 5, 0, 7, 1, 2, 6, 3};
    hsat_pattern* h = nullptr;
    EXPECT(hsat_create(&h, 0, 5, 8, ip.data(), ix.data()) == HS_OK && h, "special rows");
    if (!h) return;
    const uint32_t d = 3;
    const uint64_t ld = 4;
    Floats Q(5 * ld, 1.0f), K(8 * ld, 0.5f), V(8 * ld, 2.0f), Y(5 * ld, -7.0f), lse(5, -7.0f);
    K[4 * ld + 2] = K[5 * ld + 2] = -inf;
    K[6 * ld + 2] = inf;
    K[7 * ld + 2] = nan;
    V[0 * ld] = 1.0f;
    V[1 * ld] = 3.0f;
    EXPECT(hsat_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, d, 1.0f, Y.p(), ld, lse.p()) == HS_OK, "special rows");
    EXPECT(Y[0] == 0.0f && Y[1] == 0.0f && Y[2] == 0.0f && std::isinf(lse[0]) && lse[0] < 0, "no entries");
    EXPECT(Y[ld] == 2.0f && close_to(lse[1], 1.5L + std::log(2.0L)), "three -inf scores before two equal finite ones weigh 0");
    EXPECT(std::isnan(Y[2 * ld]) && std::isnan(Y[2 * ld + 2]) && std::isinf(lse[2]) && lse[2] < 0, "only -inf scores");
    EXPECT(std::isnan(Y[3 * ld]) && std::isnan(Y[3 * ld + 1]) && std::isnan(lse[3]), "a NaN score");
    EXPECT(std::isnan(Y[4 * ld]) && std::isnan(Y[4 * ld + 1]) && std::isnan(lse[4]), "a +inf score");
    EXPECT(hsat_destroy(h) == HS_OK, "destroy");
}

void refusals() {
    const std::vector<uint32_t> ip = {0, 3, 3, 8, 9}, ix = {0, 2, 4, 1, 1, 2, 3, 4, 0};
    std::vector<uint32_t> bad;
    hsat_pattern* h = reinterpret_cast<hsat_pattern*>(16);
    auto refused = [&](int rc, int code, const char* what) {
        EXPECT(rc == code && h == nullptr && std::strlen(hsat_last_error(nullptr)) > 0, what);
        h = reinterpret_cast<hsat_pattern*>(16);
    };
    refused(hsat_create(&h, 0, 0, 5, ip.data(), ix.data()), HS_ERR_BAD_ARG, "no rows");
    refused(hsat_create(&h, 0, 4, 0, ip.data(), ix.data()), HS_ERR_BAD_ARG, "no columns");
    refused(hsat_create(&h, 0, 4, 5, nullptr, ix.data()), HS_ERR_BAD_ARG, "null indptr");
    refused(hsat_create(&h, 0, 4, 5, ip.data(), nullptr), HS_ERR_BAD_ARG, "null indices");
    bad = {0, 3, 2, 8, 9};
    refused(hsat_create(&h, 0, 4, 5, bad.data(), ix.data()), HS_ERR_BAD_MATRIX, "indptr decreases");
    bad = {1, 3, 3, 8, 9};
    refused(hsat_create(&h, 0, 4, 5, bad.data(), ix.data()), HS_ERR_BAD_MATRIX, "indptr[0] = 1");
    refused(hsat_create(&h, 0, 4, 4, ip.data(), ix.data()), HS_ERR_BAD_MATRIX, "index = num_cols");
    EXPECT(hsat_create(nullptr, 0, 4, 5, ip.data(), ix.data()) == HS_ERR_BAD_ARG, "null out");
    Floats one(4);
    EXPECT(hsat_info(nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG && hsat_sync(nullptr) == HS_ERR_BAD_ARG && hsat_set_stream(nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsat_forward_device(nullptr, one.p(), 4, one.p(), 4, one.p(), 4, 1, 1.0f, one.p(), 4, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsat_forward(nullptr, one.p(), one.p(), one.p(), 1, 1.0f, one.p(), nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsat_destroy(nullptr) == HS_OK, "destroy(NULL)");

    h = nullptr;
    EXPECT(hsat_create(&h, 0, 4, 5, ip.data(), ix.data()) == HS_OK && h, "create");
    if (!h) return;
    const uint32_t d = 5;
    const uint64_t ld = 8;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    Floats q(4 * ld), k(5 * ld), v(5 * ld), y(4 * ld), l(4), want(4 * ld), got(4 * ld);
    for (size_t i = 0; i < 4 * ld; ++i) q[i] = next_float(2.0f);
    for (size_t i = 0; i < 5 * ld; ++i) k[i] = next_float(2.0f), v[i] = next_float(2.0f);
    EXPECT(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 0.5f, want.p(), ld, nullptr) == HS_OK, "reference call");
    auto still_usable = [&](int rc, const char* what) {
        EXPECT(rc == HS_ERR_BAD_ARG && std::strlen(hsat_last_error(h)) > 0, what);
        EXPECT(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 0.5f, got.p(), ld, nullptr) == HS_OK && std::memcmp(got.p(), want.p(), 4 * ld * 4) == 0, what);
    };
    float* odd4 = reinterpret_cast<float*>(reinterpret_cast<char*>(l.p()) + 2);
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, 0, 1.0f, y.p(), ld, l.p()), "d = 0");
    still_usable(hsat_forward_device(h, q.p(), 260, k.p(), 260, v.p(), 260, 257, 1.0f, y.p(), 260, l.p()), "d = 257");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, nan, y.p(), ld, l.p()), "scale NaN");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, inf, y.p(), ld, l.p()), "scale inf");
    still_usable(hsat_forward_device(h, nullptr, ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), ld, l.p()), "null q");
    still_usable(hsat_forward_device(h, q.p(), ld, nullptr, ld, v.p(), ld, d, 1.0f, y.p(), ld, l.p()), "null k");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, nullptr, ld, d, 1.0f, y.p(), ld, l.p()), "null v");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, nullptr, ld, l.p()), "null y");
    still_usable(hsat_forward_device(h, q.p() + 1, ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), ld, l.p()), "misaligned q");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p() + 2, ld, v.p(), ld, d, 1.0f, y.p(), ld, l.p()), "misaligned k");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p() + 3, ld, d, 1.0f, y.p(), ld, l.p()), "misaligned v");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p() + 1, ld, l.p()), "misaligned y");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), ld, odd4), "misaligned lse");
    still_usable(hsat_forward_device(h, q.p(), 6, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), ld, l.p()), "ldq % 4");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), 4, v.p(), ld, d, 1.0f, y.p(), ld, l.p()), "ldk < d");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), 7, d, 1.0f, y.p(), ld, l.p()), "ldv % 4");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), 4, l.p()), "ldy < d");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, q.p(), ld, l.p()), "y is q");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, k.p() + 4, ld, l.p()), "y inside k");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, v.p(), ld, l.p()), "y is v");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), ld, y.p() + 2), "lse inside y");
    still_usable(hsat_forward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, d, 1.0f, y.p(), ld, v.p() + 1), "lse inside v");
    still_usable(hsat_forward(h, nullptr, k.p(), v.p(), d, 1.0f, y.p(), l.p()), "host form null q");
    still_usable(hsat_forward(h, q.p(), k.p(), v.p(), 0, 1.0f, y.p(), l.p()), "host form d = 0");
    still_usable(hsat_forward(h, q.p(), k.p(), v.p(), d, nan, y.p(), l.p()), "host form scale NaN");
    still_usable(hsat_forward(h, q.p(), k.p(), v.p(), d, 1.0f, nullptr, l.p()), "host form null y");
    still_usable(hsat_forward(h, q.p(), k.p(), v.p(), d, 1.0f, k.p(), l.p()), "host form y is k");
    still_usable(hsat_forward(h, q.p(), k.p(), v.p(), d, 1.0f, y.p(), y.p() + 1), "host form lse inside y");
    EXPECT(hsat_destroy(h) == HS_OK, "destroy");
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
            for (uint32_t pad : {0u, 8u}) check_pattern(p, d, pad, d == 5 ? -0.75f : 0.5f);
    special_rows();
    refusals();
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("ATTENTION CPU OK\n");
    return 0;
}
