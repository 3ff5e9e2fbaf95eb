// test_attention_backward_cpu.cpp — the CPU twin of include/hisparse_attention_backward.h (hisparse_amd/csrc/hsab_cpu.cpp) through its C
// boundary, as a program of its own: tests/test_attention_backward_cpu.py compiles both files with -fsanitize=address,undefined and runs
// the result.  The edge patterns and the refusals of the header; buffers are exactly as large as the contract says, so a read or write
// past them is the sanitizer's.  Values are checked against long double loops over the same lse words with a tolerance far above the
// contract's bound and far below any mistake of indexing (the bound itself is tests/attention_backward_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_attention_backward.h"
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

bool close_to(float got, long double want) { return std::fabs((long double)got - want) <= 1e-4L * (1.0L + std::fabs(want)); }

void check_pattern(const Pattern& pt, uint32_t d, uint32_t pad, float scale) {
    const std::string what = pt.name + ", d " + std::to_string(d) + ", pad " + std::to_string(pad);
    hsab_pattern* h = nullptr;
    EXPECT(hsab_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr) == HS_OK && h, what);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsab_info(h, &nnz, &bytes) == HS_OK && nnz == pt.nnz() && bytes == 0 && hsab_info(h, nullptr, nullptr) == HS_OK, what);
    const uint64_t ld = (d + 3) / 4 * 4 + pad;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f;
    // the last row of an operand ends with the 16-byte chunk of its word d - 1: the buffers are that short
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + (d + 3) / 4 * 4 : 0; };
    Floats Q(reach(pt.rows), nan), K(reach(pt.cols), nan), V(reach(pt.cols), nan), G(reach(pt.rows), nan), lse(pt.rows, -std::numeric_limits<float>::infinity());
    Floats gq(reach(pt.rows), mark), gk(reach(pt.cols), mark), gv(reach(pt.cols), mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < d; ++j) Q[r * ld + j] = next_float(2.0f), G[r * ld + j] = next_float(1.5f);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < d; ++j) K[c * ld + j] = next_float(2.0f), V[c * ld + j] = next_float(3.0f);
    // lse as a forward would write it, then the gradients in long double from those words
    std::vector<long double> want_q(size_t(pt.rows) * d, 0), want_k(size_t(pt.cols) * d, 0), want_v(size_t(pt.cols) * d, 0);
    std::vector<uint32_t> col_len(pt.cols, 0);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const uint64_t lo = pt.indptr[r], hi = pt.indptr[r + 1];
        if (lo == hi) continue;
        std::vector<long double> t(hi - lo), gp(hi - lo, 0);
        long double m = -std::numeric_limits<long double>::infinity(), l = 0, dsum = 0;
        for (uint64_t e = lo; e < hi; ++e) {
            long double s = 0;
            for (uint32_t j = 0; j < d; ++j) s += (long double)Q[r * ld + j] * K[pt.indices[e] * ld + j], gp[e - lo] += (long double)G[r * ld + j] * V[pt.indices[e] * ld + j];
            t[e - lo] = scale * s;
            m = std::fmax(m, t[e - lo]);
        }
        for (long double x : t) l += std::exp(x - m);
        lse[r] = float(m + std::log(l));
        for (uint64_t e = lo; e < hi; ++e) t[e - lo] = std::exp(t[e - lo] - (long double)lse[r]), dsum += t[e - lo] * gp[e - lo];
        for (uint64_t e = lo; e < hi; ++e) {
            const uint32_t c = pt.indices[e];
            const long double gs = scale * t[e - lo] * (gp[e - lo] - dsum);
            ++col_len[c];
            for (uint32_t j = 0; j < d; ++j) {
                want_q[size_t(r) * d + j] += gs * K[c * ld + j];
                want_k[size_t(c) * d + j] += gs * Q[r * ld + j];
                want_v[size_t(c) * d + j] += t[e - lo] * G[r * ld + j];
            }
        }
    }
    EXPECT(hsab_backward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.p(), d, scale, gq.p(), ld, gk.p(), ld, gv.p(), ld) == HS_OK, what);
    EXPECT(hsab_sync(h) == HS_OK && hsab_set_stream(h, nullptr) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const bool empty = pt.indptr[r] == pt.indptr[r + 1];
        for (uint32_t j = 0; j < d; ++j) {
            if (empty) EXPECT(gq[r * ld + j] == 0.0f && !std::signbit(gq[r * ld + j]), what + ", an empty row");
            else EXPECT(close_to(gq[r * ld + j], want_q[size_t(r) * d + j]), what + ", gq of row " + std::to_string(r));
        }
        for (uint64_t j = d; j < (r + 1 < pt.rows ? ld : (d + 3) / 4 * 4); ++j) EXPECT(gq[r * ld + j] == mark, what + ", a pad word of gq was written");
    }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t j = 0; j < d; ++j) {
            if (!col_len[c]) {
                EXPECT(gk[c * ld + j] == 0.0f && !std::signbit(gk[c * ld + j]) && gv[c * ld + j] == 0.0f && !std::signbit(gv[c * ld + j]), what + ", an empty column");
            } else {
                EXPECT(close_to(gk[c * ld + j], want_k[size_t(c) * d + j]), what + ", gk of column " + std::to_string(c));
                EXPECT(close_to(gv[c * ld + j], want_v[size_t(c) * d + j]), what + ", gv of column " + std::to_string(c));
            }
        }
        for (uint64_t j = d; j < (c + 1 < pt.cols ? ld : (d + 3) / 4 * 4); ++j) EXPECT(gk[c * ld + j] == mark && gv[c * ld + j] == mark, what + ", a pad word of gk or gv was written");
    }
    // the host form (ld = d) gives the words of the device form
    Floats hq(size_t(pt.rows) * d), hg(size_t(pt.rows) * d), hk(size_t(pt.cols) * d), hv(size_t(pt.cols) * d);
    Floats oq(size_t(pt.rows) * d, mark), ok(size_t(pt.cols) * d, mark), ov(size_t(pt.cols) * d, mark);
    for (uint32_t r = 0; r < pt.rows; ++r) std::memcpy(&hq[size_t(r) * d], &Q[r * ld], d * 4), std::memcpy(&hg[size_t(r) * d], &G[r * ld], d * 4);
    for (uint32_t c = 0; c < pt.cols; ++c) std::memcpy(&hk[size_t(c) * d], &K[c * ld], d * 4), std::memcpy(&hv[size_t(c) * d], &V[c * ld], d * 4);
    EXPECT(hsab_backward(h, hq.p(), hk.p(), hv.p(), hg.p(), lse.p(), d, scale, oq.p(), ok.p(), ov.p()) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) EXPECT(std::memcmp(&oq[size_t(r) * d], &gq[r * ld], d * 4) == 0, what + ": hsab_backward's gq differs");
    for (uint32_t c = 0; c < pt.cols; ++c)
        EXPECT(std::memcmp(&ok[size_t(c) * d], &gk[c * ld], d * 4) == 0 && std::memcmp(&ov[size_t(c) * d], &gv[c * ld], d * 4) == 0, what + ": hsab_backward's gk or gv differs");
    EXPECT(hsab_destroy(h) == HS_OK, what);
}

// an lse word of NaN and one of -inf on rows with entries: NaN in their gQ and in gK and gV of the columns they touch, nowhere else
void special_rows() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    //   row 0 empty (lse -inf, as the forward writes it), row 1 NaN over columns 0 and 1, row 2 -inf over column 2, rows 3 and 4 ordinary over 3 ... 5
    const std::vector<uint32_t> ip = {0, 0, 2, 3, 5, 7}, ix = {0, 1, 2, 3, 4, 4, 5};
    hsab_pattern* h = nullptr;
    EXPECT(hsab_create(&h, 0, 5, 7, ip.data(), ix.data()) == HS_OK && h, "special rows");
    if (!h) return;
    const uint32_t d = 3;
    const uint64_t ld = 4;
    Floats Q(5 * ld, 1.0f), K(7 * ld, 0.5f), V(7 * ld, 2.0f), G(5 * ld, 0.25f), lse(5), gq(5 * ld, -7.0f), gk(7 * ld, -7.0f), gv(7 * ld, -7.0f);
    lse[0] = -inf, lse[1] = nan, lse[2] = -inf, lse[3] = lse[4] = 1.5f + std::log(2.0f);
    EXPECT(hsab_backward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.p(), d, 1.0f, gq.p(), ld, gk.p(), ld, gv.p(), ld) == HS_OK, "special rows");
    for (uint32_t j = 0; j < d; ++j) {
        EXPECT(gq[j] == 0.0f && !std::signbit(gq[j]), "no entries");
        EXPECT(std::isnan(gq[ld + j]) && std::isnan(gq[2 * ld + j]), "gq of the rows with a non-finite lse");
        EXPECT(std::isfinite(gq[3 * ld + j]) && std::isfinite(gq[4 * ld + j]), "gq of the other rows");
        for (uint32_t c = 0; c < 3; ++c) EXPECT(std::isnan(gk[c * ld + j]) && std::isnan(gv[c * ld + j]), "the columns such a row touches");
        for (uint32_t c = 3; c < 6; ++c) EXPECT(std::isfinite(gk[c * ld + j]) && std::isfinite(gv[c * ld + j]), "the other columns");
        EXPECT(gk[6 * ld + j] == 0.0f && gv[6 * ld + j] == 0.0f && !std::signbit(gk[6 * ld + j]) && !std::signbit(gv[6 * ld + j]), "an empty column");
    }
    // equal scores and equal dots: P = 1/2, GP = D, so gs = 0 and gV = P gY summed over the column
    EXPECT(close_to(gv[3 * ld], 0.125L) && close_to(gv[4 * ld], 0.25L) && close_to(gq[3 * ld], 0.0L) && close_to(gk[4 * ld], 0.0L), "rows of two equal entries");
    EXPECT(hsab_destroy(h) == HS_OK, "destroy");
}

void refusals() {
    const std::vector<uint32_t> ip = {0, 3, 3, 8, 9}, ix = {0, 2, 4, 1, 1, 2, 3, 4, 0};
    std::vector<uint32_t> bad;
    hsab_pattern* h = reinterpret_cast<hsab_pattern*>(16);
    auto refused = [&](int rc, int code, const char* what) {
        EXPECT(rc == code && h == nullptr && std::strlen(hsab_last_error(nullptr)) > 0, what);
        h = reinterpret_cast<hsab_pattern*>(16);
    };
    refused(hsab_create(&h, 0, 0, 5, ip.data(), ix.data()), HS_ERR_BAD_ARG, "no rows");
    refused(hsab_create(&h, 0, 4, 0, ip.data(), ix.data()), HS_ERR_BAD_ARG, "no columns");
    refused(hsab_create(&h, 0, 4, 5, nullptr, ix.data()), HS_ERR_BAD_ARG, "null indptr");
    refused(hsab_create(&h, 0, 4, 5, ip.data(), nullptr), HS_ERR_BAD_ARG, "null indices");
    bad = {0, 3, 2, 8, 9};
    refused(hsab_create(&h, 0, 4, 5, bad.data(), ix.data()), HS_ERR_BAD_MATRIX, "indptr decreases");
    bad = {1, 3, 3, 8, 9};
    refused(hsab_create(&h, 0, 4, 5, bad.data(), ix.data()), HS_ERR_BAD_MATRIX, "indptr[0] = 1");
    refused(hsab_create(&h, 0, 4, 4, ip.data(), ix.data()), HS_ERR_BAD_MATRIX, "index = num_cols");
    EXPECT(hsab_create(nullptr, 0, 4, 5, ip.data(), ix.data()) == HS_ERR_BAD_ARG, "null out");
    Floats one(4);
    float* o = one.p();
    EXPECT(hsab_info(nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG && hsab_sync(nullptr) == HS_ERR_BAD_ARG && hsab_set_stream(nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsab_backward_device(nullptr, o, 4, o, 4, o, 4, o, 4, o, 1, 1.0f, o, 4, o, 4, o, 4) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsab_backward(nullptr, o, o, o, o, o, 1, 1.0f, o, o, o) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsab_destroy(nullptr) == HS_OK, "destroy(NULL)");

    h = nullptr;
    EXPECT(hsab_create(&h, 0, 4, 5, ip.data(), ix.data()) == HS_OK && h, "create");
    if (!h) return;
    const uint32_t d = 5;
    const uint64_t ld = 8;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    Floats q(4 * ld), k(5 * ld), v(5 * ld), g(4 * ld), l(4, 1.0f), gq(4 * ld), gk(5 * ld), gv(5 * ld), want(5 * ld), got(5 * ld), sink(5 * ld);
    for (size_t i = 0; i < 4 * ld; ++i) q[i] = next_float(2.0f), g[i] = next_float(2.0f);
    for (size_t i = 0; i < 5 * ld; ++i) k[i] = next_float(2.0f), v[i] = next_float(2.0f);
    EXPECT(hsab_backward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, g.p(), ld, l.p(), d, 0.5f, gq.p(), ld, want.p(), ld, sink.p(), ld) == HS_OK, "reference call");
    auto still_usable = [&](int rc, const char* what) {
        EXPECT(rc == HS_ERR_BAD_ARG && std::strlen(hsab_last_error(h)) > 0, what);
        EXPECT(hsab_backward_device(h, q.p(), ld, k.p(), ld, v.p(), ld, g.p(), ld, l.p(), d, 0.5f, gq.p(), ld, got.p(), ld, sink.p(), ld) == HS_OK &&
                   std::memcmp(got.p(), want.p(), 5 * ld * 4) == 0,
               what);
    };
    // one call with one argument changed: the eight pointers, the seven leading dimensions, d and scale
    struct Args {
        float *q, *k, *v, *g, *l, *gq, *gk, *gv;
        uint64_t ldq, ldk, ldv, ldg, ldgq, ldgk, ldgv;
        uint32_t d;
        float scale;
    };
    const Args ok = {q.p(), k.p(), v.p(), g.p(), l.p(), gq.p(), gk.p(), gv.p(), ld, ld, ld, ld, ld, ld, ld, d, 1.0f};
    auto call = [&](const Args& a) { return hsab_backward_device(h, a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, a.g, a.ldg, a.l, a.d, a.scale, a.gq, a.ldgq, a.gk, a.ldgk, a.gv, a.ldgv); };
    Args a = ok;
    a.d = 0, still_usable(call(a), "d = 0"), a = ok;
    a.d = 257, a.ldq = a.ldk = a.ldv = a.ldg = a.ldgq = a.ldgk = a.ldgv = 260, still_usable(call(a), "d = 257"), a = ok;
    a.scale = nan, still_usable(call(a), "scale NaN"), a = ok;
    a.scale = inf, still_usable(call(a), "scale inf"), a = ok;
    a.l = nullptr, still_usable(call(a), "null lse"), a = ok;
    a.l = reinterpret_cast<float*>(reinterpret_cast<char*>(l.p()) + 2), still_usable(call(a), "misaligned lse"), a = ok;
    float* Args::*const pointers[] = {&Args::q, &Args::k, &Args::v, &Args::g, &Args::gq, &Args::gk, &Args::gv};
    uint64_t Args::*const lds[] = {&Args::ldq, &Args::ldk, &Args::ldv, &Args::ldg, &Args::ldgq, &Args::ldgk, &Args::ldgv};
    for (int i = 0; i < 7; ++i) {
        const std::string name = std::string("feature argument ") + std::to_string(i);
        a.*pointers[i] = nullptr, still_usable(call(a), (name + " null").c_str()), a = ok;
        a.*pointers[i] = ok.*pointers[i] + 1 + i % 3, still_usable(call(a), (name + " misaligned").c_str()), a = ok;
        a.*lds[i] = 6, still_usable(call(a), (name + ": ld % 4").c_str()), a = ok;
        a.*lds[i] = 4, still_usable(call(a), (name + ": ld < d").c_str()), a = ok;
    }
    a.gq = q.p(), still_usable(call(a), "gq is q"), a = ok;
    a.gk = k.p() + 4, still_usable(call(a), "gk inside k"), a = ok;
    a.gv = v.p(), still_usable(call(a), "gv is v"), a = ok;
    a.gq = g.p(), still_usable(call(a), "gq is gy"), a = ok;
    a.gv = gk.p(), still_usable(call(a), "gv is gk"), a = ok;
    a.gk = gq.p() + 8, still_usable(call(a), "gk inside gq"), a = ok;
    a.l = gv.p() + 2, still_usable(call(a), "lse inside gv"), a = ok;
    still_usable(hsab_backward(h, nullptr, k.p(), v.p(), g.p(), l.p(), d, 1.0f, gq.p(), gk.p(), gv.p()), "host form null q");
    still_usable(hsab_backward(h, q.p(), k.p(), v.p(), g.p(), nullptr, d, 1.0f, gq.p(), gk.p(), gv.p()), "host form null lse");
    still_usable(hsab_backward(h, q.p(), k.p(), v.p(), g.p(), l.p(), d, 1.0f, gq.p(), gk.p(), nullptr), "host form null gv");
    still_usable(hsab_backward(h, q.p(), k.p(), v.p(), g.p(), l.p(), 0, 1.0f, gq.p(), gk.p(), gv.p()), "host form d = 0");
    still_usable(hsab_backward(h, q.p(), k.p(), v.p(), g.p(), l.p(), d, nan, gq.p(), gk.p(), gv.p()), "host form scale NaN");
    still_usable(hsab_backward(h, q.p(), k.p(), v.p(), g.p(), l.p(), d, 1.0f, gq.p(), k.p(), gv.p()), "host form gk is k");
    still_usable(hsab_backward(h, q.p(), k.p(), v.p(), g.p(), l.p(), d, 1.0f, gq.p(), gk.p(), gk.p() + 1), "host form gv inside gk");
    EXPECT(hsab_destroy(h) == HS_OK, "destroy");
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
    std::printf("ATTENTION BACKWARD CPU OK\n");
    return 0;
}
