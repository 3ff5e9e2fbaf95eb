// test_heads_cpu.cpp — the CPU twin of include/hisparse_heads.h (hisparse_amd/csrc/hsmh_cpu.cpp) through its C boundary, as a program of
// its own: tests/test_heads_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge patterns and the
// refusals of the header; buffers are exactly as large as the contract says (a feature operand ends with the 16-byte chunk of its last
// word, lse with head `heads - 1` of its last row), so a read or write past them is the sanitizer's.  Values are checked against long
// double loops per head with a tolerance far above the contract's bound and far below any mistake of indexing (the bound itself is
// tests/heads_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_heads.h"
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

// n floats, 16-byte aligned, that end at most three floats before the end of their allocation
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
bool plus_zero(float x) { return x == 0.0f && !std::signbit(x); }

void check_pattern(const Pattern& pt, uint32_t heads, uint32_t d, uint32_t pad, uint32_t ldl_extra, float scale) {
    const std::string what = pt.name + ", " + std::to_string(heads) + " heads of d " + std::to_string(d) + ", pad " + std::to_string(pad);
    hsmh_pattern* h = nullptr;
    EXPECT(hsmh_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr, heads, HSMH_BACKWARD) == HS_OK && h, what);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsmh_info(h, &nnz, &bytes) == HS_OK && nnz == pt.nnz() && bytes == 0 && hsmh_info(h, nullptr, nullptr) == HS_OK, what);
    const uint32_t w = heads * d;
    const uint64_t ld = w + pad, ldl = heads + ldl_extra;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f, ninf = -std::numeric_limits<float>::infinity();
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + w : 0; };
    const size_t lse_words = size_t(pt.rows - 1) * ldl + heads;
    Floats Q(reach(pt.rows), nan), K(reach(pt.cols), nan), V(reach(pt.cols), nan), G(reach(pt.rows), nan);
    Floats y(reach(pt.rows), mark), lse(lse_words, mark), gq(reach(pt.rows), mark), gk(reach(pt.cols), mark), gv(reach(pt.cols), mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < w; ++j) Q[r * ld + j] = next_float(2.0f), G[r * ld + j] = next_float(1.5f);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < w; ++j) K[c * ld + j] = next_float(2.0f), V[c * ld + j] = next_float(3.0f);
    EXPECT(hsmh_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, heads, d, scale, y.p(), ld, lse.p(), ldl) == HS_OK, what);
    EXPECT(hsmh_sync(h) == HS_OK && hsmh_set_stream(h, nullptr) == HS_OK, what);
    // the forward per head in long double, then the gradients from the lse words the call wrote
    std::vector<long double> want_y(size_t(pt.rows) * w, 0), want_l(size_t(pt.rows) * heads, 0), want_q(size_t(pt.rows) * w, 0), want_k(size_t(pt.cols) * w, 0),
        want_v(size_t(pt.cols) * w, 0);
    std::vector<uint32_t> col_len(pt.cols, 0);
    for (uint64_t e = 0; e < pt.nnz(); ++e) ++col_len[pt.indices[e]];
    for (uint32_t hd = 0; hd < heads; ++hd) {
        const uint32_t at = hd * d;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            const uint64_t lo = pt.indptr[r], hi = pt.indptr[r + 1];
            if (lo == hi) continue;
            std::vector<long double> t(hi - lo), gp(hi - lo, 0);
            long double m = -std::numeric_limits<long double>::infinity(), l = 0, dsum = 0;
            for (uint64_t e = lo; e < hi; ++e) {
                long double s = 0;
                for (uint32_t j = at; j < at + d; ++j) s += (long double)Q[r * ld + j] * K[pt.indices[e] * ld + j], gp[e - lo] += (long double)G[r * ld + j] * V[pt.indices[e] * ld + j];
                t[e - lo] = scale * s;
                m = std::fmax(m, t[e - lo]);
            }
            for (long double x : t) l += std::exp(x - m);
            want_l[size_t(r) * heads + hd] = m + std::log(l);
            for (uint64_t e = lo; e < hi; ++e)
                for (uint32_t j = at; j < at + d; ++j) want_y[size_t(r) * w + j] += std::exp(t[e - lo] - m) / l * V[pt.indices[e] * ld + j];
            const long double given = lse[r * ldl + hd];
            for (uint64_t e = lo; e < hi; ++e) t[e - lo] = std::exp(t[e - lo] - given), dsum += t[e - lo] * gp[e - lo];
            for (uint64_t e = lo; e < hi; ++e) {
                const uint32_t c = pt.indices[e];
                const long double gs = scale * t[e - lo] * (gp[e - lo] - dsum);
                for (uint32_t j = at; j < at + d; ++j) {
                    want_q[size_t(r) * w + j] += gs * K[c * ld + j];
                    want_k[size_t(c) * w + j] += gs * Q[r * ld + j];
                    want_v[size_t(c) * w + j] += t[e - lo] * G[r * ld + j];
                }
            }
        }
    }
    EXPECT(hsmh_backward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.p(), ldl, heads, d, scale, gq.p(), ld, gk.p(), ld, gv.p(), ld) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const bool empty = pt.indptr[r] == pt.indptr[r + 1];
        for (uint32_t j = 0; j < w; ++j) {
            if (empty) EXPECT(plus_zero(y[r * ld + j]) && plus_zero(gq[r * ld + j]), what + ", an empty row");
            else EXPECT(close_to(y[r * ld + j], want_y[size_t(r) * w + j]) && close_to(gq[r * ld + j], want_q[size_t(r) * w + j]), what + ", y and gq");
        }
        for (uint32_t hd = 0; hd < heads; ++hd) {
            if (empty) EXPECT(lse[r * ldl + hd] == ninf, what + ", lse of an empty row");
            else EXPECT(close_to(lse[r * ldl + hd], want_l[size_t(r) * heads + hd]), what + ", lse");
        }
        if (r + 1 < pt.rows) {
            for (uint64_t j = w; j < ld; ++j) EXPECT(y[r * ld + j] == mark && gq[r * ld + j] == mark, what + ", a pad word of y or gq was written");
            for (uint64_t j = heads; j < ldl; ++j) EXPECT(lse[r * ldl + j] == mark, what + ", a pad word of lse was written");
        }
    }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t j = 0; j < w; ++j) {
            if (!col_len[c]) EXPECT(plus_zero(gk[c * ld + j]) && plus_zero(gv[c * ld + j]), what + ", an empty column");
            else EXPECT(close_to(gk[c * ld + j], want_k[size_t(c) * w + j]) && close_to(gv[c * ld + j], want_v[size_t(c) * w + j]), what + ", gk and gv");
        }
        if (c + 1 < pt.cols)
            for (uint64_t j = w; j < ld; ++j) EXPECT(gk[c * ld + j] == mark && gv[c * ld + j] == mark, what + ", a pad word of gk or gv was written");
    }
    // the host forms over arrays of exactly n * heads * d words give the same words
    {
        std::vector<float> q(size_t(pt.rows) * w), g(q.size()), k(size_t(pt.cols) * w), v(k.size()), hy(q.size(), mark), hl(size_t(pt.rows) * heads, mark), hq(q.size(), mark),
            hk(k.size(), mark), hv(k.size(), mark);
        for (uint32_t r = 0; r < pt.rows; ++r)
            for (uint32_t j = 0; j < w; ++j) q[size_t(r) * w + j] = Q[r * ld + j], g[size_t(r) * w + j] = G[r * ld + j];
        for (uint32_t c = 0; c < pt.cols; ++c)
            for (uint32_t j = 0; j < w; ++j) k[size_t(c) * w + j] = K[c * ld + j], v[size_t(c) * w + j] = V[c * ld + j];
        EXPECT(hsmh_forward(h, q.data(), k.data(), v.data(), heads, d, scale, hy.data(), hl.data()) == HS_OK, what + ", host form");
        EXPECT(hsmh_backward(h, q.data(), k.data(), v.data(), g.data(), hl.data(), heads, d, scale, hq.data(), hk.data(), hv.data()) == HS_OK, what + ", host form");
        bool same = true;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            same = same && !std::memcmp(&hy[size_t(r) * w], &y[r * ld], w * 4) && !std::memcmp(&hq[size_t(r) * w], &gq[r * ld], w * 4) &&
                   !std::memcmp(&hl[size_t(r) * heads], &lse[r * ldl], heads * 4);
        }
        for (uint32_t c = 0; c < pt.cols; ++c) same = same && !std::memcmp(&hk[size_t(c) * w], &gk[c * ld], w * 4) && !std::memcmp(&hv[size_t(c) * w], &gv[c * ld], w * 4);
        EXPECT(same, what + ", the host forms give other words than the device forms");
        std::vector<float> y2(q.size(), mark);
        EXPECT(hsmh_forward(h, q.data(), k.data(), v.data(), heads, d, scale, y2.data(), nullptr) == HS_OK && !std::memcmp(y2.data(), hy.data(), y2.size() * 4), what + ", lse NULL");
    }
    EXPECT(hsmh_destroy(h) == HS_OK, what);
}

void edges() {
    std::vector<Pattern> pts;
    pts.push_back(from_lengths("nnz = 0", 5, {0, 0, 0}, true));
    pts.push_back(from_lengths("one entry", 3, {0, 1, 0, 0}, true));
    pts.push_back(from_lengths("runs of empty rows", 40, {0, 0, 3, 0, 0, 0, 7, 1, 0, 0}, true));
    pts.push_back(from_lengths("unsorted, pairs held twice", 6, {5, 9, 0, 2}, false));
    pts.push_back(from_lengths("one long row", 700, {0, 301, 2}, true));
    pts.push_back(Pattern{"1 x 1", 1, 1, {0, 1}, {0}});
    for (const Pattern& pt : pts) {
        check_pattern(pt, 3, 8, 8, 2, 1.5f);
        check_pattern(pt, 5, 4, 0, 0, -0.5f);
        check_pattern(pt, 1, 64, 4, 1, 0.25f);
    }
}

void refusals() {
    const Pattern pt = from_lengths("refusals", 9, {2, 0, 1, 3, 0, 1}, true);
    hsmh_pattern* h = reinterpret_cast<hsmh_pattern*>(0xBAD);
    const uint32_t* ip = pt.indptr.data();
    const uint32_t* ix = pt.indices.data();
    std::vector<uint32_t> bad_index = pt.indices, down = pt.indptr, shifted = pt.indptr;
    bad_index[3] = 9;
    down[2] = down[1] - 1;
    for (uint32_t& x : shifted) ++x;
    struct Create { const char* what; uint32_t rows, cols; const uint32_t* ip; const uint32_t* ix; uint32_t max_heads, flags; int code; };
    const Create creates[] = {{"null indptr", 6, 9, nullptr, ix, 4, 1, HS_ERR_BAD_ARG}, {"null indices", 6, 9, ip, nullptr, 4, 1, HS_ERR_BAD_ARG},
                              {"no rows", 0, 9, ip, ix, 4, 1, HS_ERR_BAD_ARG}, {"no columns", 6, 0, ip, ix, 4, 1, HS_ERR_BAD_ARG},
                              {"index = num_cols", 6, 9, ip, bad_index.data(), 4, 1, HS_ERR_BAD_MATRIX}, {"indptr decreases", 6, 9, down.data(), ix, 4, 1, HS_ERR_BAD_MATRIX},
                              {"indptr[0] = 1", 6, 9, shifted.data(), ix, 4, 1, HS_ERR_BAD_MATRIX}, {"max_heads = 0", 6, 9, ip, ix, 0, 1, HS_ERR_BAD_ARG},
                              {"max_heads = 65", 6, 9, ip, ix, 65, 1, HS_ERR_BAD_ARG}, {"flags = 2", 6, 9, ip, ix, 4, 2, HS_ERR_BAD_ARG}};
    for (const Create& c : creates) {
        h = reinterpret_cast<hsmh_pattern*>(0xBAD);
        EXPECT(hsmh_create(&h, 0, c.rows, c.cols, c.ip, c.ix, c.max_heads, c.flags) == c.code && !h && std::strlen(hsmh_last_error(nullptr)), c.what);
    }
    EXPECT(hsmh_create(nullptr, 0, 6, 9, ip, ix, 4, 1) == HS_ERR_BAD_ARG, "null out");
    Floats one(4);
    EXPECT(hsmh_info(nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG && hsmh_sync(nullptr) == HS_ERR_BAD_ARG && hsmh_set_stream(nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmh_forward_device(nullptr, one.p(), 4, one.p(), 4, one.p(), 4, 1, 4, 1.0f, one.p(), 4, nullptr, 1) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmh_forward(nullptr, one.p(), one.p(), one.p(), 1, 4, 1.0f, one.p(), nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmh_backward_device(nullptr, one.p(), 4, one.p(), 4, one.p(), 4, one.p(), 4, one.p(), 1, 1, 4, 1.0f, one.p(), 4, one.p(), 4, one.p(), 4) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmh_backward(nullptr, one.p(), one.p(), one.p(), one.p(), one.p(), 1, 4, 1.0f, one.p(), one.p(), one.p()) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmh_destroy(nullptr) == HS_OK, "null object");

    hsmh_pattern* fwd_only = nullptr;
    EXPECT(hsmh_create(&h, 0, 6, 9, ip, ix, 4, HSMH_BACKWARD) == HS_OK && h, "create");
    EXPECT(hsmh_create(&fwd_only, 0, 6, 9, ip, ix, 4, 0) == HS_OK && fwd_only, "create without the flag");
    if (!h || !fwd_only) return;
    const uint32_t heads = 2, d = 4, w = 8;
    const uint64_t ld = 8;
    Floats Q(6 * ld, 0.5f), K(9 * ld, 0.25f), V(9 * ld, 1.0f), G(6 * ld, -1.0f), y(6 * ld), lse(6 * heads), gq(6 * ld), gk(9 * ld), gv(9 * ld);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto fwd = [&](hsmh_pattern* p, const float* q, uint64_t ldq, uint32_t hh, uint32_t dd, float sc, float* yy, uint64_t ldy, float* ll, uint64_t ldl) {
        return hsmh_forward_device(p, q, ldq, K.p(), ld, V.p(), ld, hh, dd, sc, yy, ldy, ll, ldl);
    };
    auto bwd = [&](hsmh_pattern* p, const float* ll, uint64_t ldl, uint32_t hh, uint32_t dd, float sc, float* q_out, uint64_t ldgq, float* v_out) {
        return hsmh_backward_device(p, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, ll, ldl, hh, dd, sc, q_out, ldgq, gk.p(), ld, v_out, ld);
    };
    auto good = [&](const std::string& after) {
        EXPECT(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, lse.p(), heads) == HS_OK, std::string("the object is unusable after ") + after);
        EXPECT(bwd(h, lse.p(), heads, heads, d, 1.0f, gq.p(), ld, gv.p()) == HS_OK, std::string("the object is unusable after ") + after);
    };
    good("nothing");
#define REFUSED(call, what)                                                              \
    do {                                                                                 \
        EXPECT((call) == HS_ERR_BAD_ARG && std::strlen(hsmh_last_error(h)), what);       \
        good(what);                                                                      \
    } while (0)
    for (uint32_t bad_d : {0u, 1u, 2u, 3u, 5u, 6u, 12u, 512u}) {
        REFUSED(fwd(h, Q.p(), ld, 1, bad_d, 1.0f, y.p(), ld, lse.p(), 1), "d = " + std::to_string(bad_d));
        REFUSED(bwd(h, lse.p(), 1, 1, bad_d, 1.0f, gq.p(), ld, gv.p()), "d = " + std::to_string(bad_d));
    }
    REFUSED(fwd(h, Q.p(), ld, 0, d, 1.0f, y.p(), ld, lse.p(), heads), "heads = 0");
    REFUSED(fwd(h, Q.p(), 512, 5, 4, 1.0f, y.p(), 512, lse.p(), 5), "heads > max_heads");
    REFUSED(fwd(h, Q.p(), 512, 4, 128, 1.0f, y.p(), 512, lse.p(), 4), "heads * d = 512");
    REFUSED(bwd(h, lse.p(), 5, 5, 4, 1.0f, gq.p(), ld, gv.p()), "heads > max_heads");
    REFUSED(bwd(h, lse.p(), 4, 4, 128, 1.0f, gq.p(), ld, gv.p()), "heads * d = 512");
    for (float sc : {nan, inf, -inf}) {
        REFUSED(fwd(h, Q.p(), ld, heads, d, sc, y.p(), ld, lse.p(), heads), "scale not finite");
        REFUSED(bwd(h, lse.p(), heads, heads, d, sc, gq.p(), ld, gv.p()), "scale not finite");
    }
    REFUSED(fwd(h, nullptr, ld, heads, d, 1.0f, y.p(), ld, lse.p(), heads), "null q");
    REFUSED(fwd(h, Q.p() + 1, ld, heads, d, 1.0f, y.p(), ld, lse.p(), heads), "misaligned q");
    REFUSED(fwd(h, Q.p(), 10, heads, d, 1.0f, y.p(), ld, lse.p(), heads), "ldq % 4");
    REFUSED(fwd(h, Q.p(), 4, heads, d, 1.0f, y.p(), ld, lse.p(), heads), "ldq < heads * d");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, nullptr, ld, lse.p(), heads), "null y");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), 4, lse.p(), heads), "ldy < heads * d");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, lse.p(), 1), "ldl < heads");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, Q.p(), ld, lse.p(), heads), "y is q");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, y.p() + 4, heads), "lse inside y");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, reinterpret_cast<float*>(reinterpret_cast<char*>(lse.p()) + 2), heads), "misaligned lse");
    REFUSED(bwd(h, nullptr, heads, heads, d, 1.0f, gq.p(), ld, gv.p()), "null lse");
    REFUSED(bwd(h, lse.p(), 1, heads, d, 1.0f, gq.p(), ld, gv.p()), "ldl < heads");
    REFUSED(bwd(h, lse.p(), heads, heads, d, 1.0f, nullptr, ld, gv.p()), "null gq");
    REFUSED(bwd(h, lse.p(), heads, heads, d, 1.0f, gq.p() + 2, ld, gv.p()), "misaligned gq");
    REFUSED(bwd(h, lse.p(), heads, heads, d, 1.0f, gq.p(), 10, gv.p()), "ldgq % 4");
    REFUSED(bwd(h, lse.p(), heads, heads, d, 1.0f, Q.p(), ld, gv.p()), "gq is q");
    REFUSED(bwd(h, lse.p(), heads, heads, d, 1.0f, gq.p(), ld, gk.p()), "gv is gk");
    REFUSED(bwd(h, lse.p(), heads, heads, d, 1.0f, lse.p(), ld, gv.p()), "gq is lse");
    REFUSED(hsmh_forward(h, nullptr, K.p(), V.p(), heads, d, 1.0f, y.p(), lse.p()), "host form: null q");
    REFUSED(hsmh_forward(h, Q.p(), K.p(), V.p(), heads, 6, 1.0f, y.p(), lse.p()), "host form: d = 6");
    REFUSED(hsmh_forward(h, Q.p(), K.p(), V.p(), heads, d, 1.0f, K.p(), lse.p()), "host form: y is k");
    REFUSED(hsmh_backward(h, Q.p(), K.p(), V.p(), G.p(), nullptr, heads, d, 1.0f, gq.p(), gk.p(), gv.p()), "host form: null lse");
    REFUSED(hsmh_backward(h, Q.p(), K.p(), V.p(), G.p(), lse.p(), 5, d, 1.0f, gq.p(), gk.p(), gv.p()), "host form: heads > max_heads");
    REFUSED(hsmh_backward(h, Q.p(), K.p(), V.p(), G.p(), lse.p(), heads, d, 1.0f, gq.p(), gq.p(), gv.p()), "host form: gk is gq");
#undef REFUSED
    // backward without HSMH_BACKWARD: refused in both forms, and the forward of that object runs
    EXPECT(bwd(fwd_only, lse.p(), heads, heads, d, 1.0f, gq.p(), ld, gv.p()) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(fwd_only), "HSMH_BACKWARD"), "backward without the flag");
    EXPECT(hsmh_backward(fwd_only, Q.p(), K.p(), V.p(), G.p(), lse.p(), heads, d, 1.0f, gq.p(), gk.p(), gv.p()) == HS_ERR_BAD_ARG, "backward without the flag");
    EXPECT(fwd(fwd_only, Q.p(), ld, heads, d, 1.0f, y.p(), ld, nullptr, 0) == HS_OK, "forward on an object without the flag");
    (void)w;
    EXPECT(hsmh_destroy(h) == HS_OK && hsmh_destroy(fwd_only) == HS_OK, "destroy");
}

}  // namespace

int main() {
    edges();
    refusals();
    if (g_failures) {
        std::printf("%d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("HEADS CPU OK\n");
    return 0;
}
