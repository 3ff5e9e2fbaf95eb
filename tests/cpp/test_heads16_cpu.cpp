// test_heads16_cpu.cpp — the CPU twin of include/hisparse_heads_bf16.h (hisparse_amd/csrc/hsmh_cpu.cpp) through its C boundary, as a
// program of its own: tests/test_heads16_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge
// patterns and the refusals of the header; buffers are exactly as large as the contract says (a feature operand ends with the 16-byte
// chunk of its last element, lse with head `heads - 1` of its last row), so a read or write past them is the sanitizer's.  Values are
// checked against long double loops per head with a tolerance of two bf16 ulps, far below any mistake of indexing (the bound itself is
// tests/heads16_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_heads_bf16.h"
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

float widen(uint16_t x) {
    const uint32_t bits = uint32_t(x) << 16;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
// a bf16 value of magnitude below `magnitude`: an fp32 word with its lower half cut off
uint16_t next_bf16(float magnitude) {
    const float f = (float(next_word() >> 8) / float(1 << 24) - 0.5f) * 2.0f * magnitude;
    uint32_t bits;
    std::memcpy(&bits, &f, 4);
    return uint16_t(bits >> 16);
}

constexpr uint16_t kNaN = 0x7FC0, kMark = 0xC0E0;      // -7.0

// n elements, 16-byte aligned, that end at most seven elements before the end of their allocation
struct Halves {
    std::vector<uint16_t> raw;
    uint16_t* base;
    explicit Halves(size_t count, uint16_t fill = 0) : raw((count ? count : 1) + 8, fill) {
        uintptr_t p = reinterpret_cast<uintptr_t>(raw.data() + 8);
        base = reinterpret_cast<uint16_t*>(p - p % 16);
    }
    uint16_t* p() { return base; }
    uint16_t& operator[](size_t i) { return base[i]; }
    float at(size_t i) const { return widen(base[i]); }
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

bool close_to(uint16_t got, long double want) { return std::fabs((long double)widen(got) - want) <= 0.0079L * (1e-3L + std::fabs(want)); }
bool close_to(float got, long double want) { return std::fabs((long double)got - want) <= 1e-4L * (1.0L + std::fabs(want)); }

void check_pattern(const Pattern& pt, uint32_t heads, uint32_t d, uint32_t pad, uint32_t ldl_extra, float scale) {
    const std::string what = pt.name + ", " + std::to_string(heads) + " heads of d " + std::to_string(d) + ", pad " + std::to_string(pad);
    hsmh_pattern* h = nullptr;
    EXPECT(hsmh_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr, heads, HSMH_BACKWARD) == HS_OK && h, what);
    if (!h) return;
    const uint32_t w = heads * d;
    const uint64_t ld = w + pad, ldl = heads + ldl_extra;
    const float mark = -7.0f, ninf = -std::numeric_limits<float>::infinity();
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + w : 0; };
    const size_t lse_words = size_t(pt.rows - 1) * ldl + heads;
    Halves Q(reach(pt.rows), kNaN), K(reach(pt.cols), kNaN), V(reach(pt.cols), kNaN), G(reach(pt.rows), kNaN);
    Halves y(reach(pt.rows), kMark), gq(reach(pt.rows), kMark), gk(reach(pt.cols), kMark), gv(reach(pt.cols), kMark);
    std::vector<float> lse(lse_words, mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < w; ++j) Q[r * ld + j] = next_bf16(2.0f), G[r * ld + j] = next_bf16(1.5f);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < w; ++j) K[c * ld + j] = next_bf16(2.0f), V[c * ld + j] = next_bf16(3.0f);
    EXPECT(hsmh16_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, heads, d, scale, y.p(), ld, lse.data(), ldl) == HS_OK, what);
    EXPECT(hsmh_sync(h) == HS_OK, what);
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
                for (uint32_t j = at; j < at + d; ++j) s += (long double)Q.at(r * ld + j) * K.at(pt.indices[e] * ld + j), gp[e - lo] += (long double)G.at(r * ld + j) * V.at(pt.indices[e] * ld + j);
                t[e - lo] = scale * s;
                m = std::fmax(m, t[e - lo]);
            }
            for (long double x : t) l += std::exp(x - m);
            want_l[size_t(r) * heads + hd] = m + std::log(l);
            for (uint64_t e = lo; e < hi; ++e)
                for (uint32_t j = at; j < at + d; ++j) want_y[size_t(r) * w + j] += std::exp(t[e - lo] - m) / l * V.at(pt.indices[e] * ld + j);
            const long double given = lse[r * ldl + hd];
            for (uint64_t e = lo; e < hi; ++e) t[e - lo] = std::exp(t[e - lo] - given), dsum += t[e - lo] * gp[e - lo];
            for (uint64_t e = lo; e < hi; ++e) {
                const uint32_t c = pt.indices[e];
                const long double gs = scale * t[e - lo] * (gp[e - lo] - dsum);
                for (uint32_t j = at; j < at + d; ++j) {
                    want_q[size_t(r) * w + j] += gs * K.at(c * ld + j);
                    want_k[size_t(c) * w + j] += gs * Q.at(r * ld + j);
                    want_v[size_t(c) * w + j] += t[e - lo] * G.at(r * ld + j);
                }
            }
        }
    }
    EXPECT(hsmh16_backward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.data(), ldl, heads, d, scale, gq.p(), ld, gk.p(), ld, gv.p(), ld) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const bool empty = pt.indptr[r] == pt.indptr[r + 1];
        for (uint32_t j = 0; j < w; ++j) {
            if (empty) EXPECT(y[r * ld + j] == 0 && gq[r * ld + j] == 0, what + ", an empty row is not 0x0000");
            else EXPECT(close_to(y[r * ld + j], want_y[size_t(r) * w + j]) && close_to(gq[r * ld + j], want_q[size_t(r) * w + j]), what + ", y and gq");
        }
        for (uint32_t hd = 0; hd < heads; ++hd) {
            if (empty) EXPECT(lse[r * ldl + hd] == ninf, what + ", lse of an empty row");
            else EXPECT(close_to(lse[r * ldl + hd], want_l[size_t(r) * heads + hd]), what + ", lse");
        }
        if (r + 1 < pt.rows) {
            for (uint64_t j = w; j < ld; ++j) EXPECT(y[r * ld + j] == kMark && gq[r * ld + j] == kMark, what + ", a pad element of y or gq was written");
            for (uint64_t j = heads; j < ldl; ++j) EXPECT(lse[r * ldl + j] == mark, what + ", a pad word of lse was written");
        }
    }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t j = 0; j < w; ++j) {
            if (!col_len[c]) EXPECT(gk[c * ld + j] == 0 && gv[c * ld + j] == 0, what + ", an empty column is not 0x0000");
            else EXPECT(close_to(gk[c * ld + j], want_k[size_t(c) * w + j]) && close_to(gv[c * ld + j], want_v[size_t(c) * w + j]), what + ", gk and gv");
        }
        if (c + 1 < pt.cols)
            for (uint64_t j = w; j < ld; ++j) EXPECT(gk[c * ld + j] == kMark && gv[c * ld + j] == kMark, what + ", a pad element of gk or gv was written");
    }
    // the host forms over arrays of exactly n * heads * d elements give the same words
    {
        std::vector<uint16_t> q(size_t(pt.rows) * w), g(q.size()), k(size_t(pt.cols) * w), v(k.size()), hy(q.size(), kMark), hq(q.size(), kMark), hk(k.size(), kMark), hv(k.size(), kMark);
        std::vector<float> hl(size_t(pt.rows) * heads, mark);
        for (uint32_t r = 0; r < pt.rows; ++r)
            for (uint32_t j = 0; j < w; ++j) q[size_t(r) * w + j] = Q[r * ld + j], g[size_t(r) * w + j] = G[r * ld + j];
        for (uint32_t c = 0; c < pt.cols; ++c)
            for (uint32_t j = 0; j < w; ++j) k[size_t(c) * w + j] = K[c * ld + j], v[size_t(c) * w + j] = V[c * ld + j];
        EXPECT(hsmh16_forward(h, q.data(), k.data(), v.data(), heads, d, scale, hy.data(), hl.data()) == HS_OK, what + ", host form");
        EXPECT(hsmh16_backward(h, q.data(), k.data(), v.data(), g.data(), hl.data(), heads, d, scale, hq.data(), hk.data(), hv.data()) == HS_OK, what + ", host form");
        bool same = true;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            same = same && !std::memcmp(&hy[size_t(r) * w], &y[r * ld], w * 2) && !std::memcmp(&hq[size_t(r) * w], &gq[r * ld], w * 2) &&
                   !std::memcmp(&hl[size_t(r) * heads], &lse[r * ldl], heads * 4);
        }
        for (uint32_t c = 0; c < pt.cols; ++c) same = same && !std::memcmp(&hk[size_t(c) * w], &gk[c * ld], w * 2) && !std::memcmp(&hv[size_t(c) * w], &gv[c * ld], w * 2);
        EXPECT(same, what + ", the host forms give other words than the device forms");
        std::vector<uint16_t> y2(q.size(), kMark);
        EXPECT(hsmh16_forward(h, q.data(), k.data(), v.data(), heads, d, scale, y2.data(), nullptr) == HS_OK && !std::memcmp(y2.data(), hy.data(), y2.size() * 2), what + ", lse NULL");
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
        check_pattern(pt, 3, 16, 8, 2, 1.5f);
        check_pattern(pt, 5, 8, 0, 0, -0.5f);
        check_pattern(pt, 1, 64, 16, 1, 0.25f);
    }
}

void refusals() {
    const Pattern pt = from_lengths("refusals", 9, {2, 0, 1, 3, 0, 1}, true);
    const uint32_t* ip = pt.indptr.data();
    const uint32_t* ix = pt.indices.data();
    Halves one(8);
    EXPECT(hsmh16_forward_device(nullptr, one.p(), 8, one.p(), 8, one.p(), 8, 1, 8, 1.0f, one.p(), 8, nullptr, 1) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmh16_forward(nullptr, one.p(), one.p(), one.p(), 1, 8, 1.0f, one.p(), nullptr) == HS_ERR_BAD_ARG, "null object");
    hsmh_pattern *h = nullptr, *fwd_only = nullptr;
    EXPECT(hsmh_create(&h, 0, 6, 9, ip, ix, 4, HSMH_BACKWARD) == HS_OK && h, "create");
    EXPECT(hsmh_create(&fwd_only, 0, 6, 9, ip, ix, 4, 0) == HS_OK && fwd_only, "create without the flag");
    if (!h || !fwd_only) return;
    const uint32_t heads = 2, d = 8;
    const uint64_t ld = 16;
    Halves Q(6 * ld, 0x3F00), K(9 * ld, 0x3E80), V(9 * ld, 0x3F80), G(6 * ld, 0xBF80), y(6 * ld), gq(6 * ld), gk(9 * ld), gv(9 * ld);
    std::vector<float> lse_store(6 * heads + 4);
    float* lse = lse_store.data();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto fwd = [&](hsmh_pattern* p, const uint16_t* q, uint64_t ldq, uint32_t hh, uint32_t dd, float sc, uint16_t* yy, uint64_t ldy, float* ll, uint64_t ldl) {
        return hsmh16_forward_device(p, q, ldq, K.p(), ld, V.p(), ld, hh, dd, sc, yy, ldy, ll, ldl);
    };
    auto bwd = [&](hsmh_pattern* p, const float* ll, uint64_t ldl, uint32_t hh, uint32_t dd, float sc, uint16_t* q_out, uint64_t ldgq, uint16_t* v_out) {
        return hsmh16_backward_device(p, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, ll, ldl, hh, dd, sc, q_out, ldgq, gk.p(), ld, v_out, ld);
    };
    auto good = [&](const std::string& after) {
        EXPECT(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, lse, heads) == HS_OK, std::string("the object is unusable after ") + after);
        EXPECT(bwd(h, lse, heads, heads, d, 1.0f, gq.p(), ld, gv.p()) == HS_OK, std::string("the object is unusable after ") + after);
    };
    good("nothing");
#define REFUSED(call, what)                                                              \
    do {                                                                                 \
        EXPECT((call) == HS_ERR_BAD_ARG && std::strlen(hsmh_last_error(h)), what);       \
        good(what);                                                                      \
    } while (0)
    for (uint32_t bad_d : {0u, 4u, 12u, 24u, 512u}) {
        REFUSED(fwd(h, Q.p(), ld, 1, bad_d, 1.0f, y.p(), ld, lse, 1), "d = " + std::to_string(bad_d));
        REFUSED(bwd(h, lse, 1, 1, bad_d, 1.0f, gq.p(), ld, gv.p()), "d = " + std::to_string(bad_d));
    }
    REFUSED(fwd(h, Q.p(), ld, 0, d, 1.0f, y.p(), ld, lse, heads), "heads = 0");
    REFUSED(fwd(h, Q.p(), 1024, 5, 8, 1.0f, y.p(), 1024, lse, 5), "heads > max_heads");
    REFUSED(fwd(h, Q.p(), 1024, 4, 256, 1.0f, y.p(), 1024, lse, 4), "heads * d = 1024");
    REFUSED(bwd(h, lse, 5, 5, 8, 1.0f, gq.p(), ld, gv.p()), "heads > max_heads");
    REFUSED(bwd(h, lse, 4, 4, 256, 1.0f, gq.p(), ld, gv.p()), "heads * d = 1024");
    for (float sc : {nan, inf, -inf}) {
        REFUSED(fwd(h, Q.p(), ld, heads, d, sc, y.p(), ld, lse, heads), "scale not finite");
        REFUSED(bwd(h, lse, heads, heads, d, sc, gq.p(), ld, gv.p()), "scale not finite");
    }
    REFUSED(fwd(h, nullptr, ld, heads, d, 1.0f, y.p(), ld, lse, heads), "null q");
    for (uint32_t off : {1u, 2u, 4u}) REFUSED(fwd(h, Q.p() + off, ld, heads, d, 1.0f, y.p(), ld, lse, heads), "q misaligned by " + std::to_string(2 * off) + " bytes");
    REFUSED(fwd(h, Q.p(), 20, heads, d, 1.0f, y.p(), ld, lse, heads), "ldq % 8");
    REFUSED(fwd(h, Q.p(), 8, heads, d, 1.0f, y.p(), ld, lse, heads), "ldq < heads * d");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, nullptr, ld, lse, heads), "null y");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), 8, lse, heads), "ldy < heads * d");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, lse, 1), "ldl < heads");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, Q.p(), ld, lse, heads), "y is q");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, reinterpret_cast<float*>(y.p() + 8), heads), "lse inside y");
    REFUSED(fwd(h, Q.p(), ld, heads, d, 1.0f, y.p(), ld, reinterpret_cast<float*>(reinterpret_cast<char*>(lse) + 2), heads), "misaligned lse");
    REFUSED(bwd(h, nullptr, heads, heads, d, 1.0f, gq.p(), ld, gv.p()), "null lse");
    REFUSED(bwd(h, lse, 1, heads, d, 1.0f, gq.p(), ld, gv.p()), "ldl < heads");
    REFUSED(bwd(h, lse, heads, heads, d, 1.0f, nullptr, ld, gv.p()), "null gq");
    REFUSED(bwd(h, lse, heads, heads, d, 1.0f, gq.p() + 4, ld, gv.p()), "misaligned gq");
    REFUSED(bwd(h, lse, heads, heads, d, 1.0f, gq.p(), 20, gv.p()), "ldgq % 8");
    REFUSED(bwd(h, lse, heads, heads, d, 1.0f, Q.p(), ld, gv.p()), "gq is q");
    REFUSED(bwd(h, lse, heads, heads, d, 1.0f, gq.p(), ld, gk.p()), "gv is gk");
    REFUSED(hsmh16_forward(h, nullptr, K.p(), V.p(), heads, d, 1.0f, y.p(), lse), "host form: null q");
    REFUSED(hsmh16_forward(h, Q.p(), K.p(), V.p(), heads, 4, 1.0f, y.p(), lse), "host form: d = 4");
    REFUSED(hsmh16_forward(h, Q.p(), K.p(), V.p(), heads, d, 1.0f, K.p(), lse), "host form: y is k");
    REFUSED(hsmh16_backward(h, Q.p(), K.p(), V.p(), G.p(), nullptr, heads, d, 1.0f, gq.p(), gk.p(), gv.p()), "host form: null lse");
    REFUSED(hsmh16_backward(h, Q.p(), K.p(), V.p(), G.p(), lse, 5, d, 1.0f, gq.p(), gk.p(), gv.p()), "host form: heads > max_heads");
    REFUSED(hsmh16_backward(h, Q.p(), K.p(), V.p(), G.p(), lse, heads, d, 1.0f, gq.p(), gq.p(), gv.p()), "host form: gk is gq");
#undef REFUSED
    // backward without HSMH_BACKWARD: refused in both forms, and the forward of that object runs
    EXPECT(bwd(fwd_only, lse, heads, heads, d, 1.0f, gq.p(), ld, gv.p()) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(fwd_only), "HSMH_BACKWARD"), "backward without the flag");
    EXPECT(hsmh16_backward(fwd_only, Q.p(), K.p(), V.p(), G.p(), lse, heads, d, 1.0f, gq.p(), gk.p(), gv.p()) == HS_ERR_BAD_ARG, "backward without the flag");
    EXPECT(fwd(fwd_only, Q.p(), ld, heads, d, 1.0f, y.p(), ld, nullptr, 0) == HS_OK, "forward on an object without the flag");
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
    std::printf("HEADS16 CPU OK\n");
    return 0;
}
