// test_gat_cpu.cpp — the CPU twin of include/hisparse_gat.h (hisparse_amd/csrc/hsmh_cpu.cpp) through its C boundary, as a program of its
// own: tests/test_gat_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge patterns and the
// refusals of the header; buffers are exactly as large as the contract says (a feature operand ends with the 16-byte chunk of its last
// word, a head array with head `heads - 1` of its last row), so a read or write past them is the sanitizer's.  Values are checked against
// long double loops per head with a tolerance far above the contract's bound and far below any mistake of indexing (the bound itself is
// tests/gat_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_gat.h"
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

void check_pattern(const Pattern& pt, uint32_t heads, uint32_t d, uint32_t pad, uint32_t extra, float slope) {
    const std::string what = pt.name + ", " + std::to_string(heads) + " heads of d " + std::to_string(d) + ", pad " + std::to_string(pad) + ", slope " + std::to_string(slope);
    hsmh_pattern* h = nullptr;
    EXPECT(hsmh_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr, heads, HSMH_BACKWARD) == HS_OK && h, what);
    if (!h) return;
    const uint32_t w = heads * d;
    const uint64_t ld = w + pad, ldh = heads + extra;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f, ninf = -std::numeric_limits<float>::infinity();
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + w : 0; };
    auto reach_h = [&](uint64_t n) { return n ? (n - 1) * ldh + heads : 0; };
    Floats EL(reach_h(pt.rows), nan), ER(reach_h(pt.cols), nan), V(reach(pt.cols), nan), G(reach(pt.rows), nan);
    Floats y(reach(pt.rows), mark), lse(reach_h(pt.rows), mark), gel(reach_h(pt.rows), mark), ger(reach_h(pt.cols), mark), gv(reach(pt.cols), mark);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        for (uint32_t hd = 0; hd < heads; ++hd) EL[r * ldh + hd] = next_float(2.0f);
        for (uint32_t j = 0; j < w; ++j) G[r * ld + j] = next_float(1.5f);
    }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t hd = 0; hd < heads; ++hd) ER[c * ldh + hd] = next_float(2.0f);
        for (uint32_t j = 0; j < w; ++j) V[c * ld + j] = next_float(3.0f);
    }
    EXPECT(hsgat_forward_device(h, EL.p(), ldh, ER.p(), ldh, V.p(), ld, heads, d, slope, y.p(), ld, lse.p(), ldh) == HS_OK, what);
    EXPECT(hsmh_sync(h) == HS_OK && hsmh_set_stream(h, nullptr) == HS_OK, what);
    // the forward per head in long double, then the gradients from the lse words the call wrote
    std::vector<long double> want_y(size_t(pt.rows) * w, 0), want_l(size_t(pt.rows) * heads, 0), want_a(size_t(pt.rows) * heads, 0), want_b(size_t(pt.cols) * heads, 0),
        want_v(size_t(pt.cols) * w, 0);
    std::vector<uint32_t> col_len(pt.cols, 0);
    for (uint64_t e = 0; e < pt.nnz(); ++e) ++col_len[pt.indices[e]];
    for (uint32_t hd = 0; hd < heads; ++hd) {
        const uint32_t at = hd * d;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            const uint64_t lo = pt.indptr[r], hi = pt.indptr[r + 1];
            if (lo == hi) continue;
            std::vector<long double> t(hi - lo), dx(hi - lo), gp(hi - lo, 0);
            long double m = -std::numeric_limits<long double>::infinity(), l = 0, dsum = 0;
            for (uint64_t e = lo; e < hi; ++e) {
                const float x = EL[r * ldh + hd] + ER[pt.indices[e] * ldh + hd];
                t[e - lo] = x > 0.0f ? x : slope * x;
                dx[e - lo] = x > 0.0f ? 1.0L : (long double)slope;
                for (uint32_t j = at; j < at + d; ++j) gp[e - lo] += (long double)G[r * ld + j] * V[pt.indices[e] * ld + j];
                m = std::fmax(m, t[e - lo]);
            }
            for (long double x : t) l += std::exp(x - m);
            want_l[size_t(r) * heads + hd] = m + std::log(l);
            for (uint64_t e = lo; e < hi; ++e)
                for (uint32_t j = at; j < at + d; ++j) want_y[size_t(r) * w + j] += std::exp(t[e - lo] - m) / l * V[pt.indices[e] * ld + j];
            const long double given = lse[r * ldh + hd];
            for (uint64_t e = lo; e < hi; ++e) t[e - lo] = std::exp(t[e - lo] - given), dsum += t[e - lo] * gp[e - lo];
            for (uint64_t e = lo; e < hi; ++e) {
                const uint32_t c = pt.indices[e];
                const long double gx = t[e - lo] * (gp[e - lo] - dsum) * dx[e - lo];
                want_a[size_t(r) * heads + hd] += gx;
                want_b[size_t(c) * heads + hd] += gx;
                for (uint32_t j = at; j < at + d; ++j) want_v[size_t(c) * w + j] += t[e - lo] * G[r * ld + j];
            }
        }
    }
    EXPECT(hsgat_backward_device(h, EL.p(), ldh, ER.p(), ldh, V.p(), ld, G.p(), ld, lse.p(), ldh, heads, d, slope, gel.p(), ldh, ger.p(), ldh, gv.p(), ld) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const bool empty = pt.indptr[r] == pt.indptr[r + 1];
        for (uint32_t j = 0; j < w; ++j) {
            if (empty) EXPECT(plus_zero(y[r * ld + j]), what + ", an empty row");
            else EXPECT(close_to(y[r * ld + j], want_y[size_t(r) * w + j]), what + ", y");
        }
        for (uint32_t hd = 0; hd < heads; ++hd) {
            if (empty) EXPECT(lse[r * ldh + hd] == ninf && plus_zero(gel[r * ldh + hd]), what + ", lse and gel of an empty row");
            else EXPECT(close_to(lse[r * ldh + hd], want_l[size_t(r) * heads + hd]) && close_to(gel[r * ldh + hd], want_a[size_t(r) * heads + hd]), what + ", lse and gel");
        }
        if (r + 1 < pt.rows) {
            for (uint64_t j = w; j < ld; ++j) EXPECT(y[r * ld + j] == mark, what + ", a pad word of y was written");
            for (uint64_t j = heads; j < ldh; ++j) EXPECT(lse[r * ldh + j] == mark && gel[r * ldh + j] == mark, what + ", a pad word of lse or gel was written");
        }
    }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t j = 0; j < w; ++j) {
            if (!col_len[c]) EXPECT(plus_zero(gv[c * ld + j]), what + ", an empty column");
            else EXPECT(close_to(gv[c * ld + j], want_v[size_t(c) * w + j]), what + ", gv");
        }
        for (uint32_t hd = 0; hd < heads; ++hd) {
            if (!col_len[c]) EXPECT(plus_zero(ger[c * ldh + hd]), what + ", ger of an empty column");
            else EXPECT(close_to(ger[c * ldh + hd], want_b[size_t(c) * heads + hd]), what + ", ger");
        }
        if (c + 1 < pt.cols) {
            for (uint64_t j = w; j < ld; ++j) EXPECT(gv[c * ld + j] == mark, what + ", a pad word of gv was written");
            for (uint64_t j = heads; j < ldh; ++j) EXPECT(ger[c * ldh + j] == mark, what + ", a pad word of ger was written");
        }
    }
    // the host forms over arrays of exactly n * heads * d and n * heads words give the same words
    {
        std::vector<float> a(size_t(pt.rows) * heads), b(size_t(pt.cols) * heads), g(size_t(pt.rows) * w), v(size_t(pt.cols) * w), hy(g.size(), mark), hl(a.size(), mark),
            ha(a.size(), mark), hb(b.size(), mark), hv(v.size(), mark);
        for (uint32_t r = 0; r < pt.rows; ++r) {
            for (uint32_t hd = 0; hd < heads; ++hd) a[size_t(r) * heads + hd] = EL[r * ldh + hd];
            for (uint32_t j = 0; j < w; ++j) g[size_t(r) * w + j] = G[r * ld + j];
        }
        for (uint32_t c = 0; c < pt.cols; ++c) {
            for (uint32_t hd = 0; hd < heads; ++hd) b[size_t(c) * heads + hd] = ER[c * ldh + hd];
            for (uint32_t j = 0; j < w; ++j) v[size_t(c) * w + j] = V[c * ld + j];
        }
        EXPECT(hsgat_forward(h, a.data(), b.data(), v.data(), heads, d, slope, hy.data(), hl.data()) == HS_OK, what + ", host form");
        EXPECT(hsgat_backward(h, a.data(), b.data(), v.data(), g.data(), hl.data(), heads, d, slope, ha.data(), hb.data(), hv.data()) == HS_OK, what + ", host form");
        bool same = true;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            same = same && !std::memcmp(&hy[size_t(r) * w], &y[r * ld], w * 4) && !std::memcmp(&hl[size_t(r) * heads], &lse[r * ldh], heads * 4) &&
                   !std::memcmp(&ha[size_t(r) * heads], &gel[r * ldh], heads * 4);
        }
        for (uint32_t c = 0; c < pt.cols; ++c) same = same && !std::memcmp(&hb[size_t(c) * heads], &ger[c * ldh], heads * 4) && !std::memcmp(&hv[size_t(c) * w], &gv[c * ld], w * 4);
        EXPECT(same, what + ", the host forms give other words than the device forms");
        std::vector<float> y2(g.size(), mark);
        EXPECT(hsgat_forward(h, a.data(), b.data(), v.data(), heads, d, slope, y2.data(), nullptr) == HS_OK && !std::memcmp(y2.data(), hy.data(), y2.size() * 4), what + ", lse NULL");
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
        check_pattern(pt, 3, 8, 8, 2, 0.2f);
        check_pattern(pt, 5, 4, 0, 0, 0.0f);
        check_pattern(pt, 1, 64, 4, 1, 1.0f);
    }
}

void refusals() {
    const Pattern pt = from_lengths("refusals", 9, {2, 0, 1, 3, 0, 1}, true);
    const uint32_t* ip = pt.indptr.data();
    const uint32_t* ix = pt.indices.data();
    Floats one(4);
    EXPECT(hsgat_forward_device(nullptr, one.p(), 1, one.p(), 1, one.p(), 4, 1, 4, 0.2f, one.p(), 4, nullptr, 1) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsgat_forward(nullptr, one.p(), one.p(), one.p(), 1, 4, 0.2f, one.p(), nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsgat_backward_device(nullptr, one.p(), 1, one.p(), 1, one.p(), 4, one.p(), 4, one.p(), 1, 1, 4, 0.2f, one.p(), 1, one.p(), 1, one.p(), 4) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsgat_backward(nullptr, one.p(), one.p(), one.p(), one.p(), one.p(), 1, 4, 0.2f, one.p(), one.p(), one.p()) == HS_ERR_BAD_ARG, "null object");

    hsmh_pattern* h = nullptr;
    hsmh_pattern* fwd_only = nullptr;
    EXPECT(hsmh_create(&h, 0, 6, 9, ip, ix, 4, HSMH_BACKWARD) == HS_OK && h, "create");
    EXPECT(hsmh_create(&fwd_only, 0, 6, 9, ip, ix, 4, 0) == HS_OK && fwd_only, "create without the flag");
    if (!h || !fwd_only) return;
    const uint32_t heads = 2, d = 4;
    const uint64_t ld = 8, ldh = 2;
    Floats EL(6 * ldh, 0.5f), ER(9 * ldh, -0.25f), V(9 * ld, 1.0f), G(6 * ld, -1.0f), y(6 * ld), lse(6 * ldh), gel(6 * ldh), ger(9 * ldh), gv(9 * ld);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto fwd = [&](hsmh_pattern* p, const float* el, uint64_t ldel, uint32_t hh, uint32_t dd, float sl, float* yy, uint64_t ldy, float* ll, uint64_t ldl) {
        return hsgat_forward_device(p, el, ldel, ER.p(), ldh, V.p(), ld, hh, dd, sl, yy, ldy, ll, ldl);
    };
    auto bwd = [&](hsmh_pattern* p, const float* ll, uint64_t ldl, uint32_t hh, uint32_t dd, float sl, float* a_out, uint64_t ldgel, float* b_out, float* v_out, uint64_t ldgv) {
        return hsgat_backward_device(p, EL.p(), ldh, ER.p(), ldh, V.p(), ld, G.p(), ld, ll, ldl, hh, dd, sl, a_out, ldgel, b_out, ldh, v_out, ldgv);
    };
    auto good = [&](const std::string& after) {
        EXPECT(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p(), ld, lse.p(), ldh) == HS_OK, std::string("the object is unusable after ") + after);
        EXPECT(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, ger.p(), gv.p(), ld) == HS_OK, std::string("the object is unusable after ") + after);
    };
    good("nothing");
#define REFUSED(call, what)                                                              \
    do {                                                                                 \
        EXPECT((call) == HS_ERR_BAD_ARG && std::strlen(hsmh_last_error(h)), what);       \
        good(what);                                                                      \
    } while (0)
    for (float sl : {nan, inf, -inf, -0.5f, -1.4e-45f}) {
        REFUSED(fwd(h, EL.p(), ldh, heads, d, sl, y.p(), ld, lse.p(), ldh), "slope not finite or below 0");
        REFUSED(bwd(h, lse.p(), ldh, heads, d, sl, gel.p(), ldh, ger.p(), gv.p(), ld), "slope not finite or below 0");
    }
    EXPECT(fwd(h, EL.p(), ldh, heads, d, -0.0f, y.p(), ld, lse.p(), ldh) == HS_OK && bwd(h, lse.p(), ldh, heads, d, -0.0f, gel.p(), ldh, ger.p(), gv.p(), ld) == HS_OK, "slope -0.0 counts as 0");
    for (uint32_t bad_d : {0u, 1u, 2u, 3u, 5u, 6u, 12u, 512u}) {
        REFUSED(fwd(h, EL.p(), ldh, 1, bad_d, 0.2f, y.p(), 512, lse.p(), 1), "d = " + std::to_string(bad_d));
        REFUSED(bwd(h, lse.p(), 1, 1, bad_d, 0.2f, gel.p(), ldh, ger.p(), gv.p(), 512), "d = " + std::to_string(bad_d));
    }
    REFUSED(fwd(h, EL.p(), ldh, 0, d, 0.2f, y.p(), ld, lse.p(), ldh), "heads = 0");
    REFUSED(fwd(h, EL.p(), 5, 5, 4, 0.2f, y.p(), 512, lse.p(), 5), "heads > max_heads");
    REFUSED(fwd(h, EL.p(), 4, 4, 128, 0.2f, y.p(), 512, lse.p(), 4), "heads * d = 512");
    REFUSED(bwd(h, lse.p(), 5, 5, 4, 0.2f, gel.p(), 5, ger.p(), gv.p(), 512), "heads > max_heads");
    REFUSED(fwd(h, nullptr, ldh, heads, d, 0.2f, y.p(), ld, lse.p(), ldh), "null el");
    REFUSED(fwd(h, reinterpret_cast<float*>(reinterpret_cast<char*>(EL.p()) + 2), ldh, heads, d, 0.2f, y.p(), ld, lse.p(), ldh), "misaligned el");
    REFUSED(fwd(h, EL.p(), 1, heads, d, 0.2f, y.p(), ld, lse.p(), ldh), "ldel < heads");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, nullptr, ld, lse.p(), ldh), "null y");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p() + 1, ld, lse.p(), ldh), "misaligned y");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p(), 10, lse.p(), ldh), "ldy % 4");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p(), 4, lse.p(), ldh), "ldy < heads * d");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p(), ld, lse.p(), 1), "ldl < heads");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, V.p(), ld, lse.p(), ldh), "y is v");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p(), ld, EL.p(), ldh), "lse is el");
    REFUSED(fwd(h, EL.p(), ldh, heads, d, 0.2f, y.p(), ld, y.p() + 4, ldh), "lse inside y");
    REFUSED(bwd(h, nullptr, ldh, heads, d, 0.2f, gel.p(), ldh, ger.p(), gv.p(), ld), "null lse");
    REFUSED(bwd(h, lse.p(), 1, heads, d, 0.2f, gel.p(), ldh, ger.p(), gv.p(), ld), "ldl < heads");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, nullptr, ldh, ger.p(), gv.p(), ld), "null gel");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), 1, ger.p(), gv.p(), ld), "ldgel < heads");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, nullptr, gv.p(), ld), "null ger");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, ger.p(), gv.p() + 2, ld), "misaligned gv");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, ger.p(), gv.p(), 10), "ldgv % 4");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, EL.p(), ldh, ger.p(), gv.p(), ld), "gel is el");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, ER.p(), gv.p(), ld), "ger is er");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, gel.p(), gv.p(), ld), "ger is gel");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, lse.p(), ldh, ger.p(), gv.p(), ld), "gel is lse");
    REFUSED(bwd(h, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, ger.p(), G.p(), ld), "gv is gy");
    REFUSED(hsgat_forward(h, nullptr, ER.p(), V.p(), heads, d, 0.2f, y.p(), lse.p()), "host form: null el");
    REFUSED(hsgat_forward(h, EL.p(), ER.p(), V.p(), heads, 6, 0.2f, y.p(), lse.p()), "host form: d = 6");
    REFUSED(hsgat_forward(h, EL.p(), ER.p(), V.p(), heads, d, -1.0f, y.p(), lse.p()), "host form: slope -1");
    REFUSED(hsgat_forward(h, EL.p(), ER.p(), V.p(), heads, d, 0.2f, V.p(), lse.p()), "host form: y is v");
    REFUSED(hsgat_backward(h, EL.p(), ER.p(), V.p(), G.p(), nullptr, heads, d, 0.2f, gel.p(), ger.p(), gv.p()), "host form: null lse");
    REFUSED(hsgat_backward(h, EL.p(), ER.p(), V.p(), G.p(), lse.p(), 5, d, 0.2f, gel.p(), ger.p(), gv.p()), "host form: heads > max_heads");
    REFUSED(hsgat_backward(h, EL.p(), ER.p(), V.p(), G.p(), lse.p(), heads, d, 0.2f, gel.p(), gel.p(), gv.p()), "host form: ger is gel");
#undef REFUSED
    // backward without HSMH_BACKWARD: refused in both forms with the flag named, and the forward of that object runs
    EXPECT(bwd(fwd_only, lse.p(), ldh, heads, d, 0.2f, gel.p(), ldh, ger.p(), gv.p(), ld) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(fwd_only), "HSMH_BACKWARD"),
           "backward without the flag");
    EXPECT(hsgat_backward(fwd_only, EL.p(), ER.p(), V.p(), G.p(), lse.p(), heads, d, 0.2f, gel.p(), ger.p(), gv.p()) == HS_ERR_BAD_ARG, "backward without the flag");
    EXPECT(fwd(fwd_only, EL.p(), ldh, heads, d, 0.2f, y.p(), ld, nullptr, 0) == HS_OK, "forward on an object without the flag");
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
    std::printf("GAT CPU OK\n");
    return 0;
}
