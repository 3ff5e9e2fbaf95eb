// test_heads16_dropout_cpu.cpp — the CPU twin of include/hisparse_heads_dropout_bf16.h (hisparse_amd/csrc/hsmh_cpu.cpp) through its C
// boundary, as a program of its own: tests/test_heads16_dropout_cpu.py compiles both files with -fsanitize=address,undefined and runs the
// result.  The edge patterns and the refusals of the header; buffers are exactly as large as the contract says (a bf16 feature operand
// ends with its last row's element heads * d - 1, lse with head `heads - 1` of its last row, bias and gbias with head `heads - 1` of
// their last entry, and with nnz = 0 they hold nothing at all), so a read or write past them is the sanitizer's.  Values are checked
// against long double loops per head, weighted by the mask of hsmhd_keep_mask, with a tolerance of one bf16 ulp: far above the contract's
// bound and far below any mistake of indexing (the bound itself is tests/heads16_dropout_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "hisparse_heads_bf16.h"
#include "hisparse_heads_bias.h"
#include "hisparse_heads_dropout.h"
#include "hisparse_heads_dropout_bf16.h"
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

float widen(uint16_t x) {
    const uint32_t bits = uint32_t(x) << 16;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
uint16_t narrow(float f) {      // nearest even; the values here are finite
    uint32_t bits;
    std::memcpy(&bits, &f, 4);
    return uint16_t((bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16);
}
uint16_t next_bf16(float magnitude) { return narrow(next_float(magnitude)); }

constexpr uint16_t kNaN16 = 0x7FC0, kMark16 = 0xDEAD;

// exactly n elements on the heap (16-byte aligned by operator new[] for n * sizeof(T) >= 16, which every operand here is or is never
// dereferenced): element n belongs to nobody.  With n = 0 the pointer is valid and may not be dereferenced.
template <typename T>
struct Exact {
    std::unique_ptr<T[]> mem;
    size_t n;
    explicit Exact(size_t count, T fill) : mem(new T[count]), n(count) {
        for (size_t i = 0; i < n; ++i) mem[i] = fill;
    }
    T* p() { return mem.get(); }
    T& operator[](size_t i) { return mem[i]; }
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

// a bf16 output word: one bf16 ulp (2^-7 relative) and a little absolute room
bool close16(uint16_t got, long double want) { return std::fabs((long double)widen(got) - want) <= 0x1p-7L * std::fabs(want) + 1e-4L; }
bool close_to(float got, long double want) { return std::fabs((long double)got - want) <= 1e-4L * (1.0L + std::fabs(want)); }

void check_pattern(const Pattern& pt, uint32_t heads, uint32_t d, uint32_t pad, uint32_t extra, float scale, float drop_p, bool with_bias) {
    const std::string what = pt.name + ", " + std::to_string(heads) + " heads of d " + std::to_string(d) + ", pad " + std::to_string(pad) + ", drop_p " + std::to_string(drop_p) +
                             (with_bias ? ", a bias" : ", bias NULL");
    const uint64_t seed = 0x123456789ABCDEFull + heads, offset = (uint64_t(3) << 32) + d;
    hsmh_pattern* h = nullptr;
    EXPECT(hsmhb_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr, heads, HSMH_BACKWARD) == HS_OK && h, what);
    if (!h) return;
    const uint32_t w = heads * d;
    const uint64_t ld = w + pad, ldl = heads + extra, ldb = heads + extra, ldgb = heads + extra + 1;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f, ninf = -std::numeric_limits<float>::infinity();
    const long double c = 1.0L / (1.0L - (long double)drop_p);
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + w : 0; };
    auto entry_reach = [&](uint64_t l) { return pt.nnz() ? (pt.nnz() - 1) * l + heads : 0; };
    const size_t lse_words = size_t(pt.rows - 1) * ldl + heads;
    Exact<uint16_t> Q(reach(pt.rows), kNaN16), K(reach(pt.cols), kNaN16), V(reach(pt.cols), kNaN16), G(reach(pt.rows), kNaN16);
    Exact<uint16_t> y(reach(pt.rows), kMark16), gq(reach(pt.rows), kMark16), gk(reach(pt.cols), kMark16), gv(reach(pt.cols), kMark16);
    Exact<float> lse(lse_words, mark), B(entry_reach(ldb), nan), gb(entry_reach(ldgb), mark);
    Exact<uint8_t> keep(size_t(pt.nnz()) * heads, 9);
    EXPECT(hsmhd_keep_mask(pt.nnz(), heads, drop_p, seed, offset, keep.p()) == HS_OK, what + ", the mask");
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < w; ++j) Q[r * ld + j] = next_bf16(2.0f), G[r * ld + j] = next_bf16(1.5f);
    for (uint32_t cc = 0; cc < pt.cols; ++cc)
        for (uint32_t j = 0; j < w; ++j) K[cc * ld + j] = next_bf16(2.0f), V[cc * ld + j] = next_bf16(3.0f);
    for (uint64_t e = 0; e < pt.nnz(); ++e)
        for (uint32_t hd = 0; hd < heads; ++hd) B[e * ldb + hd] = next_float(4.0f);
    const float* bias = with_bias ? B.p() : nullptr;
    EXPECT(hsmhd16_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, bias, with_bias ? ldb : 0, heads, d, scale, drop_p, seed, offset, y.p(), ld, lse.p(), ldl) == HS_OK, what);
    EXPECT(hsmh_sync(h) == HS_OK, what);
    std::vector<long double> want_y(size_t(pt.rows) * w, 0), want_l(size_t(pt.rows) * heads, 0), want_q(size_t(pt.rows) * w, 0), want_k(size_t(pt.cols) * w, 0),
        want_v(size_t(pt.cols) * w, 0), want_b(size_t(pt.nnz()) * heads, 0);
    std::vector<uint32_t> col_len(pt.cols, 0);
    for (uint64_t e = 0; e < pt.nnz(); ++e) ++col_len[pt.indices[e]];
    for (uint32_t hd = 0; hd < heads; ++hd) {
        const uint32_t at = hd * d;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            const uint64_t lo = pt.indptr[r], hi = pt.indptr[r + 1];
            if (lo == hi) continue;
            std::vector<long double> t(hi - lo), gp(hi - lo, 0), wt(hi - lo, 0);
            long double m = -std::numeric_limits<long double>::infinity(), l = 0, dsum = 0;
            for (uint64_t e = lo; e < hi; ++e) {
                long double s = 0;
                for (uint32_t j = at; j < at + d; ++j) {
                    s += (long double)widen(Q[r * ld + j]) * widen(K[pt.indices[e] * ld + j]);
                    gp[e - lo] += (long double)widen(G[r * ld + j]) * widen(V[pt.indices[e] * ld + j]);
                }
                wt[e - lo] = keep[e * heads + hd] ? c : 0.0L;
                gp[e - lo] *= wt[e - lo];
                t[e - lo] = scale * s + (with_bias ? B[e * ldb + hd] : 0.0f);
                m = std::fmax(m, t[e - lo]);
            }
            for (long double x : t) l += std::exp(x - m);
            want_l[size_t(r) * heads + hd] = m + std::log(l);
            for (uint64_t e = lo; e < hi; ++e)
                for (uint32_t j = at; j < at + d; ++j) want_y[size_t(r) * w + j] += wt[e - lo] * std::exp(t[e - lo] - m) / l * widen(V[pt.indices[e] * ld + j]);
            const long double given = lse[r * ldl + hd];
            for (uint64_t e = lo; e < hi; ++e) t[e - lo] = std::exp(t[e - lo] - given), dsum += t[e - lo] * gp[e - lo];
            for (uint64_t e = lo; e < hi; ++e) {
                const uint32_t cc = pt.indices[e];
                const long double gbe = t[e - lo] * (gp[e - lo] - dsum), gs = scale * gbe;
                want_b[size_t(e) * heads + hd] = gbe;
                for (uint32_t j = at; j < at + d; ++j) {
                    want_q[size_t(r) * w + j] += gs * widen(K[cc * ld + j]);
                    want_k[size_t(cc) * w + j] += gs * widen(Q[r * ld + j]);
                    want_v[size_t(cc) * w + j] += wt[e - lo] * t[e - lo] * widen(G[r * ld + j]);
                }
            }
        }
    }
    EXPECT(hsmhd16_backward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.p(), ldl, bias, with_bias ? ldb : 0, heads, d, scale, drop_p, seed, offset, gq.p(), ld, gk.p(), ld,
                                   gv.p(), ld, gb.p(), ldgb) == HS_OK,
           what);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const bool empty = pt.indptr[r] == pt.indptr[r + 1];
        for (uint32_t j = 0; j < w; ++j) {
            if (empty) EXPECT(y[r * ld + j] == 0 && gq[r * ld + j] == 0, what + ", an empty row is not 0x0000");
            else EXPECT(close16(y[r * ld + j], want_y[size_t(r) * w + j]) && close16(gq[r * ld + j], want_q[size_t(r) * w + j]), what + ", y and gq");
        }
        for (uint32_t hd = 0; hd < heads; ++hd) {
            if (empty) EXPECT(lse[r * ldl + hd] == ninf, what + ", lse of an empty row");
            else EXPECT(close_to(lse[r * ldl + hd], want_l[size_t(r) * heads + hd]), what + ", lse");
        }
        if (r + 1 < pt.rows)
            for (uint64_t j = w; j < ld; ++j) EXPECT(y[r * ld + j] == kMark16 && gq[r * ld + j] == kMark16, what + ", a pad element of y or gq was written");
    }
    for (uint32_t cc = 0; cc < pt.cols; ++cc) {
        for (uint32_t j = 0; j < w; ++j) {
            if (!col_len[cc]) EXPECT(gk[cc * ld + j] == 0 && gv[cc * ld + j] == 0, what + ", an empty column is not 0x0000");
            else EXPECT(close16(gk[cc * ld + j], want_k[size_t(cc) * w + j]) && close16(gv[cc * ld + j], want_v[size_t(cc) * w + j]), what + ", gk and gv");
        }
    }
    for (uint64_t e = 0; e < pt.nnz(); ++e) {
        for (uint32_t hd = 0; hd < heads; ++hd) EXPECT(close_to(gb[e * ldgb + hd], want_b[size_t(e) * heads + hd]), what + ", gbias");
        if (e + 1 < pt.nnz())
            for (uint64_t j = heads; j < ldgb; ++j) EXPECT(gb[e * ldgb + j] == mark, what + ", a word h >= heads of gbias was written");
    }
    // gbias NULL: the same three gradients; the host forms over arrays of exactly the contract's sizes: the same words
    {
        Exact<uint16_t> q2(reach(pt.rows), kMark16), k2(reach(pt.cols), kMark16), v2(reach(pt.cols), kMark16);
        EXPECT(hsmhd16_backward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.p(), ldl, bias, with_bias ? ldb : 0, heads, d, scale, drop_p, seed, offset, q2.p(), ld, k2.p(), ld,
                                       v2.p(), ld, nullptr, 0) == HS_OK,
               what + ", gbias NULL");
        EXPECT(!std::memcmp(q2.p(), gq.p(), reach(pt.rows) * 2) && !std::memcmp(k2.p(), gk.p(), reach(pt.cols) * 2) && !std::memcmp(v2.p(), gv.p(), reach(pt.cols) * 2),
               what + ", gbias NULL changes a gradient");
        Exact<uint16_t> q(size_t(pt.rows) * w, 0), g(size_t(pt.rows) * w, 0), k(size_t(pt.cols) * w, 0), v(size_t(pt.cols) * w, 0), hy(size_t(pt.rows) * w, kMark16),
            hq(size_t(pt.rows) * w, kMark16), hk(size_t(pt.cols) * w, kMark16), hv(size_t(pt.cols) * w, kMark16);
        Exact<float> hl(size_t(pt.rows) * heads, mark), hb(size_t(pt.nnz()) * heads, nan), hgb(size_t(pt.nnz()) * heads, mark);
        for (uint32_t r = 0; r < pt.rows; ++r)
            for (uint32_t j = 0; j < w; ++j) q[size_t(r) * w + j] = Q[r * ld + j], g[size_t(r) * w + j] = G[r * ld + j];
        for (uint32_t cc = 0; cc < pt.cols; ++cc)
            for (uint32_t j = 0; j < w; ++j) k[size_t(cc) * w + j] = K[cc * ld + j], v[size_t(cc) * w + j] = V[cc * ld + j];
        for (uint64_t e = 0; e < pt.nnz(); ++e)
            for (uint32_t hd = 0; hd < heads; ++hd) hb[e * heads + hd] = B[e * ldb + hd];
        const float* hbias = with_bias ? hb.p() : nullptr;
        EXPECT(hsmhd16_forward(h, q.p(), k.p(), v.p(), hbias, heads, d, scale, drop_p, seed, offset, hy.p(), hl.p()) == HS_OK, what + ", host form");
        EXPECT(hsmhd16_backward(h, q.p(), k.p(), v.p(), g.p(), hl.p(), hbias, heads, d, scale, drop_p, seed, offset, hq.p(), hk.p(), hv.p(), hgb.p()) == HS_OK, what + ", host form");
        bool same = true;
        for (uint32_t r = 0; r < pt.rows; ++r) {
            same = same && !std::memcmp(&hy[size_t(r) * w], &y[r * ld], w * 2) && !std::memcmp(&hq[size_t(r) * w], &gq[r * ld], w * 2) &&
                   !std::memcmp(&hl[size_t(r) * heads], &lse[r * ldl], heads * 4);
        }
        for (uint32_t cc = 0; cc < pt.cols; ++cc) same = same && !std::memcmp(&hk[size_t(cc) * w], &gk[cc * ld], w * 2) && !std::memcmp(&hv[size_t(cc) * w], &gv[cc * ld], w * 2);
        for (uint64_t e = 0; e < pt.nnz(); ++e) same = same && !std::memcmp(&hgb[e * heads], &gb[e * ldgb], heads * 4);
        EXPECT(same, what + ", the host forms give other words than the device forms");
        // drop_p = 0 with bias NULL gives the words of hsmh16_forward_device, and lse at any drop_p is the lse without dropout
        Exact<uint16_t> y0(reach(pt.rows), kMark16), y1(reach(pt.rows), kMark16), y2(reach(pt.rows), kMark16);
        Exact<float> l0(lse_words, mark), l1(lse_words, mark), l2(lse_words, mark);
        EXPECT(hsmh16_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, heads, d, scale, y0.p(), ld, l0.p(), ldl) == HS_OK, what + ", the bf16 forward without bias and dropout");
        EXPECT(hsmhd16_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, nullptr, 0, heads, d, scale, 0.0f, seed, offset, y1.p(), ld, l1.p(), ldl) == HS_OK, what + ", drop_p 0, bias NULL");
        EXPECT(!std::memcmp(y0.p(), y1.p(), reach(pt.rows) * 2) && !std::memcmp(l0.p(), l1.p(), lse_words * 4), what + ", drop_p 0 and bias NULL change the forward");
        EXPECT(hsmhd16_forward_device(h, Q.p(), ld, K.p(), ld, V.p(), ld, bias, with_bias ? ldb : 0, heads, d, scale, 0.0f, seed, offset, y2.p(), ld, l2.p(), ldl) == HS_OK, what + ", drop_p 0");
        EXPECT(!std::memcmp(l2.p(), lse.p(), lse_words * 4), what + ", lse is not the lse without dropout");
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
        check_pattern(pt, 3, 8, 8, 2, 1.5f, 0.5f, true);
        check_pattern(pt, 5, 8, 0, 0, -0.5f, 0.9f, false);
        check_pattern(pt, 1, 64, 16, 1, 0.25f, 0.1f, true);
        check_pattern(pt, 8, 16, 0, 1, 0.5f, 0.5f, false);
    }
}

void refusals() {
    const Pattern pt = from_lengths("refusals", 9, {2, 0, 1, 3, 0, 1}, true);
    const uint32_t* ip = pt.indptr.data();
    const uint32_t* ix = pt.indices.data();
    Exact<uint16_t> one(8, 0);
    Exact<float> onef(4, 0.0f);
    EXPECT(hsmhd16_forward_device(nullptr, one.p(), 8, one.p(), 8, one.p(), 8, onef.p(), 1, 1, 8, 1.0f, 0.5f, 1, 1, one.p(), 8, nullptr, 1) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmhd16_forward(nullptr, one.p(), one.p(), one.p(), onef.p(), 1, 8, 1.0f, 0.5f, 1, 1, one.p(), nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsmhd16_backward_device(nullptr, one.p(), 8, one.p(), 8, one.p(), 8, one.p(), 8, onef.p(), 1, onef.p(), 1, 1, 8, 1.0f, 0.5f, 1, 1, one.p(), 8, one.p(), 8, one.p(), 8, nullptr, 1) ==
               HS_ERR_BAD_ARG,
           "null object");
    EXPECT(hsmhd16_backward(nullptr, one.p(), one.p(), one.p(), one.p(), onef.p(), onef.p(), 1, 8, 1.0f, 0.5f, 1, 1, one.p(), one.p(), one.p(), nullptr) == HS_ERR_BAD_ARG, "null object");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float bad_drops[] = {1.0f, -0.1f, nan, inf, -inf, 1.5f};

    hsmh_pattern *h = nullptr, *plain = nullptr, *no_flag = nullptr;
    EXPECT(hsmhb_create(&h, 0, 6, 9, ip, ix, 4, HSMH_BACKWARD) == HS_OK && h, "create");
    EXPECT(hsmh_create(&plain, 0, 6, 9, ip, ix, 4, HSMH_BACKWARD) == HS_OK && plain, "plain create");
    EXPECT(hsmhb_create(&no_flag, 0, 6, 9, ip, ix, 4, 0) == HS_OK && no_flag, "create without the flag");
    if (!h || !plain || !no_flag) return;
    const uint32_t heads = 2, d = 8;
    const uint64_t ld = 16, nnz = pt.nnz();
    Exact<uint16_t> Q(6 * ld, narrow(0.5f)), K(9 * ld, narrow(0.25f)), V(9 * ld, narrow(1.0f)), G(6 * ld, narrow(-1.0f)), y(6 * ld, 0), gq(6 * ld, 0), gk(9 * ld, 0), gv(9 * ld, 0);
    Exact<float> lse(6 * heads, 0.0f), B(nnz * 4, 0.125f), gb(nnz * 4, 0.0f);
    auto fwd = [&](hsmh_pattern* p, const float* b, uint64_t ldb, float drop, uint16_t* yy, float* ll, uint32_t dd = 8, uint64_t ldq = 16) {
        return hsmhd16_forward_device(p, Q.p(), ldq, K.p(), ld, V.p(), ld, b, ldb, heads, dd, 1.0f, drop, 7, 8, yy, ld, ll, heads);
    };
    auto bwd = [&](hsmh_pattern* p, const float* b, uint64_t ldb, float drop, uint16_t* q_out, uint16_t* k_out, uint16_t* v_out, float* b_out, uint64_t ldgb) {
        return hsmhd16_backward_device(p, Q.p(), ld, K.p(), ld, V.p(), ld, G.p(), ld, lse.p(), heads, b, ldb, heads, d, 1.0f, drop, 7, 8, q_out, ld, k_out, ld, v_out, ld, b_out, ldgb);
    };
    auto good = [&](const std::string& after) {
        EXPECT(fwd(h, B.p(), heads, 0.5f, y.p(), lse.p()) == HS_OK, std::string("the object is unusable after ") + after);
        EXPECT(bwd(h, B.p(), heads, 0.5f, gq.p(), gk.p(), gv.p(), gb.p(), heads) == HS_OK, std::string("the object is unusable after ") + after);
        EXPECT(bwd(h, nullptr, 0, 0.5f, gq.p(), gk.p(), gv.p(), gb.p(), heads) == HS_OK, std::string("the object is unusable without a bias after ") + after);
    };
    good("nothing");
#define REFUSED(call, what)                                                              \
    do {                                                                                 \
        EXPECT((call) == HS_ERR_BAD_ARG && std::strlen(hsmh_last_error(h)), what);       \
        good(what);                                                                      \
    } while (0)
    for (float bad : bad_drops) {
        REFUSED(fwd(h, B.p(), heads, bad, y.p(), lse.p()), "forward: a bad drop_p");
        EXPECT(fwd(h, nullptr, 0, bad, y.p(), lse.p()) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(h), "drop_p"), "forward, bias NULL: a bad drop_p");
        EXPECT(bwd(h, B.p(), heads, bad, gq.p(), gk.p(), gv.p(), gb.p(), heads) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(h), "drop_p"), "backward: a bad drop_p");
        REFUSED(bwd(h, nullptr, 0, bad, gq.p(), gk.p(), gv.p(), nullptr, 0), "backward, bias NULL: a bad drop_p");
        REFUSED(hsmhd16_forward(h, Q.p(), K.p(), V.p(), B.p(), heads, d, 1.0f, bad, 7, 8, y.p(), lse.p()), "host form: a bad drop_p");
        REFUSED(hsmhd16_backward(h, Q.p(), K.p(), V.p(), G.p(), lse.p(), nullptr, heads, d, 1.0f, bad, 7, 8, gq.p(), gk.p(), gv.p(), gb.p()), "host form: a bad drop_p");
    }
    float* odd = reinterpret_cast<float*>(reinterpret_cast<char*>(B.p()) + 2);
    REFUSED(fwd(h, odd, heads, 0.5f, y.p(), lse.p()), "misaligned bias");
    REFUSED(fwd(h, B.p(), 1, 0.5f, y.p(), lse.p()), "ldb < heads");
    REFUSED(fwd(h, B.p(), heads, 0.5f, reinterpret_cast<uint16_t*>(B.p()), lse.p()), "y is bias");
    REFUSED(fwd(h, nullptr, 0, 0.5f, Q.p(), lse.p()), "y is q");
    REFUSED(fwd(h, B.p(), heads, 0.5f, y.p(), lse.p(), 4), "d = 4");
    REFUSED(fwd(h, B.p(), heads, 0.5f, y.p(), lse.p(), 8, 20), "ldq not a multiple of 8");
    REFUSED(fwd(h, B.p(), heads, 0.5f, y.p() + 4, lse.p()), "misaligned y");
    REFUSED(bwd(h, B.p(), 1, 0.5f, gq.p(), gk.p(), gv.p(), gb.p(), heads), "ldb < heads");
    REFUSED(bwd(h, nullptr, 0, 0.5f, gq.p(), gk.p(), gv.p(), gb.p(), 1), "ldgb < heads without a bias");
    REFUSED(bwd(h, B.p(), heads, 0.5f, reinterpret_cast<uint16_t*>(B.p()), gk.p(), gv.p(), gb.p(), heads), "gq is bias");
    for (void* other : {(void*)Q.p(), (void*)K.p(), (void*)V.p(), (void*)G.p(), (void*)lse.p(), (void*)gq.p(), (void*)gk.p(), (void*)gv.p()}) {
        REFUSED(bwd(h, B.p(), heads, 0.5f, gq.p(), gk.p(), gv.p(), static_cast<float*>(other), heads), "gbias over another operand");
        REFUSED(bwd(h, nullptr, 0, 0.5f, gq.p(), gk.p(), gv.p(), static_cast<float*>(other), heads), "gbias over another operand, bias NULL");
    }
    REFUSED(hsmhd16_backward(h, Q.p(), K.p(), V.p(), G.p(), lse.p(), B.p(), heads, d, 1.0f, 0.5f, 7, 8, gq.p(), gk.p(), gv.p(), B.p()), "host form: gbias is bias");
#undef REFUSED
    EXPECT(bwd(h, B.p(), heads, 0.5f, gq.p(), gk.p(), gv.p(), nullptr, 0) == HS_OK, "gbias NULL");
    // objects without the entry map: the forward runs, the backward is refused and names hsmhb_create, with a bias and without
    for (hsmh_pattern* p : {plain, no_flag}) {
        EXPECT(fwd(p, B.p(), heads, 0.5f, y.p(), lse.p()) == HS_OK && fwd(p, nullptr, 0, 0.5f, y.p(), lse.p()) == HS_OK, "forward on an object without the map");
        EXPECT(bwd(p, B.p(), heads, 0.5f, gq.p(), gk.p(), gv.p(), gb.p(), heads) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(p), "hsmhb_create"), "backward without the map");
        EXPECT(bwd(p, nullptr, 0, 0.5f, gq.p(), gk.p(), gv.p(), nullptr, 0) == HS_ERR_BAD_ARG && std::strstr(hsmh_last_error(p), "hsmhb_create"), "backward without the map, bias NULL");
        EXPECT(hsmhd16_backward(p, Q.p(), K.p(), V.p(), G.p(), lse.p(), B.p(), heads, d, 1.0f, 0.5f, 7, 8, gq.p(), gk.p(), gv.p(), gb.p()) == HS_ERR_BAD_ARG, "backward without the map, host form");
        EXPECT(fwd(p, B.p(), heads, 0.5f, y.p(), nullptr) == HS_OK, "forward after the refusal");
    }
    EXPECT(hsmh_destroy(h) == HS_OK && hsmh_destroy(plain) == HS_OK && hsmh_destroy(no_flag) == HS_OK, "destroy");
}

}  // namespace

int main() {
    edges();
    refusals();
    if (g_failures) {
        std::printf("%d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("HEADS16 DROPOUT CPU OK\n");
    return 0;
}
