// test_gatv2_cpu.cpp — the CPU twin of include/hisparse_gatv2.h (hisparse_amd/csrc/hsmh_cpu.cpp) through its C boundary, as a program of
// its own: tests/test_gatv2_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  Edge patterns and
// a few refusals; every buffer is a heap block of exactly the contract's reach (a feature operand ends with its last row's word
// heads * d - 1, lse with head `heads - 1` of its last row, a and ga hold heads * d words, the workspace hsgat2_work_bytes bytes), so a read
// or write past one is the sanitizer's.  Values are checked against long double loops per head with a tolerance far above the contract's
// bound and far below any mistake of indexing (the bound itself is tests/gatv2_cases.py's business).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_gatv2.h"
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

// exactly n floats in a heap block of their own, 16-byte aligned (malloc's alignment)
struct Floats {
    float* base;
    size_t n;
    explicit Floats(size_t count, float fill = 0.0f) : base(static_cast<float*>(std::malloc((count ? count : 1) * sizeof(float)))), n(count) {
        for (size_t i = 0; i < (count ? count : 1); ++i) base[i] = fill;
    }
    Floats(const Floats&) = delete;
    ~Floats() { std::free(base); }
    float* p() { return base; }
    float& operator[](size_t i) { return base[i]; }
};

struct Pattern {
    std::string name;
    uint32_t rows, cols;
    std::vector<uint32_t> indptr, indices;
    uint64_t nnz() const { return indptr.back(); }
};

Pattern from_lengths(const std::string& name, uint32_t cols, const std::vector<uint32_t>& lengths) {
    Pattern p{name, uint32_t(lengths.size()), cols, {0}, {}};
    for (uint32_t n : lengths) {
        for (uint32_t k = 0; k < n; ++k) p.indices.push_back(next_word() % cols);
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
    const uint64_t ld = w + pad, ldl = heads + extra;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f, ninf = -std::numeric_limits<float>::infinity();
    auto reach = [&](uint64_t n) { return n ? (n - 1) * ld + w : 0; };
    auto reach_l = [&](uint64_t n) { return n ? (n - 1) * ldl + heads : 0; };
    Floats XD(reach(pt.rows), nan), XS(reach(pt.cols), nan), G(reach(pt.rows), nan), A(w);
    Floats y(reach(pt.rows), mark), lse(reach_l(pt.rows), mark), gxd(reach(pt.rows), mark), gxs(reach(pt.cols), mark), ga(w, mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < w; ++j) XD[r * ld + j] = next_float(2.0f), G[r * ld + j] = next_float(1.5f);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < w; ++j) XS[c * ld + j] = next_float(2.0f);
    for (uint32_t j = 0; j < w; ++j) A[j] = next_float(1.0f);
    uint64_t work_bytes = 0;
    EXPECT(hsgat2_work_bytes(h, heads, d, &work_bytes) == HS_OK && work_bytes == uint64_t(w) * 8, what);
    void* work = std::malloc(work_bytes);
    EXPECT(hsgat2_forward_device(h, XD.p(), ld, XS.p(), ld, A.p(), heads, d, slope, y.p(), ld, lse.p(), ldl) == HS_OK, what + ": " + hsmh_last_error(h));
    EXPECT(hsgat2_backward_device(h, XD.p(), ld, XS.p(), ld, A.p(), G.p(), ld, lse.p(), ldl, heads, d, slope, gxd.p(), ld, gxs.p(), ld, ga.p(), work, work_bytes) == HS_OK,
           what + ": " + hsmh_last_error(h));
    std::vector<uint32_t> count(pt.cols, 0);
    for (uint32_t c : pt.indices) ++count[c];
    for (uint32_t hd = 0; hd < heads; ++hd) {
        const uint32_t at = hd * d;
        std::vector<long double> want_s(size_t(pt.cols) * d, 0.0L), want_a(d, 0.0L);
        for (uint32_t r = 0; r < pt.rows; ++r) {
            const uint32_t lo = pt.indptr[r], hi = pt.indptr[r + 1];
            if (lo == hi) {
                for (uint32_t j = 0; j < d; ++j) EXPECT(plus_zero(y[r * ld + at + j]) && plus_zero(gxd[r * ld + at + j]), what + ": an empty row");
                EXPECT(lse[r * ldl + hd] == ninf, what + ": lse of an empty row");
                continue;
            }
            std::vector<long double> t(hi - lo), p(hi - lo), gp(hi - lo);
            long double m = -INFINITY, l = 0.0L, dsum = 0.0L;
            for (uint32_t e = lo; e < hi; ++e) {
                long double s = 0.0L;
                for (uint32_t j = 0; j < d; ++j) {
                    const long double z = (long double)XD[r * ld + at + j] + XS[pt.indices[e] * ld + at + j];
                    s += (long double)A[at + j] * (z > 0 ? z : slope * z);
                }
                t[e - lo] = s;
                m = std::fmax(m, s);
            }
            for (uint32_t e = lo; e < hi; ++e) l += std::exp(t[e - lo] - m);
            EXPECT(close_to(lse[r * ldl + hd], m + std::log(l)), what + ": lse");
            for (uint32_t e = lo; e < hi; ++e) {
                p[e - lo] = std::exp(t[e - lo] - m) / l;
                long double s = 0.0L;
                for (uint32_t j = 0; j < d; ++j) s += (long double)G[r * ld + at + j] * XS[pt.indices[e] * ld + at + j];
                gp[e - lo] = s;
                dsum += p[e - lo] * s;
            }
            for (uint32_t j = 0; j < d; ++j) {
                long double yy = 0.0L, gd = 0.0L;
                for (uint32_t e = lo; e < hi; ++e) {
                    const uint32_t c = pt.indices[e];
                    const long double z = (long double)XD[r * ld + at + j] + XS[c * ld + at + j], dz = z > 0 ? 1.0L : slope, gt = p[e - lo] * (gp[e - lo] - dsum);
                    yy += p[e - lo] * XS[c * ld + at + j];
                    gd += gt * A[at + j] * dz;
                    want_s[size_t(c) * d + j] += p[e - lo] * G[r * ld + at + j] + gt * A[at + j] * dz;
                    want_a[j] += gt * (z > 0 ? z : slope * z);
                }
                EXPECT(close_to(y[r * ld + at + j], yy), what + ": y");
                EXPECT(close_to(gxd[r * ld + at + j], gd), what + ": gxd");
            }
        }
        for (uint32_t c = 0; c < pt.cols; ++c)
            for (uint32_t j = 0; j < d; ++j)
                EXPECT(count[c] ? close_to(gxs[c * ld + at + j], want_s[size_t(c) * d + j]) : plus_zero(gxs[c * ld + at + j]), what + ": gxs");
        for (uint32_t j = 0; j < d; ++j) EXPECT(pt.nnz() ? close_to(ga[at + j], want_a[j]) : plus_zero(ga[at + j]), what + ": ga");
    }
    for (uint32_t r = 0; r + 1 < pt.rows; ++r) {      // the pad words between two rows were not written
        for (uint64_t j = w; j < ld; ++j) EXPECT(y[r * ld + j] == mark && gxd[r * ld + j] == mark, what + ": pad words of a row");
        for (uint64_t j = heads; j < ldl; ++j) EXPECT(lse[r * ldl + j] == mark, what + ": pad words of lse");
    }
    // refusals leave the object usable: a workspace one byte short, a misaligned one, ga laid over it, a bad slope, a bad shape
    EXPECT(hsgat2_backward_device(h, XD.p(), ld, XS.p(), ld, A.p(), G.p(), ld, lse.p(), ldl, heads, d, slope, gxd.p(), ld, gxs.p(), ld, ga.p(), work, work_bytes - 1) == HS_ERR_BAD_ARG, what);
    EXPECT(hsgat2_backward_device(h, XD.p(), ld, XS.p(), ld, A.p(), G.p(), ld, lse.p(), ldl, heads, d, slope, gxd.p(), ld, gxs.p(), ld, ga.p(), static_cast<char*>(work) + 8, work_bytes) ==
               HS_ERR_BAD_ARG, what);
    EXPECT(hsgat2_backward_device(h, XD.p(), ld, XS.p(), ld, A.p(), G.p(), ld, lse.p(), ldl, heads, d, slope, gxd.p(), ld, gxs.p(), ld, static_cast<float*>(work), work, work_bytes) ==
               HS_ERR_BAD_ARG, what);
    EXPECT(hsgat2_forward_device(h, XD.p(), ld, XS.p(), ld, A.p(), heads, d, -1.0f, y.p(), ld, nullptr, 0) == HS_ERR_BAD_ARG, what);
    EXPECT(hsgat2_forward_device(h, XD.p(), ld, XS.p(), ld, A.p(), heads, d + 1, slope, y.p(), ld, nullptr, 0) == HS_ERR_BAD_ARG, what);
    EXPECT(hsgat2_forward_device(h, XD.p(), ld, XS.p(), ld, A.p(), heads, d, slope, y.p(), ld, nullptr, 0) == HS_OK, what + ": lse NULL after the refusals");
    std::free(work);
    hsmh_destroy(h);
}

}  // namespace

int main() {
    std::vector<Pattern> patterns;
    patterns.push_back(from_lengths("nnz = 0", 7, {0, 0, 0, 0, 0}));
    patterns.push_back(from_lengths("one entry", 9, {0, 0, 1, 0}));
    patterns.push_back(from_lengths("one row", 9, {5}));
    patterns.push_back(from_lengths("one column", 1, {1, 0, 1, 1, 0, 0, 1}));
    patterns.push_back(from_lengths("empty rows at the start, in runs and at the end", 11, {0, 0, 3, 1, 0, 0, 0, 6, 0, 2, 0, 0}));
    patterns.push_back(from_lengths("one row holds every entry", 301, {0, 0, 301, 0}));
    patterns.push_back(from_lengths("pairs held twice", 3, {4, 5, 1}));
    for (const Pattern& pt : patterns) {
        check_pattern(pt, 3, 8, 0, 0, 0.2f);
        check_pattern(pt, 5, 4, 8, 3, 0.0f);
        check_pattern(pt, 1, 4, 4, 1, 1.0f);
    }
    check_pattern(patterns[4], 2, 128, 0, 0, 0.2f);
    check_pattern(patterns[4], 64, 4, 0, 0, 0.2f);
    if (g_failures) {
        std::printf("%d failures\n", g_failures);
        return 1;
    }
    std::printf("GATV2 CPU OK\n");
    return 0;
}
