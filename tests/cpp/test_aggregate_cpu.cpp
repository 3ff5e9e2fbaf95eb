// test_aggregate_cpu.cpp — the CPU twin of include/hisparse_aggregate.h (hisparse_amd/csrc/hsw_cpu.cpp) through its C boundary, as a
// program of its own: tests/test_aggregate_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge
// patterns and the refusals of the header; buffers are exactly as large as the contract says, so a read or write past them is the
// sanitizer's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_aggregate.h"
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
// a few distinct values only, so that ties are common
float next_float() { return float(int(next_word() % 9) - 4) * 0.5f; }

// n words, 16-byte aligned, that end at most three words before the end of their allocation (n = 0: never touched by a correct callee)
template <class T>
struct Words {
    std::vector<T> raw;
    T* base;
    size_t n;
    explicit Words(size_t count, T fill = T()) : raw((count ? count : 1) + 4, fill), n(count) {
        uintptr_t p = reinterpret_cast<uintptr_t>(raw.data() + 4);
        base = reinterpret_cast<T*>(p - p % 16);
    }
    T* p() { return base; }
    T& operator[](size_t i) { return base[i]; }
};
using Floats = Words<float>;
using Args = Words<uint32_t>;

struct Pattern {
    std::string name;
    uint32_t rows, cols;
    std::vector<uint32_t> indptr, indices;
    uint64_t nnz() const { return indptr.back(); }
};

Pattern from_lengths(const std::string& name, uint32_t cols, const std::vector<uint32_t>& lengths, bool sorted) {
    Pattern p{name, uint32_t(lengths.size()), cols, {0}, {}};
    for (uint32_t n : lengths) {
        for (uint32_t k = 0; k < n; ++k) p.indices.push_back(sorted ? uint32_t(uint64_t(k) * cols / n) : next_word() % cols);
        p.indptr.push_back(uint32_t(p.indices.size()));
    }
    return p;
}

uint32_t bits(float v) {
    uint32_t w;
    std::memcpy(&w, &v, 4);
    return w;
}

const double kU = std::ldexp(1.0, -24);

// |got - E| <= u |E| + (n + 16) 2^-52 A + 2^-149 for the sum of `terms` over `over` (long double sums stand for E)
void check_sum(float got, const std::vector<double>& terms, double over, const std::string& what) {
    long double E = 0, A = 0;
    for (double t : terms) E += t, A += std::fabs((long double)t);
    E /= over, A /= over;
    const long double bound = kU * std::fabs(E) + (long double)(terms.size() + 16) * std::ldexp(1.0L, -52) * A + std::ldexp(1.0L, -149);
    EXPECT(std::fabs((long double)got - E) <= bound, what);
    if (terms.empty()) EXPECT(bits(got) == 0, what + ": nothing summed is +0.0");
}

// the header's rule over the entries of row r at feature j, as a walk that keeps the first of equals
uint32_t winner(const Pattern& pt, uint32_t r, const float* x, uint64_t ld, uint32_t j, bool max) {
    uint32_t best = HSAGG_NONE;
    for (uint32_t e = pt.indptr[r]; e < pt.indptr[r + 1]; ++e) {
        if (best == HSAGG_NONE) {
            best = e;
            continue;
        }
        const float v = x[pt.indices[e] * ld + j], b = x[pt.indices[best] * ld + j];
        const bool better = std::isnan(v) != std::isnan(b) ? std::isnan(v) : !std::isnan(v) && (max ? v > b : v < b);
        if (better) best = e;
    }
    return best;
}

void check_pattern(const Pattern& pt, uint32_t d, uint32_t pad, uint32_t ops, bool poison) {
    const std::string what = pt.name + ", d " + std::to_string(d) + ", pad " + std::to_string(pad) + ", ops " + std::to_string(ops) + (poison ? ", NaN and -0.0 among the words" : "");
    hsw_pattern* h = nullptr;
    EXPECT(hsw_create(&h, 0, pt.rows, pt.cols, pt.indptr.data(), pt.nnz() ? pt.indices.data() : nullptr, HSW_TRANSPOSED) == HS_OK && h, what);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsw_info(h, &nnz, &bytes) == HS_OK && nnz == pt.nnz() && bytes == 0, what);
    const uint64_t ld = (d + 3) / 4 * 4 + pad;
    const float nan = std::numeric_limits<float>::quiet_NaN(), mark = -7.0f;
    const uint32_t amark = 0xABCDEF01u;
    const bool sum = ops & (HSAGG_SUM | HSAGG_MEAN), mean = ops & HSAGG_MEAN, max = ops & HSAGG_MAX, min = ops & HSAGG_MIN;
    Floats X(pt.cols * ld, nan), ysum(sum ? pt.rows * ld : 0, mark), ymax(max ? pt.rows * ld : 0, mark), ymin(min ? pt.rows * ld : 0, mark);
    Args amax(max ? pt.rows * ld : 0, amark), amin(min ? pt.rows * ld : 0, amark);
    for (uint32_t c = 0; c < pt.cols; ++c)
        for (uint32_t j = 0; j < d; ++j) X[c * ld + j] = poison && next_word() % 7 == 0 ? (next_word() % 2 ? nan : -0.0f) : next_float();
    EXPECT(hsagg_forward_device(h, ops, X.p(), ld, d, sum ? ysum.p() : nullptr, max ? ymax.p() : nullptr, max ? amax.p() : nullptr, min ? ymin.p() : nullptr, min ? amin.p() : nullptr,
                                ld) == HS_OK, what);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const uint32_t n = pt.indptr[r + 1] - pt.indptr[r];
        for (uint32_t j = 0; j < d; ++j) {
            const uint64_t at = r * ld + j;
            if (sum) {
                std::vector<double> terms;
                bool finite = true;
                for (uint32_t e = pt.indptr[r]; e < pt.indptr[r + 1]; ++e) {
                    terms.push_back(X[pt.indices[e] * ld + j]);
                    finite = finite && std::isfinite(terms.back());
                }
                if (finite) check_sum(ysum[at], terms, mean && n ? double(n) : 1.0, what + ", sum of row " + std::to_string(r));
                else EXPECT(std::isnan(ysum[at]), what + ", a NaN term");
            }
            for (int side = 0; side < 2; ++side) {
                if (!(side ? min : max)) continue;
                const uint32_t e = winner(pt, r, X.p(), ld, j, side == 0);
                const float got = side ? ymin[at] : ymax[at];
                EXPECT((side ? amin[at] : amax[at]) == e, what + ", arg of row " + std::to_string(r));
                EXPECT(bits(got) == (e == HSAGG_NONE ? 0u : bits(X[pt.indices[e] * ld + j])), what + ", extreme of row " + std::to_string(r));
            }
        }
        for (uint64_t j = d; j < ld; ++j) {
            if (sum) EXPECT(ysum[r * ld + j] == mark, what + ", ysum's pad word written");
            if (max) EXPECT(ymax[r * ld + j] == mark && amax[r * ld + j] == amark, what + ", ymax's or amax's pad word written");
            if (min) EXPECT(ymin[r * ld + j] == mark && amin[r * ld + j] == amark, what + ", ymin's or amin's pad word written");
        }
    }
    // the backward with the args just written; the gradients' pad words are NaN
    Floats gsum(sum ? pt.rows * ld : 0, nan), gmax(max ? pt.rows * ld : 0, nan), gmin(min ? pt.rows * ld : 0, nan), gx(pt.cols * ld, mark);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t j = 0; j < d; ++j) {
            if (sum) gsum[r * ld + j] = next_float() + 0.25f;
            if (max) gmax[r * ld + j] = next_float() + 0.25f;
            if (min) gmin[r * ld + j] = next_float() + 0.25f;
        }
    EXPECT(hsagg_backward_device(h, ops, sum ? gsum.p() : nullptr, max ? gmax.p() : nullptr, max ? amax.p() : nullptr, min ? gmin.p() : nullptr, min ? amin.p() : nullptr, ld, d, gx.p(),
                                 ld) == HS_OK, what);
    std::vector<std::vector<double>> terms(size_t(pt.cols) * d);
    for (uint32_t r = 0; r < pt.rows; ++r)
        for (uint32_t e = pt.indptr[r]; e < pt.indptr[r + 1]; ++e)
            for (uint32_t j = 0; j < d; ++j) {
                std::vector<double>& t = terms[size_t(pt.indices[e]) * d + j];
                const uint64_t at = r * ld + j;
                if (sum) t.push_back(mean ? double(gsum[at]) / double(pt.indptr[r + 1] - pt.indptr[r]) : double(gsum[at]));
                if (max && amax[at] == e) t.push_back(gmax[at]);
                if (min && amin[at] == e) t.push_back(gmin[at]);
            }
    for (uint32_t c = 0; c < pt.cols; ++c) {
        for (uint32_t j = 0; j < d; ++j) check_sum(gx[c * ld + j], terms[size_t(c) * d + j], 1.0, what + ", gx of column " + std::to_string(c));
        for (uint64_t j = d; j < ld; ++j) EXPECT(gx[c * ld + j] == mark, what + ", gx's pad word written");
    }
    // the host forms (ld = d) give the words of the device forms
    Floats hx(size_t(pt.cols) * d), hsum(sum ? size_t(pt.rows) * d : 0, mark), hmax(max ? size_t(pt.rows) * d : 0, mark), hmin(min ? size_t(pt.rows) * d : 0, mark);
    Args hamax(max ? size_t(pt.rows) * d : 0, amark), hamin(min ? size_t(pt.rows) * d : 0, amark);
    for (uint32_t c = 0; c < pt.cols; ++c) std::memcpy(&hx[size_t(c) * d], &X[c * ld], d * 4);
    EXPECT(hsagg_forward(h, ops, hx.p(), d, sum ? hsum.p() : nullptr, max ? hmax.p() : nullptr, max ? hamax.p() : nullptr, min ? hmin.p() : nullptr, min ? hamin.p() : nullptr) == HS_OK, what);
    Floats hgs(sum ? size_t(pt.rows) * d : 0), hgt(max ? size_t(pt.rows) * d : 0), hgb(min ? size_t(pt.rows) * d : 0), hgx(size_t(pt.cols) * d, mark);
    for (uint32_t r = 0; r < pt.rows; ++r) {
        const size_t to = size_t(r) * d, from = r * ld;
        if (sum) {
            EXPECT(std::memcmp(&hsum[to], &ysum[from], d * 4) == 0, what + ": hsagg_forward's sum differs");
            std::memcpy(&hgs[to], &gsum[from], d * 4);
        }
        if (max) {
            EXPECT(std::memcmp(&hmax[to], &ymax[from], d * 4) == 0 && std::memcmp(&hamax[to], &amax[from], d * 4) == 0, what + ": hsagg_forward's max differs");
            std::memcpy(&hgt[to], &gmax[from], d * 4);
        }
        if (min) {
            EXPECT(std::memcmp(&hmin[to], &ymin[from], d * 4) == 0 && std::memcmp(&hamin[to], &amin[from], d * 4) == 0, what + ": hsagg_forward's min differs");
            std::memcpy(&hgb[to], &gmin[from], d * 4);
        }
    }
    EXPECT(hsagg_backward(h, ops, sum ? hgs.p() : nullptr, max ? hgt.p() : nullptr, max ? hamax.p() : nullptr, min ? hgb.p() : nullptr, min ? hamin.p() : nullptr, d, hgx.p()) == HS_OK, what);
    for (uint32_t c = 0; c < pt.cols; ++c) EXPECT(std::memcmp(&hgx[size_t(c) * d], &gx[c * ld], d * 4) == 0, what + ": hsagg_backward differs");
    // the arg arrays may be left out
    if (max || min) EXPECT(hsagg_forward_device(h, ops, X.p(), ld, d, sum ? ysum.p() : nullptr, max ? ymax.p() : nullptr, nullptr, min ? ymin.p() : nullptr, nullptr, ld) == HS_OK, what);
    uint64_t nnz2 = 0, bytes2 = 1;
    EXPECT(hsw_info(h, &nnz2, &bytes2) == HS_OK && nnz2 == nnz && bytes2 == 0, what + ": hsw_info changed");
    EXPECT(hsw_destroy(h) == HS_OK, what);
}

void refusals() {
    const std::vector<uint32_t> ip = {0, 3, 3, 8, 9}, ix = {0, 2, 4, 1, 1, 2, 3, 4, 0};
    Floats one(4);
    EXPECT(hsagg_forward_device(nullptr, HSAGG_SUM, one.p(), 4, 1, one.p(), nullptr, nullptr, nullptr, nullptr, 4) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsagg_backward_device(nullptr, HSAGG_SUM, one.p(), nullptr, nullptr, nullptr, nullptr, 4, 1, one.p(), 4) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsagg_forward(nullptr, HSAGG_SUM, one.p(), 1, one.p(), nullptr, nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsagg_backward(nullptr, HSAGG_SUM, one.p(), nullptr, nullptr, nullptr, nullptr, 1, one.p()) == HS_ERR_BAD_ARG, "null object");

    hsw_pattern *h = nullptr, *plain = nullptr;
    EXPECT(hsw_create(&h, 0, 4, 5, ip.data(), ix.data(), HSW_TRANSPOSED) == HS_OK && h, "create");
    EXPECT(hsw_create(&plain, 0, 4, 5, ip.data(), ix.data(), 0) == HS_OK && plain, "create without the flag");
    if (!h || !plain) return;
    const uint32_t d = 5, all = HSAGG_MEAN | HSAGG_MAX | HSAGG_MIN;
    const uint64_t ld = 8;
    Floats x(5 * ld), ysum(5 * ld), ymax(5 * ld), ymin(5 * ld), gx(5 * ld), want(4 * ld), got(4 * ld);
    Args amax(5 * ld), amin(5 * ld);
    for (size_t i = 0; i < 5 * ld; ++i) x[i] = next_float();
    EXPECT(hsagg_forward_device(h, HSAGG_SUM, x.p(), ld, d, want.p(), nullptr, nullptr, nullptr, nullptr, ld) == HS_OK, "reference call");
    auto still_usable = [&](int rc, const char* what, int code = HS_ERR_BAD_ARG, hsw_pattern* obj = nullptr) {
        obj = obj ? obj : h;
        EXPECT(rc == code && std::strlen(hsw_last_error(obj)) > 0, what);
        EXPECT(hsagg_forward_device(obj, HSAGG_SUM, x.p(), ld, d, got.p(), nullptr, nullptr, nullptr, nullptr, ld) == HS_OK && std::memcmp(got.p(), want.p(), 4 * ld * 4) == 0, what);
    };
    auto fwd = [&](uint32_t ops, const float* xx, uint64_t ldx, uint32_t dd, float* s, float* t, uint32_t* at, float* b, uint32_t* ab, uint64_t ldy) {
        return hsagg_forward_device(h, ops, xx, ldx, dd, s, t, at, b, ab, ldy);
    };
    EXPECT(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld) == HS_OK, "the full forward");
    still_usable(fwd(0, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "ops = 0");
    still_usable(fwd(16, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "ops = 16");
    still_usable(fwd(HSAGG_MAX | 0x80000000u, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "an unknown bit beside a known one");
    still_usable(fwd(HSAGG_SUM | HSAGG_MEAN, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "SUM | MEAN");
    still_usable(fwd(all, x.p(), ld, 0, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "d = 0");
    still_usable(fwd(all, x.p(), 260, 257, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), 260), "d = 257");
    still_usable(fwd(all, nullptr, ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "null x");
    still_usable(fwd(all, x.p(), ld, d, nullptr, ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "null ysum");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), nullptr, amax.p(), ymin.p(), amin.p(), ld), "null ymax");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), nullptr, amin.p(), ld), "null ymin");
    still_usable(fwd(all, x.p() + 1, ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "misaligned x");
    still_usable(fwd(all, x.p(), ld, d, ysum.p() + 2, ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "misaligned ysum");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), amax.p() + 1, ymin.p(), amin.p(), ld), "misaligned amax");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p() + 3, amin.p(), ld), "misaligned ymin");
    still_usable(fwd(all, x.p(), 6, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "ldx % 4");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), 4), "ldy < d");
    still_usable(fwd(all, x.p(), ld, d, x.p(), ymax.p(), amax.p(), ymin.p(), amin.p(), ld), "ysum is x");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ysum.p(), amax.p(), ymin.p(), amin.p(), ld), "ymax is ysum");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amax.p() + 4, ld), "amin inside amax");
    still_usable(fwd(all, x.p(), ld, d, ysum.p(), ymax.p(), reinterpret_cast<uint32_t*>(ymin.p()), ymin.p(), amin.p(), ld), "amax is ymin");
    EXPECT(fwd(HSAGG_SUM, x.p(), ld, d, ysum.p(), nullptr, amax.p() + 1, x.p(), nullptr, ld) == HS_OK, "outputs whose bit is not set are not looked at");

    Floats gs(4 * ld, 1.0f), gt(4 * ld, 1.0f), gb(4 * ld, 1.0f);
    auto bwd = [&](hsw_pattern* obj, uint32_t ops, const float* s, const float* t, const uint32_t* at, const float* b, const uint32_t* ab, uint64_t ldg, uint32_t dd, float* out,
                   uint64_t ldgx) { return hsagg_backward_device(obj, ops, s, t, at, b, ab, ldg, dd, out, ldgx); };
    EXPECT(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld) == HS_OK, "the full backward");
    still_usable(bwd(h, 0, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld), "backward ops = 0");
    still_usable(bwd(h, HSAGG_SUM | HSAGG_MEAN | HSAGG_MIN, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld), "backward SUM | MEAN");
    still_usable(bwd(h, all, nullptr, gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld), "null gsum");
    still_usable(bwd(h, all, gs.p(), nullptr, amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld), "null gmax");
    still_usable(bwd(h, all, gs.p(), gt.p(), nullptr, gb.p(), amin.p(), ld, d, gx.p(), ld), "null amax");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), nullptr, ld, d, gx.p(), ld), "null amin");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, nullptr, ld), "null gx");
    still_usable(bwd(h, all, gs.p(), gt.p() + 1, amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld), "misaligned gmax");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p() + 2, ld, d, gx.p(), ld), "misaligned amin");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), 7, d, gx.p(), ld), "ldg % 4");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gx.p(), 4), "ldgx < d");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gs.p(), ld), "gx is gsum");
    still_usable(bwd(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, reinterpret_cast<float*>(amax.p()), ld), "gx is amax");
    still_usable(bwd(plain, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), ld, d, gx.p(), ld), "backward_device without the flag", HS_ERR_UNSUPPORTED, plain);
    // the host forms
    still_usable(hsagg_forward(h, all, nullptr, d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p()), "host null x");
    still_usable(hsagg_forward(h, all, x.p(), d, ysum.p(), ymax.p(), amax.p(), nullptr, amin.p()), "host null ymin");
    still_usable(hsagg_forward(h, 3, x.p(), d, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p()), "host SUM | MEAN");
    still_usable(hsagg_forward(h, all, x.p(), 257, ysum.p(), ymax.p(), amax.p(), ymin.p(), amin.p()), "host d = 257");
    still_usable(hsagg_forward(h, all, x.p(), d, x.p(), ymax.p(), amax.p(), ymin.p(), amin.p()), "host ysum is x");
    still_usable(hsagg_forward(h, all, x.p(), d, ysum.p(), ymax.p(), amax.p(), ymax.p() + 4, amin.p()), "host ymin inside ymax");
    still_usable(hsagg_backward(h, all, gs.p(), gt.p(), nullptr, gb.p(), amin.p(), d, gx.p()), "host null amax");
    still_usable(hsagg_backward(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), 0, gx.p()), "host backward d = 0");
    still_usable(hsagg_backward(h, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), d, gb.p()), "host gx is gmin");
    still_usable(hsagg_backward(plain, all, gs.p(), gt.p(), amax.p(), gb.p(), amin.p(), d, gx.p()), "backward without the flag", HS_ERR_UNSUPPORTED, plain);
    EXPECT(hsagg_forward(h, all, x.p(), d, ysum.p(), ymax.p(), nullptr, ymin.p(), nullptr) == HS_OK, "host form without args");
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
    const uint32_t masks[] = {HSAGG_SUM, HSAGG_MEAN, HSAGG_MAX, HSAGG_MIN, HSAGG_SUM | HSAGG_MAX | HSAGG_MIN, HSAGG_MEAN | HSAGG_MAX | HSAGG_MIN};
    for (const Pattern& p : patterns)
        for (uint32_t d : {1u, 5u, 64u})
            for (uint32_t pad : {0u, 8u})
                for (uint32_t ops : masks) check_pattern(p, d, pad, ops, pad == 8 && (ops & (HSAGG_MAX | HSAGG_MIN)));
    refusals();
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("AGGREGATE CPU OK\n");
    return 0;
}
