// test_rows_cpu.cpp — the CPU twin of include/hisparse_rows.h (hisparse_amd/csrc/hsr_cpu.cpp) through its C boundary, as a program of its
// own: tests/test_rows_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edges and the refusals of
// the header; buffers are exactly as large as the contract says, so a read or write past them is the sanitizer's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "hisparse_hip.h"
#include "hisparse_rows.h"

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
float next_float(float magnitude) {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return (float(uint32_t(g_seed >> 40)) / float(1 << 24) - 0.5f) * 2.0f * magnitude;
}

std::vector<uint32_t> indptr_of(const std::vector<uint32_t>& lengths) {
    std::vector<uint32_t> ip = {0};
    for (uint32_t n : lengths) ip.push_back(ip.back() + n);
    return ip;
}

// exactly n floats on the heap (n = 0: one, never touched by a correct callee -- the sentinel says so)
struct Floats {
    std::vector<float> v;
    explicit Floats(size_t n, float fill = 0.0f) : v(n ? n : 1, n ? fill : 12345.0f) {}
    float* p() { return v.data(); }
};

void check_forward(const std::vector<uint32_t>& ip, const float* s, float scale, const float* p, const std::string& what) {
    for (size_t i = 0; i + 1 < ip.size(); ++i) {
        const size_t lo = ip[i], n = ip[i + 1] - lo;
        if (!n) continue;
        float m = -INFINITY;
        for (size_t k = 0; k < n; ++k) {
            volatile float t = scale * s[lo + k];
            m = std::fmax(m, t);
        }
        std::vector<double> E(n);
        long double sum = 0;
        for (size_t k = 0; k < n; ++k) {
            volatile float t = scale * s[lo + k];
            volatile float d = t - m;
            E[k] = std::exp(double(d));
            sum += E[k];
        }
        for (size_t k = 0; k < n; ++k) {
            const double P = double(E[k] / sum);
            EXPECT(std::fabs(double(p[lo + k]) - P) <= 3.0 * std::ldexp(P, -23) + std::ldexp(1.0, -125), what + ", row " + std::to_string(i) + ", entry " + std::to_string(k));
        }
        if (n == 1) EXPECT(p[lo] == 1.0f, what + ", a row of one entry");
    }
}

void check_backward(const std::vector<uint32_t>& ip, const float* p, const float* gp, float scale, const float* gs, const std::string& what) {
    for (size_t i = 0; i + 1 < ip.size(); ++i) {
        const size_t lo = ip[i], n = ip[i + 1] - lo;
        long double D = 0, A = 0;
        for (size_t k = 0; k < n; ++k) {
            D += (long double)p[lo + k] * gp[lo + k];
            A += std::fabs((long double)p[lo + k] * gp[lo + k]);
        }
        for (size_t k = 0; k < n; ++k) {
            const long double G = (long double)scale * p[lo + k] * ((long double)gp[lo + k] - D);
            const long double bound = std::ldexp(std::fabs(G), -23) + std::fabs((long double)scale) * p[lo + k] * (n + 4) * std::ldexp(1.0L, -52) * (A + std::fabs((long double)gp[lo + k])) +
                                      std::ldexp(1.0L, -149);
            EXPECT(std::fabs((long double)gs[lo + k] - G) <= bound, what + ", row " + std::to_string(i) + ", entry " + std::to_string(k));
        }
    }
}

void check_edge(const std::string& name, const std::vector<uint32_t>& lengths) {
    const std::vector<uint32_t> ip = indptr_of(lengths);
    hsr_rows* h = nullptr;
    EXPECT(hsr_create(&h, 0, uint32_t(lengths.size()), ip.data()) == HS_OK && h, name);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsr_info(h, &nnz, &bytes) == HS_OK && nnz == ip.back() && bytes == 0, name);
    EXPECT(hsr_info(h, nullptr, nullptr) == HS_OK, name);
    for (float scale : {1.0f, 0.125f, -2.5f}) {
        const std::string what = name + ", scale " + std::to_string(scale);
        Floats s(nnz), p(nnz, -7.0f), inplace(nnz), gp(nnz), gs(nnz, -7.0f), ginplace(nnz), hp(nnz), hgs(nnz);
        for (size_t e = 0; e < nnz; ++e) {
            inplace.v[e] = s.v[e] = next_float(30.0f);
            ginplace.v[e] = gp.v[e] = next_float(3.0f);
        }
        EXPECT(hsr_softmax_device(h, s.p(), scale, p.p()) == HS_OK, what);
        EXPECT(hsr_softmax_device(h, inplace.p(), scale, inplace.p()) == HS_OK, what + ", in place");
        EXPECT(hsr_softmax(h, s.p(), scale, hp.p()) == HS_OK, what + ", host form");
        EXPECT(hsr_softmax_backward_device(h, p.p(), gp.p(), scale, gs.p()) == HS_OK, what);
        EXPECT(hsr_softmax_backward_device(h, p.p(), ginplace.p(), scale, ginplace.p()) == HS_OK, what + ", in place");
        EXPECT(hsr_softmax_backward(h, p.p(), gp.p(), scale, hgs.p()) == HS_OK, what + ", host form");
        EXPECT(hsr_sync(h) == HS_OK && hsr_set_stream(h, nullptr) == HS_OK, what);
        if (nnz == 0) {
            for (Floats* f : {&s, &p, &inplace, &gp, &gs, &ginplace, &hp, &hgs}) EXPECT(f->v[0] == 12345.0f, what + ": a call on an empty pattern wrote");
            continue;
        }
        check_forward(ip, s.p(), scale, p.p(), what);
        check_backward(ip, p.p(), gp.p(), scale, gs.p(), what);
        EXPECT(std::memcmp(p.p(), inplace.p(), nnz * 4) == 0 && std::memcmp(p.p(), hp.p(), nnz * 4) == 0, what + ": the three forward forms differ");
        EXPECT(std::memcmp(gs.p(), ginplace.p(), nnz * 4) == 0 && std::memcmp(gs.p(), hgs.p(), nnz * 4) == 0, what + ": the three backward forms differ");
    }
    // exact answers: scale = 0 is float(1.0 / n); non-finite rows are NaN in every entry and nowhere else
    if (nnz) {
        Floats s(nnz), p(nnz);
        for (size_t e = 0; e < nnz; ++e) s.v[e] = next_float(300.0f);
        EXPECT(hsr_softmax_device(h, s.p(), 0.0f, p.p()) == HS_OK, name);
        for (size_t i = 0; i + 1 < ip.size(); ++i)
            for (size_t e = ip[i]; e < ip[i + 1]; ++e) EXPECT(p.v[e] == float(1.0 / double(ip[i + 1] - ip[i])), name + ", scale 0");
        s.v[nnz - 1] = std::numeric_limits<float>::quiet_NaN();
        EXPECT(hsr_softmax_device(h, s.p(), 1.0f, p.p()) == HS_OK, name);
        size_t its_row = ip.size() - 2;      // the last non-empty row
        while (ip[its_row] == ip[its_row + 1]) --its_row;
        for (size_t e = 0; e < nnz; ++e) EXPECT(std::isnan(p.v[e]) == (e >= ip[its_row]), name + ", a NaN in the last entry");
    }
    EXPECT(hsr_destroy(h) == HS_OK, name);
}

void refusals() {
    const std::vector<uint32_t> ip = {0, 3, 3, 8, 9};
    std::vector<uint32_t> bad;
    hsr_rows* h = reinterpret_cast<hsr_rows*>(16);
    auto refused = [&](int rc, int code, const char* what) {
        EXPECT(rc == code && h == nullptr && std::strlen(hsr_last_error(nullptr)) > 0, what);
        h = reinterpret_cast<hsr_rows*>(16);
    };
    refused(hsr_create(&h, 0, 0, ip.data()), HS_ERR_BAD_ARG, "no rows");
    refused(hsr_create(&h, 0, 4, nullptr), HS_ERR_BAD_ARG, "null indptr");
    bad = {0, 3, 2, 8, 9};
    refused(hsr_create(&h, 0, 4, bad.data()), HS_ERR_BAD_MATRIX, "indptr decreases");
    bad = {1, 3, 3, 8, 9};
    refused(hsr_create(&h, 0, 4, bad.data()), HS_ERR_BAD_MATRIX, "indptr[0] = 1");
    EXPECT(hsr_create(nullptr, 0, 4, ip.data()) == HS_ERR_BAD_ARG, "null out");
    float one = 1.0f;
    EXPECT(hsr_info(nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG && hsr_sync(nullptr) == HS_ERR_BAD_ARG && hsr_set_stream(nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsr_softmax_device(nullptr, &one, 1.0f, &one) == HS_ERR_BAD_ARG && hsr_softmax(nullptr, &one, 1.0f, &one) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsr_softmax_backward_device(nullptr, &one, &one, 1.0f, &one) == HS_ERR_BAD_ARG && hsr_softmax_backward(nullptr, &one, &one, 1.0f, &one) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsr_destroy(nullptr) == HS_OK, "destroy(NULL)");

    h = nullptr;
    EXPECT(hsr_create(&h, 0, 4, ip.data()) == HS_OK && h, "create");
    if (!h) return;
    const size_t n = 9;
    Floats s(2 * n), p(2 * n), g(2 * n), want(n), out(n);
    for (size_t e = 0; e < 2 * n; ++e) s.v[e] = next_float(4.0f), g.v[e] = next_float(3.0f);
    EXPECT(hsr_softmax_device(h, s.p(), 0.5f, want.p()) == HS_OK, "reference call");
    auto still_usable = [&](int rc, const char* what) {
        EXPECT(rc == HS_ERR_BAD_ARG && std::strlen(hsr_last_error(h)) > 0, what);
        EXPECT(hsr_softmax_device(h, s.p(), 0.5f, out.p()) == HS_OK && std::memcmp(out.p(), want.p(), n * 4) == 0, what);
    };
    const float inf = INFINITY, nan = std::numeric_limits<float>::quiet_NaN();
    float* odd = reinterpret_cast<float*>(reinterpret_cast<char*>(s.p()) + 2);
    still_usable(hsr_softmax_device(h, nullptr, 1.0f, p.p()), "null s");
    still_usable(hsr_softmax_device(h, s.p(), 1.0f, nullptr), "null p");
    still_usable(hsr_softmax_device(h, odd, 1.0f, p.p()), "misaligned s");
    still_usable(hsr_softmax_device(h, p.p(), 1.0f, odd), "misaligned p");
    still_usable(hsr_softmax_device(h, s.p(), inf, p.p()), "scale inf");
    still_usable(hsr_softmax_device(h, s.p(), nan, p.p()), "scale NaN");
    still_usable(hsr_softmax_device(h, s.p(), 1.0f, s.p() + 1), "p one word into s");
    still_usable(hsr_softmax_device(h, s.p() + n - 1, 1.0f, s.p()), "s's last word in p");
    still_usable(hsr_softmax_backward_device(h, nullptr, g.p(), 1.0f, p.p()), "null p");
    still_usable(hsr_softmax_backward_device(h, want.p(), nullptr, 1.0f, p.p()), "null gp");
    still_usable(hsr_softmax_backward_device(h, want.p(), g.p(), 1.0f, nullptr), "null gs");
    still_usable(hsr_softmax_backward_device(h, odd, g.p(), 1.0f, p.p()), "misaligned p");
    still_usable(hsr_softmax_backward_device(h, want.p(), odd, 1.0f, p.p()), "misaligned gp");
    still_usable(hsr_softmax_backward_device(h, want.p(), g.p(), 1.0f, odd), "misaligned gs");
    still_usable(hsr_softmax_backward_device(h, want.p(), g.p(), -inf, p.p()), "scale -inf");
    still_usable(hsr_softmax_backward_device(h, want.p(), g.p(), nan, p.p()), "scale NaN");
    still_usable(hsr_softmax_backward_device(h, p.p(), g.p(), 1.0f, p.p()), "gs is p");
    still_usable(hsr_softmax_backward_device(h, p.p(), g.p(), 1.0f, p.p() + 1), "gs one word into p");
    still_usable(hsr_softmax_backward_device(h, p.p(), g.p(), 1.0f, g.p() + 1), "gs one word into gp");
    still_usable(hsr_softmax_backward_device(h, p.p(), g.p() + 1, 1.0f, g.p()), "gp one word into gs");
    still_usable(hsr_softmax(h, nullptr, 1.0f, p.p()), "host null s");
    still_usable(hsr_softmax(h, s.p(), 1.0f, nullptr), "host null p");
    still_usable(hsr_softmax(h, s.p(), inf, p.p()), "host scale inf");
    still_usable(hsr_softmax(h, s.p(), 1.0f, s.p() + 1), "host overlap");
    still_usable(hsr_softmax_backward(h, nullptr, g.p(), 1.0f, p.p()), "host null p");
    still_usable(hsr_softmax_backward(h, want.p(), g.p(), nan, p.p()), "host scale NaN");
    still_usable(hsr_softmax_backward(h, p.p(), g.p(), 1.0f, p.p()), "host gs is p");
    // ranges that touch without sharing a word, and the host forms on arrays that are not 4-byte aligned
    EXPECT(hsr_softmax_device(h, s.p(), 0.5f, s.p() + n) == HS_OK && std::memcmp(s.p() + n, want.p(), n * 4) == 0, "adjacent ranges");
    std::vector<char> raw_s(n * 4 + 1), raw_p(n * 4 + 1);
    std::memcpy(raw_s.data() + 1, s.p(), n * 4);
    EXPECT(hsr_softmax(h, reinterpret_cast<float*>(raw_s.data() + 1), 0.5f, reinterpret_cast<float*>(raw_p.data() + 1)) == HS_OK && std::memcmp(raw_p.data() + 1, want.p(), n * 4) == 0,
           "host form, odd addresses");
    EXPECT(hsr_destroy(h) == HS_OK, "destroy");
}

}  // namespace

int main() {
    check_edge("nnz = 0", {0, 0, 0, 0, 0});
    check_edge("one row of one entry", {1});
    check_edge("all rows empty but the last", std::vector<uint32_t>{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7});
    check_edge("one row of 70 000 entries", {70000});
    check_edge("every class", {0, 1, 16, 17, 0, 33, 65, 129, 256, 257, 1025, 0});
    refusals();
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("ROWS CPU OK\n");
    return 0;
}
