// test_pattern_cpu.cpp — the CPU twin of include/hisparse_pattern.h (hisparse_amd/csrc/hsp_cpu.cpp) through its C boundary, as a program of
// its own: tests/test_pattern_cpu.py compiles both files with -fsanitize=address,undefined and runs the result.  The edge patterns and
// the refusals of the issue; buffers are exactly as large as the contract says, so a read or write past them is the sanitizer's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hisparse_hip.h"
#include "hisparse_pattern.h"

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
uint32_t next_u32() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return uint32_t(g_seed >> 16);
}

// 16-byte aligned storage of exactly n words (aligned_alloc wants whole multiples of the alignment: the slack is poisoned by nobody, so
// the vectors below are sized in whole quads and hand out n)
struct Words {
    uint32_t* p = nullptr;
    size_t n = 0;
    explicit Words(size_t count) : n(count) {
        p = static_cast<uint32_t*>(std::aligned_alloc(16, ((count * 4 + 15) / 16 + (count == 0)) * 16));
        std::memset(p, 0, count * 4);
    }
    ~Words() { std::free(p); }
    Words(const Words&) = delete;
    Words& operator=(const Words&) = delete;
};

uint32_t q_mul(uint32_t a, uint32_t b) {
    const unsigned __int128 wide = (unsigned __int128)a * b + (1u << 23);
    const unsigned __int128 r = wide >> 24;
    return r > 0xffffffffu ? 0xffffffffu : uint32_t(r);
}

uint32_t value_word(int impl, bool small) {
    if (impl == HS_IMPL_FIXED) return small ? next_u32() >> 7 : next_u32();      // [0, 2) or up to 256: sums saturate
    const float f = (float(next_u32() >> 8) / float(1 << 24) - 0.5f) * 4.0f;
    uint32_t w;
    std::memcpy(&w, &f, 4);
    return w;
}

struct Pattern {
    std::string name;
    uint32_t rows, cols;
    std::vector<uint32_t> indptr, indices;
};

Pattern from_counts(const std::string& name, uint32_t cols, const std::vector<uint32_t>& counts) {
    Pattern p{name, uint32_t(counts.size()), cols, {0}, {}};
    for (uint32_t c : counts) {
        for (uint32_t i = 0; i < c; ++i) p.indices.push_back(next_u32() % cols);      // unsorted, repeats allowed
        p.indptr.push_back(uint32_t(p.indices.size()));
    }
    return p;
}

void check_pattern(const Pattern& pt, int impl, uint32_t k, uint64_t pad, bool large) {
    const std::string what = pt.name + ", impl " + std::to_string(impl) + ", k " + std::to_string(k);
    hsp_pattern* h = nullptr;
    int rc = hsp_create(&h, 0, impl, pt.rows, pt.cols, pt.indptr.data(), pt.indices.empty() ? nullptr : pt.indices.data(), 8);
    EXPECT(rc == HS_OK && h, what);
    if (!h) return;
    uint64_t nnz = 99, bytes = 99;
    EXPECT(hsp_info(h, &nnz, &bytes) == HS_OK && nnz == pt.indices.size(), what);
    EXPECT(hsp_info(h, nullptr, nullptr) == HS_OK, what);
    const uint64_t ldu = (pt.rows + 3u) / 4u * 4u + pad, ldv = (pt.cols + 3u) / 4u * 4u + pad;
    // the last column holds exactly num_rows / num_cols words: "at least num_rows words used"
    Words u((k - 1) * ldu + pt.rows), v((k - 1) * ldv + pt.cols), out(nnz), twice(nnz);
    for (size_t i = 0; i < u.n; ++i) u.p[i] = value_word(impl, !large);
    for (size_t i = 0; i < v.n; ++i) v.p[i] = value_word(impl, !large);
    EXPECT(hsp_sddmm_device(h, u.p, ldu, v.p, ldv, k, out.p, 0) == HS_OK, what);
    EXPECT(hsp_sddmm_device(h, u.p, ldu, v.p, ldv, k, twice.p, 0) == HS_OK && hsp_sddmm_device(h, u.p, ldu, v.p, ldv, k, twice.p, 1) == HS_OK, what);
    EXPECT(hsp_sync(h) == HS_OK && hsp_set_stream(h, nullptr) == HS_OK, what);
    uint64_t e = 0, saturated = 0;
    for (uint32_t r = 0; r < pt.rows; ++r) {
        for (; e < pt.indptr[r + 1]; ++e) {
            const uint32_t c = pt.indices[e];
            if (impl == HS_IMPL_FIXED) {
                uint64_t s = 0;
                for (uint32_t j = 0; j < k; ++j) s += q_mul(u.p[j * ldu + r], v.p[j * ldv + c]);
                const uint32_t want = s > 0xffffffffull ? 0xffffffffu : uint32_t(s);
                const uint32_t want2 = 2 * s > 0xffffffffull ? 0xffffffffu : uint32_t(2 * s);
                saturated += want == 0xffffffffu;
                EXPECT(out.p[e] == want, what + ", entry " + std::to_string(e));
                EXPECT(twice.p[e] == want2, what + ", accumulated entry " + std::to_string(e));
            } else {
                double s = 0.0;
                for (uint32_t j = 0; j < k; ++j) {
                    float a, b;
                    std::memcpy(&a, &u.p[j * ldu + r], 4);
                    std::memcpy(&b, &v.p[j * ldv + c], 4);
                    volatile float prod = a * b;
                    s += double(prod);
                }
                float got, got2;
                std::memcpy(&got, &out.p[e], 4);
                std::memcpy(&got2, &twice.p[e], 4);
                EXPECT(got == float(s), what + ", entry " + std::to_string(e));
                EXPECT(got2 == float(s) + float(s), what + ", accumulated entry " + std::to_string(e));
            }
        }
    }
    EXPECT(e == nnz, what);
    if (large && impl == HS_IMPL_FIXED && nnz >= 50 && k >= 5) EXPECT(saturated > 0, what + ": no sum saturated");
    // the host form: columns back to back at the rounded dimensions
    if (pad == 0) {
        std::vector<uint32_t> hu(k * ldu), hv(k * ldv), ho(nnz);
        for (uint32_t j = 0; j < k; ++j) {
            for (uint32_t i = 0; i < pt.rows; ++i) hu[j * ldu + i] = u.p[j * ldu + i];
            for (uint32_t i = 0; i < pt.cols; ++i) hv[j * ldv + i] = v.p[j * ldv + i];
        }
        uint32_t dummy = 0;
        EXPECT(hsp_sddmm(h, hu.data(), hv.data(), k, nnz ? ho.data() : &dummy) == HS_OK, what + ", host form");
        EXPECT(nnz == 0 || std::memcmp(ho.data(), out.p, nnz * 4) == 0, what + ", host form");
    }
    EXPECT(hsp_destroy(h) == HS_OK, what);
}

void refusals(int impl) {
    const std::vector<uint32_t> indptr = {0, 2, 2, 5, 7}, indices = {1, 8, 0, 3, 3, 2, 8};
    std::vector<uint32_t> bad;
    hsp_pattern* h = reinterpret_cast<hsp_pattern*>(16);
    auto refused = [&](int rc, int code, const char* what) {
        EXPECT(rc == code && h == nullptr && std::strlen(hsp_last_error(nullptr)) > 0, what);
        h = reinterpret_cast<hsp_pattern*>(16);
    };
    refused(hsp_create(&h, 0, impl, 4, 9, indptr.data(), indices.data(), 0), HS_ERR_BAD_ARG, "max_k 0");
    refused(hsp_create(&h, 0, impl, 4, 9, indptr.data(), indices.data(), 65), HS_ERR_BAD_ARG, "max_k 65");
    refused(hsp_create(&h, 0, 7, 4, 9, indptr.data(), indices.data(), 4), HS_ERR_BAD_ARG, "impl 7");
    refused(hsp_create(&h, 0, impl, 4, 9, nullptr, indices.data(), 4), HS_ERR_BAD_ARG, "null indptr");
    refused(hsp_create(&h, 0, impl, 4, 9, indptr.data(), nullptr, 4), HS_ERR_BAD_ARG, "null indices");
    refused(hsp_create(&h, 0, impl, 4, 8, indptr.data(), indices.data(), 4), HS_ERR_BAD_MATRIX, "index = num_cols");
    bad = {0, 2, 1, 5, 7};
    refused(hsp_create(&h, 0, impl, 4, 9, bad.data(), indices.data(), 4), HS_ERR_BAD_MATRIX, "indptr decreases");
    bad = {1, 2, 2, 5, 7};
    refused(hsp_create(&h, 0, impl, 4, 9, bad.data(), indices.data(), 4), HS_ERR_BAD_MATRIX, "indptr[0] = 1");
    EXPECT(hsp_create(nullptr, 0, impl, 4, 9, indptr.data(), indices.data(), 4) == HS_ERR_BAD_ARG, "null out");
    EXPECT(hsp_info(nullptr, nullptr, nullptr) == HS_ERR_BAD_ARG && hsp_sync(nullptr) == HS_ERR_BAD_ARG && hsp_set_stream(nullptr, nullptr) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsp_sddmm_device(nullptr, &bad, 4, &bad, 12, 1, &bad, 0) == HS_ERR_BAD_ARG && hsp_sddmm(nullptr, &bad, &bad, 1, &bad) == HS_ERR_BAD_ARG, "null object");
    EXPECT(hsp_destroy(nullptr) == HS_OK, "destroy(NULL)");

    h = nullptr;
    EXPECT(hsp_create(&h, 0, impl, 4, 9, indptr.data(), indices.data(), 4) == HS_OK && h, "create");
    if (!h) return;
    Words u(4 * 4), v(4 * 12), out(8), want(8);
    for (size_t i = 0; i < u.n; ++i) u.p[i] = value_word(impl, true);
    for (size_t i = 0; i < v.n; ++i) v.p[i] = value_word(impl, true);
    EXPECT(hsp_sddmm_device(h, u.p, 4, v.p, 12, 4, want.p, 0) == HS_OK, "reference call");
    auto still_usable = [&](int rc, const char* what) {
        EXPECT(rc == HS_ERR_BAD_ARG && std::strlen(hsp_last_error(h)) > 0, what);
        EXPECT(hsp_sddmm_device(h, u.p, 4, v.p, 12, 4, out.p, 0) == HS_OK && std::memcmp(out.p, want.p, 7 * 4) == 0, what);
    };
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p, 12, 0, out.p, 0), "k = 0");
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p, 12, 5, out.p, 0), "k > max_k");
    still_usable(hsp_sddmm_device(h, u.p + 1, 4, v.p, 12, 1, out.p, 0), "misaligned u");
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p + 2, 12, 1, out.p, 0), "misaligned v");
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p, 12, 1, out.p + 3, 0), "misaligned out");
    still_usable(hsp_sddmm_device(h, u.p, 6, v.p, 12, 1, out.p, 0), "odd ldu");
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p, 11, 1, out.p, 0), "odd ldv");
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p, 8, 1, out.p, 0), "ldv < num_cols");
    still_usable(hsp_sddmm_device(h, nullptr, 4, v.p, 12, 1, out.p, 0), "null u");
    still_usable(hsp_sddmm_device(h, u.p, 4, nullptr, 12, 1, out.p, 0), "null v");
    still_usable(hsp_sddmm_device(h, u.p, 4, v.p, 12, 1, nullptr, 0), "null out");
    still_usable(hsp_sddmm(h, u.p, v.p, 0, out.p), "host k = 0");
    still_usable(hsp_sddmm(h, u.p, v.p, 5, out.p), "host k > max_k");
    still_usable(hsp_sddmm(h, nullptr, v.p, 1, out.p), "host null u");
    still_usable(hsp_sddmm(h, u.p, v.p, 1, nullptr), "host null out");
    EXPECT(hsp_destroy(h) == HS_OK, "destroy");
}

}  // namespace

int main() {
    std::vector<Pattern> patterns;
    patterns.push_back(from_counts("nnz = 0", 7, {0, 0, 0, 0, 0}));
    for (uint32_t n : {1u, 2u, 3u, 5u, 7u}) patterns.push_back(from_counts("nnz = " + std::to_string(n), 9, {0, n / 2, 0, n - n / 2, 0, 0}));
    {
        std::vector<uint32_t> counts(40, 0);      // empty rows first, in runs between, and last
        counts[7] = 3, counts[8] = 1, counts[20] = 6, counts[31] = 2;
        patterns.push_back(from_counts("runs of empty rows", 11, counts));
    }
    patterns.push_back(from_counts("one row holds every entry", 301, {0, 0, 0, 0, 300, 0, 0, 0, 0}));
    patterns.push_back({"an entry in the last row and column", 7, 13, {0, 1, 1, 1, 1, 1, 1, 2}, {0, 12}});
    patterns.push_back({"unsorted columns", 3, 10, {0, 4, 4, 9}, {9, 0, 5, 2, 7, 1, 8, 3, 4}});
    patterns.push_back({"a pair held twice", 3, 6, {0, 1, 5, 6}, {2, 4, 1, 4, 0, 3}});
    for (const Pattern& pt : patterns)
        for (int impl : {HS_IMPL_FIXED, HS_IMPL_FLOAT_POB, HS_IMPL_FLOAT_STALL})
            for (uint32_t k : {1u, 5u})
                for (uint64_t pad : {uint64_t(0), uint64_t(8)}) check_pattern(pt, impl, k, pad, pad != 0);
    for (int impl : {HS_IMPL_FIXED, HS_IMPL_FLOAT_POB, HS_IMPL_FLOAT_STALL}) refusals(impl);
    if (g_failures) {
        std::printf("%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("PATTERN CPU OK\n");
    return 0;
}
