// hsmh_cpu.cpp — include/hisparse_heads.h in libhisparse_cpu.so: multi-head attention over a CSR pattern, forward and backward, on the
// host, for machines WITHOUT a GPU.  Like hsat_cpu.cpp and hsab_cpu.cpp a second implementation that a driver loads INSTEAD of
// libhisparse_hip.so, never a fallback of it.  "Device" pointers are host pointers here, hsmh_set_stream accepts and ignores, hsmh_sync
// is a no-op.  Single-threaded: plain loops on the calling thread, head by head, two passes per row (forward: the scores and their
// maximum, then the weights and the sums; backward: the weights, the dots of gY and V and their sum D, then the three gradients); gK and
// gV of a head are summed in double over all rows and rounded at the end.  HSMH_BACKWARD is recorded and checked as the device library
// checks it; nothing is built for it.
//
// Arithmetic = the kernels' (heads_attention.hip), the header's ARITHMETIC paragraph: one fp32 multiply per product (built with
// -ffp-contract=off), added in double, s rounded once; t = scale * s in fp32; everything after that in double, one rounding per output
// word.
// The four hsmh16_* calls of include/hisparse_heads_bf16.h run the same loops over bf16 elements (widen / narrow below): the operands
// widened exactly, the same sums, and each output word rounded to fp32 and then to bf16.
// The five hsmhb_* calls of include/hisparse_heads_bias.h run the fp32 loops with one more fp32 add per score, t = (scale * s) + bias of
// the entry and head, and store gB = P (GP - D) per entry and head, formed in double and rounded once, where gbias is given.
// The five hsmhd_* calls of include/hisparse_heads_dropout.h run the fp32 loops with a weight w = keep(e, h) ? c : 0 per entry and head from
// philox.h's generator: forward, l over all entries and the sums over w times the weight; backward, GP becomes w GP and gV takes w P.
// With drop_p = 0 every w is 1.0 and the loops form the words of the calls without dropout.
// The four hsmhd16_* calls of include/hisparse_heads_dropout_bf16.h run those loops over bf16 elements: widen, the fp32 bias, w, narrow.
// The four hsgat_* calls of include/hisparse_gat.h run loops of their own (gat_forward_head, gat_backward_head): the score is
// x = el[row] + er[col], one fp32 add, and t = x > 0 ? x : slope * x, one fp32 multiply; the rest in double as above; gel = A - D B.
// The six hsgat2_* calls of include/hisparse_gatv2.h run loops of their own too (gat2_forward_head, gat2_backward_head): z = xd + xs and
// w = LeakyReLU(z) per word, t = a . w with fp32 products added in double; gXD = a (A - D B) per word, and ga is the rows' A' - D B' added
// in row order in the doubles of the caller's workspace (ONE vector here) and rounded once.
// No dependency beyond the headers and hsmh_common.h: tests/cpp/test_heads_cpu.cpp compiles this file alone under the sanitizers.
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "hisparse_gat.h"
#include "hisparse_gatv2.h"
#include "hisparse_heads_bf16.h"
#include "hisparse_heads_bias.h"
#include "hisparse_heads_dropout.h"
#include "hisparse_heads_dropout_bf16.h"
#include "hsmh_common.h"

struct hsmh_pattern {
    uint32_t num_rows = 0, num_cols = 0, max_heads = 0;
    bool backward = false;
    bool map = false;      // hsmhb_create with HSMH_BACKWARD: what the device library keeps the entry map for
    std::vector<uint32_t> indptr, indices;
    std::string error;
    uint64_t nnz() const { return indptr.back(); }
};

namespace {

thread_local std::string g_create_error;

int fail(hsmh_pattern* p, int code, const std::string& msg) {
    if (p) p->error = msg; else g_create_error = msg;
    return code;
}

// An element as the arithmetic reads it and an output word as it is stored.  fp32: the word itself and one rounding.  bf16 (a bit pattern
// in uint16_t): the upper half of the fp32 of the same value, so widening is exact; an output word is rounded to fp32 and then to bf16,
// to nearest even, and a NaN stays a NaN (the integer rounding alone would carry some NaNs into infinity).  +-inf and -0 survive.
inline float widen(float x) { return x; }
inline float widen(uint16_t x) {
    const uint32_t bits = uint32_t(x) << 16;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
inline void narrow(double x, float& out) { out = float(x); }
inline void narrow(double x, uint16_t& out) {
    const float f = float(x);
    uint32_t bits;
    std::memcpy(&bits, &f, 4);
    out = f != f ? uint16_t((bits >> 16) | 0x0040u) : uint16_t((bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16);
}

// one head: the pointers are the head's first word of row 0, lse (may be null) its word of row 0
template <typename T>
void forward_head(const hsmh_pattern* p, const T* q, uint64_t ldq, const T* k, uint64_t ldk, const T* v, uint64_t ldv, uint32_t d, float scale, T* y, uint64_t ldy,
                  float* lse, uint64_t ldl, const float* bias = nullptr, uint64_t ldb = 0, const hisparse::philox::Dropout* dr = nullptr, uint32_t head = 0) {
    const float ninf = -std::numeric_limits<float>::infinity();
    std::vector<float> t;
    std::vector<double> acc(d);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        T* dst = y + uint64_t(r) * ldy;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = T(0);
            if (lse) lse[uint64_t(r) * ldl] = ninf;
            continue;
        }
        const T* a = q + uint64_t(r) * ldq;
        t.resize(hi - lo);
        float m = ninf;      // one of the t words; a NaN is never the maximum
        for (uint64_t e = lo; e < hi; ++e) {
            const T* b = k + uint64_t(p->indices[e]) * ldk;
            double s = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(widen(a[j]) * widen(b[j]));
            t[e - lo] = scale * float(s);
            if (bias) t[e - lo] = t[e - lo] + bias[e * ldb];      // the second rounding of t (hisparse_heads_bias.h)
            m = std::fmax(m, t[e - lo]);
        }
        double l = 0.0;
        acc.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            // a -inf score weighs exactly 0, also while the maximum is -inf itself; a NaN, or +inf under a maximum of +inf, gives NaN
            const double w = t[e - lo] == ninf ? 0.0 : std::exp(double(t[e - lo]) - double(m));
            const T* b = v + uint64_t(p->indices[e]) * ldv;
            l += w;      // over every entry, dropped or not
            const double wv = dr ? (hisparse::philox::keep(*dr, uint32_t(e), head) ? dr->c : 0.0) * w : w;
            for (uint32_t j = 0; j < d; ++j) acc[j] += wv * double(widen(b[j]));
        }
        for (uint32_t j = 0; j < d; ++j) narrow(acc[j] / l, dst[j]);
        if (lse) lse[uint64_t(r) * ldl] = float(double(m) + std::log(l));
    }
}

template <typename T>
void backward_head(const hsmh_pattern* p, const T* q, uint64_t ldq, const T* k, uint64_t ldk, const T* v, uint64_t ldv, const T* gy, uint64_t ldgy, const float* lse, uint64_t ldl,
                   uint32_t d, float scale, T* gq, uint64_t ldgq, T* gk, uint64_t ldgk, T* gv, uint64_t ldgv, const float* bias = nullptr, uint64_t ldb = 0,
                   float* gbias = nullptr, uint64_t ldgb = 0, const hisparse::philox::Dropout* dr = nullptr, uint32_t head = 0) {
    std::vector<double> w, gp, wt, row(d);
    std::vector<double> sum_k(size_t(p->num_cols) * d, 0.0), sum_v(size_t(p->num_cols) * d, 0.0);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        T* dst = gq + uint64_t(r) * ldgq;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = T(0);
            continue;
        }
        const T* a = q + uint64_t(r) * ldq;
        const T* g = gy + uint64_t(r) * ldgy;
        // a word that is not finite (a dead or bad row of the forward) makes every weight of the row's head NaN
        const float lw = lse[uint64_t(r) * ldl];
        const double l = std::isfinite(lw) ? double(lw) : std::numeric_limits<double>::quiet_NaN();
        w.resize(hi - lo);
        gp.resize(hi - lo);
        wt.assign(hi - lo, 1.0);
        double dsum = 0.0;
        for (uint64_t e = lo; e < hi; ++e) {
            const T* b = k + uint64_t(p->indices[e]) * ldk;
            const T* c = v + uint64_t(p->indices[e]) * ldv;
            double s = 0.0, x = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(widen(a[j]) * widen(b[j]));
            for (uint32_t j = 0; j < d; ++j) x += double(widen(g[j]) * widen(c[j]));
            float t = scale * float(s);
            if (bias) t = t + bias[e * ldb];
            w[e - lo] = std::exp(double(t) - l);      // a -inf score under a finite lse weighs exactly 0
            if (dr) {      // GP = w (gY . V): 1.0 x = x without dropout
                wt[e - lo] = hisparse::philox::keep(*dr, uint32_t(e), head) ? dr->c : 0.0;
                x = wt[e - lo] * x;
            }
            gp[e - lo] = x;
            dsum += w[e - lo] * x;
        }
        row.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            const uint32_t c = p->indices[e];
            const double pe = w[e - lo], gb = pe * (gp[e - lo] - dsum), gs = double(scale) * gb, pw = dr ? wt[e - lo] * pe : pe;
            if (gbias) gbias[e * ldgb] = float(gb);
            const T* b = k + uint64_t(c) * ldk;
            double* to_k = sum_k.data() + size_t(c) * d;
            double* to_v = sum_v.data() + size_t(c) * d;
            for (uint32_t j = 0; j < d; ++j) {
                row[j] += gs * double(widen(b[j]));
                to_k[j] += gs * double(widen(a[j]));
                to_v[j] += pw * double(widen(g[j]));
            }
        }
        for (uint32_t j = 0; j < d; ++j) narrow(row[j], dst[j]);
    }
    for (uint32_t c = 0; c < p->num_cols; ++c) {
        for (uint32_t j = 0; j < d; ++j) {
            narrow(sum_k[size_t(c) * d + j], gk[uint64_t(c) * ldgk + j]);
            narrow(sum_v[size_t(c) * d + j], gv[uint64_t(c) * ldgv + j]);
        }
    }
}

template <typename T>
void forward(const hsmh_pattern* p, const T* q, uint64_t ldq, const T* k, uint64_t ldk, const T* v, uint64_t ldv, uint32_t heads, uint32_t d, float scale, T* y, uint64_t ldy,
             float* lse, uint64_t ldl, const float* bias = nullptr, uint64_t ldb = 0, const hisparse::philox::Dropout* dr = nullptr) {
    for (uint32_t h = 0; h < heads; ++h) {
        const uint32_t at = h * d;
        forward_head(p, q + at, ldq, k + at, ldk, v + at, ldv, d, scale, y + at, ldy, lse ? lse + h : nullptr, ldl, bias ? bias + h : nullptr, ldb, dr, h);
    }
}

template <typename T>
void backward(const hsmh_pattern* p, const T* q, uint64_t ldq, const T* k, uint64_t ldk, const T* v, uint64_t ldv, const T* gy, uint64_t ldgy, const float* lse, uint64_t ldl,
              uint32_t heads, uint32_t d, float scale, T* gq, uint64_t ldgq, T* gk, uint64_t ldgk, T* gv, uint64_t ldgv, const float* bias = nullptr, uint64_t ldb = 0,
              float* gbias = nullptr, uint64_t ldgb = 0, const hisparse::philox::Dropout* dr = nullptr) {
    for (uint32_t h = 0; h < heads; ++h) {
        const uint32_t at = h * d;
        backward_head(p, q + at, ldq, k + at, ldk, v + at, ldv, gy + at, ldgy, lse + h, ldl, d, scale, gq + at, ldgq, gk + at, ldgk, gv + at, ldgv, bias ? bias + h : nullptr, ldb,
                      gbias ? gbias + h : nullptr, ldgb, dr, h);
    }
}

// ---- include/hisparse_gat.h: one head; el, gel and lse point at the head's word of row 0, er and ger at its word of column 0 ------------
inline float gat_score(float a, float b) { return a + b; }                                        // x: one fp32 add
inline float gat_leaky(float x, float slope) { return x > 0.0f ? x : slope * x; }                 // t: one fp32 multiply; x == 0 and NaN take the slope branch
inline double gat_slope_at(float x, float slope) { return x > 0.0f ? 1.0 : double(slope); }      // torch's leaky_relu derivative, at x == 0 too

void gat_forward_head(const hsmh_pattern* p, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, uint32_t d, float slope, float* y,
                      uint64_t ldy, float* lse, uint64_t ldl) {
    const float ninf = -std::numeric_limits<float>::infinity();
    std::vector<float> t;
    std::vector<double> acc(d);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        float* dst = y + uint64_t(r) * ldy;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = 0.0f;
            if (lse) lse[uint64_t(r) * ldl] = ninf;
            continue;
        }
        const float a = el[uint64_t(r) * ldel];
        t.resize(hi - lo);
        float m = ninf;      // one of the t words; a NaN is never the maximum
        for (uint64_t e = lo; e < hi; ++e) {
            t[e - lo] = gat_leaky(gat_score(a, er[uint64_t(p->indices[e]) * lder]), slope);
            m = std::fmax(m, t[e - lo]);
        }
        double l = 0.0;
        acc.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            // a -inf score weighs exactly 0, also while the maximum is -inf itself; a NaN, or +inf under a maximum of +inf, gives NaN
            const double w = t[e - lo] == ninf ? 0.0 : std::exp(double(t[e - lo]) - double(m));
            const float* b = v + uint64_t(p->indices[e]) * ldv;
            l += w;
            for (uint32_t j = 0; j < d; ++j) acc[j] += w * double(b[j]);
        }
        for (uint32_t j = 0; j < d; ++j) dst[j] = float(acc[j] / l);
        if (lse) lse[uint64_t(r) * ldl] = float(double(m) + std::log(l));
    }
}

void gat_backward_head(const hsmh_pattern* p, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy,
                       const float* lse, uint64_t ldl, uint32_t d, float slope, float* gel, uint64_t ldgel, float* ger, uint64_t ldger, float* gv, uint64_t ldgv) {
    std::vector<double> w, gp, dx;
    std::vector<double> sum_r(p->num_cols, 0.0), sum_v(size_t(p->num_cols) * d, 0.0);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        if (lo == hi) {
            gel[uint64_t(r) * ldgel] = 0.0f;
            continue;
        }
        const float a = el[uint64_t(r) * ldel];
        const float* g = gy + uint64_t(r) * ldgy;
        // a word that is not finite (a dead or bad row of the forward) makes every weight of the row's head NaN
        const float lw = lse[uint64_t(r) * ldl];
        const double l = std::isfinite(lw) ? double(lw) : std::numeric_limits<double>::quiet_NaN();
        w.resize(hi - lo);
        gp.resize(hi - lo);
        dx.resize(hi - lo);
        double dsum = 0.0, asum = 0.0, bsum = 0.0;      // D = sum P GP, A = sum P GP dx, B = sum P dx
        for (uint64_t e = lo; e < hi; ++e) {
            const float* c = v + uint64_t(p->indices[e]) * ldv;
            const float x = gat_score(a, er[uint64_t(p->indices[e]) * lder]);
            double s = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(g[j] * c[j]);
            w[e - lo] = std::exp(double(gat_leaky(x, slope)) - l);      // a -inf score under a finite lse weighs exactly 0
            gp[e - lo] = s;
            dx[e - lo] = gat_slope_at(x, slope);
            const double pg = w[e - lo] * s;
            dsum += pg;
            asum += pg * dx[e - lo];
            bsum += w[e - lo] * dx[e - lo];
        }
        gel[uint64_t(r) * ldgel] = float(asum - dsum * bsum);
        for (uint64_t e = lo; e < hi; ++e) {
            const uint32_t c = p->indices[e];
            const double pe = w[e - lo];
            sum_r[c] += (pe * (gp[e - lo] - dsum)) * dx[e - lo];
            double* to_v = sum_v.data() + size_t(c) * d;
            for (uint32_t j = 0; j < d; ++j) to_v[j] += pe * double(g[j]);
        }
    }
    for (uint32_t c = 0; c < p->num_cols; ++c) {
        ger[uint64_t(c) * ldger] = float(sum_r[c]);
        for (uint32_t j = 0; j < d; ++j) gv[uint64_t(c) * ldgv + j] = float(sum_v[size_t(c) * d + j]);
    }
}

void gat_forward(const hsmh_pattern* p, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, uint32_t heads, uint32_t d, float slope, float* y,
                 uint64_t ldy, float* lse, uint64_t ldl) {
    for (uint32_t h = 0; h < heads; ++h) gat_forward_head(p, el + h, ldel, er + h, lder, v + h * d, ldv, d, slope, y + h * d, ldy, lse ? lse + h : nullptr, ldl);
}

void gat_backward(const hsmh_pattern* p, const float* el, uint64_t ldel, const float* er, uint64_t lder, const float* v, uint64_t ldv, const float* gy, uint64_t ldgy, const float* lse,
                  uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gel, uint64_t ldgel, float* ger, uint64_t ldger, float* gv, uint64_t ldgv) {
    for (uint32_t h = 0; h < heads; ++h)
        gat_backward_head(p, el + h, ldel, er + h, lder, v + h * d, ldv, gy + h * d, ldgy, lse + h, ldl, d, slope, gel + h, ldgel, ger + h, ldger, gv + h * d, ldgv);
}

// ---- include/hisparse_gatv2.h: one head; xd, xs, a, gy, y, gxd, gxs and ga point at the head's first word, lse at its word of row 0 --------
// t = fl32(sum_j fl32(a_j * w_j)), w_j = LeakyReLU(fl32(xd_j + xs_j)): fp32 products added in double, one rounding
inline float gat2_score(const float* xd, const float* xs, const float* a, uint32_t d, float slope) {
    double s = 0.0;
    for (uint32_t j = 0; j < d; ++j) s += double(a[j] * gat_leaky(gat_score(xd[j], xs[j]), slope));
    return float(s);
}

void gat2_forward_head(const hsmh_pattern* p, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, uint32_t d, float slope, float* y, uint64_t ldy, float* lse,
                       uint64_t ldl) {
    const float ninf = -std::numeric_limits<float>::infinity();
    std::vector<float> t;
    std::vector<double> acc(d);
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        float* dst = y + uint64_t(r) * ldy;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = 0.0f;
            if (lse) lse[uint64_t(r) * ldl] = ninf;
            continue;
        }
        const float* x = xd + uint64_t(r) * ldxd;
        t.resize(hi - lo);
        float m = ninf;      // one of the t words; a NaN is never the maximum
        for (uint64_t e = lo; e < hi; ++e) {
            t[e - lo] = gat2_score(x, xs + uint64_t(p->indices[e]) * ldxs, a, d, slope);
            m = std::fmax(m, t[e - lo]);
        }
        double l = 0.0;
        acc.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            // a -inf score weighs exactly 0, also while the maximum is -inf itself; a NaN, or +inf under a maximum of +inf, gives NaN
            const double w = t[e - lo] == ninf ? 0.0 : std::exp(double(t[e - lo]) - double(m));
            const float* b = xs + uint64_t(p->indices[e]) * ldxs;
            l += w;
            for (uint32_t j = 0; j < d; ++j) acc[j] += w * double(b[j]);
        }
        for (uint32_t j = 0; j < d; ++j) dst[j] = float(acc[j] / l);
        if (lse) lse[uint64_t(r) * ldl] = float(double(m) + std::log(l));
    }
}

// ga_sum: d doubles, the head's words of the caller's workspace (or of the host form's own), rounded once into ga at the end
void gat2_backward_head(const hsmh_pattern* p, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, const float* gy, uint64_t ldgy, const float* lse,
                        uint64_t ldl, uint32_t d, float slope, float* gxd, uint64_t ldgxd, float* gxs, uint64_t ldgxs, float* ga, double* ga_sum) {
    std::vector<double> w, gp, sa(d), sb(d), ta(d), tb(d);
    std::vector<double> sum_v(size_t(p->num_cols) * d, 0.0), sum_z(size_t(p->num_cols) * d, 0.0);
    std::vector<uint32_t> count(p->num_cols, 0);
    for (uint32_t j = 0; j < d; ++j) ga_sum[j] = 0.0;
    for (uint32_t r = 0; r < p->num_rows; ++r) {
        const uint64_t lo = p->indptr[r], hi = p->indptr[r + 1];
        float* dst = gxd + uint64_t(r) * ldgxd;
        if (lo == hi) {
            for (uint32_t j = 0; j < d; ++j) dst[j] = 0.0f;
            continue;
        }
        const float* x = xd + uint64_t(r) * ldxd;
        const float* g = gy + uint64_t(r) * ldgy;
        // a word that is not finite (a dead or bad row of the forward) makes every weight of the row's head NaN
        const float lw = lse[uint64_t(r) * ldl];
        const double l = std::isfinite(lw) ? double(lw) : std::numeric_limits<double>::quiet_NaN();
        w.resize(hi - lo);
        gp.resize(hi - lo);
        double dsum = 0.0;      // D = sum P GP; per word A = sum P GP dz, B = sum P dz, A' = sum P GP w, B' = sum P w
        sa.assign(d, 0.0);
        sb.assign(d, 0.0);
        ta.assign(d, 0.0);
        tb.assign(d, 0.0);
        for (uint64_t e = lo; e < hi; ++e) {
            const float* c = xs + uint64_t(p->indices[e]) * ldxs;
            double s = 0.0;
            for (uint32_t j = 0; j < d; ++j) s += double(g[j] * c[j]);
            const double pe = std::exp(double(gat2_score(x, c, a, d, slope)) - l);      // a -inf score under a finite lse weighs exactly 0
            const double pg = pe * s;
            w[e - lo] = pe;
            gp[e - lo] = s;
            dsum += pg;
            for (uint32_t j = 0; j < d; ++j) {
                const float z = gat_score(x[j], c[j]);
                const double dz = gat_slope_at(z, slope), wj = double(gat_leaky(z, slope));
                sa[j] += pg * dz;
                sb[j] += pe * dz;
                ta[j] += pg * wj;
                tb[j] += pe * wj;
            }
        }
        for (uint32_t j = 0; j < d; ++j) {
            dst[j] = float(double(a[j]) * (sa[j] - dsum * sb[j]));
            ga_sum[j] += ta[j] - dsum * tb[j];
        }
        for (uint64_t e = lo; e < hi; ++e) {
            const uint32_t c = p->indices[e];
            const float* b = xs + uint64_t(c) * ldxs;
            const double pe = w[e - lo], gt = pe * (gp[e - lo] - dsum);
            double* to_v = sum_v.data() + size_t(c) * d;
            double* to_z = sum_z.data() + size_t(c) * d;
            ++count[c];
            for (uint32_t j = 0; j < d; ++j) {
                to_v[j] += pe * double(g[j]);
                to_z[j] += gt * gat_slope_at(gat_score(x[j], b[j]), slope);
            }
        }
    }
    for (uint32_t c = 0; c < p->num_cols; ++c) {      // a column without entries: +0.0 whatever a holds
        for (uint32_t j = 0; j < d; ++j) gxs[uint64_t(c) * ldgxs + j] = count[c] ? float(sum_v[size_t(c) * d + j] + double(a[j]) * sum_z[size_t(c) * d + j]) : 0.0f;
    }
    for (uint32_t j = 0; j < d; ++j) ga[j] = float(ga_sum[j]);
}

void gat2_forward(const hsmh_pattern* p, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, uint32_t heads, uint32_t d, float slope, float* y, uint64_t ldy,
                  float* lse, uint64_t ldl) {
    for (uint32_t h = 0; h < heads; ++h) gat2_forward_head(p, xd + h * d, ldxd, xs + h * d, ldxs, a + h * d, d, slope, y + h * d, ldy, lse ? lse + h : nullptr, ldl);
}

void gat2_backward(const hsmh_pattern* p, const float* xd, uint64_t ldxd, const float* xs, uint64_t ldxs, const float* a, const float* gy, uint64_t ldgy, const float* lse, uint64_t ldl,
                   uint32_t heads, uint32_t d, float slope, float* gxd, uint64_t ldgxd, float* gxs, uint64_t ldgxs, float* ga, double* work) {
    for (uint32_t h = 0; h < heads; ++h)
        gat2_backward_head(p, xd + h * d, ldxd, xs + h * d, ldxs, a + h * d, gy + h * d, ldgy, lse + h, ldl, d, slope, gxd + h * d, ldgxd, gxs + h * d, ldgxs, ga + h * d, work + h * d);
}

}  // namespace

extern "C" {

int hsmh_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags) {
    (void)device_id;
    if (!out) return fail(nullptr, HS_ERR_BAD_ARG, "null pattern pointer");
    *out = nullptr;
    std::string why;
    if (int rc = hisparse::hsmh::check_create(num_rows, num_cols, indptr, indices, max_heads, flags, why)) return fail(nullptr, rc, why);
    hsmh_pattern* p = new (std::nothrow) hsmh_pattern;
    if (!p) return fail(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    p->num_rows = num_rows;
    p->num_cols = num_cols;
    p->max_heads = max_heads;
    p->backward = (flags & HSMH_BACKWARD) != 0;
    p->indptr.assign(indptr, indptr + size_t(num_rows) + 1);
    if (p->nnz()) p->indices.assign(indices, indices + p->nnz());
    *out = p;
    return HS_OK;
}

int hsmh_destroy(hsmh_pattern* p) {
    delete p;
    return HS_OK;
}

const char* hsmh_last_error(const hsmh_pattern* p) { return p ? p->error.c_str() : g_create_error.c_str(); }

int hsmh_info(const hsmh_pattern* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz();
    if (device_bytes) *device_bytes = 0;      // nothing lives on a device
    return HS_OK;
}

int hsmh_set_stream(hsmh_pattern* p, void* hip_stream) {
    (void)hip_stream;
    return p ? HS_OK : HS_ERR_BAD_ARG;
}

int hsmh_sync(hsmh_pattern* p) { return p ? HS_OK : HS_ERR_BAD_ARG; }

int hsmh_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d, float scale,
                        float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward(p->num_rows, p->num_cols, p->max_heads, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    forward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl);
    return HS_OK;
}

// the host forms: ld = heads * d, ldl = heads and no alignment rule, so the loops walk the caller's arrays as they are
int hsmh_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, uint32_t heads, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_host(p->num_rows, p->num_cols, p->max_heads, q, k, v, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    forward(p, q, w, k, w, v, w, heads, d, scale, y, w, lse, heads);
    return HS_OK;
}

int hsmh_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                         const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float scale, float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev,
                         uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward(p->num_rows, p->num_cols, p->max_heads, p->backward, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale,
                                                gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, why))
        return fail(p, rc, why);
    backward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv);
    return HS_OK;
}

int hsmh_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, uint32_t heads, uint32_t d, float scale, float* gq, float* gk,
                  float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_host(p->num_rows, p->num_cols, p->max_heads, p->backward, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    backward(p, q, w, k, w, v, w, gy, w, lse, heads, heads, d, scale, gq, w, gk, w, gv, w);
    return HS_OK;
}

// ---- include/hisparse_heads_bf16.h: the same object, bf16 operands ----------------------------------------------------------------------
int hsmh16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                          float scale, uint16_t* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward16(p->num_rows, p->num_cols, p->max_heads, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    forward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl);
    return HS_OK;
}

int hsmh16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint32_t heads, uint32_t d, float scale, uint16_t* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward16_host(p->num_rows, p->num_cols, p->max_heads, q, k, v, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    forward(p, q, w, k, w, v, w, heads, d, scale, y, w, lse, heads);
    return HS_OK;
}

int hsmh16_backward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const uint16_t* gy_dev,
                           uint64_t ldgy, const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float scale, uint16_t* gq_dev, uint64_t ldgq, uint16_t* gk_dev, uint64_t ldgk,
                           uint16_t* gv_dev, uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward16(p->num_rows, p->num_cols, p->max_heads, p->backward, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale,
                                                  gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, why))
        return fail(p, rc, why);
    backward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv);
    return HS_OK;
}

int hsmh16_backward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy, const float* lse, uint32_t heads, uint32_t d, float scale,
                    uint16_t* gq, uint16_t* gk, uint16_t* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward16_host(p->num_rows, p->num_cols, p->max_heads, p->backward, q, k, v, gy, lse, heads, d, scale, gq, gk, gv, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    backward(p, q, w, k, w, v, w, gy, w, lse, heads, heads, d, scale, gq, w, gk, w, gv, w);
    return HS_OK;
}

// ---- include/hisparse_heads_bias.h: the same object, a bias per entry and head --------------------------------------------------------
int hsmhb_create(hsmh_pattern** out, int device_id, uint32_t num_rows, uint32_t num_cols, const uint32_t* indptr, const uint32_t* indices, uint32_t max_heads, uint32_t flags) {
    const int rc = hsmh_create(out, device_id, num_rows, num_cols, indptr, indices, max_heads, flags);
    if (rc == HS_OK) (*out)->map = (*out)->backward;
    return rc;
}

int hsmhb_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* bias_dev, uint64_t ldb,
                         uint32_t heads, uint32_t d, float scale, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_bias(p->num_rows, p->num_cols, p->max_heads, p->nnz(), q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, y_dev, ldy,
                                                    lse_dev, ldl, why))
        return fail(p, rc, why);
    forward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, bias_dev, ldb);
    return HS_OK;
}

int hsmhb_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias, uint32_t heads, uint32_t d, float scale, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_bias_host(p->num_rows, p->num_cols, p->max_heads, p->nnz(), q, k, v, bias, heads, d, scale, y, lse, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    forward(p, q, w, k, w, v, w, heads, d, scale, y, w, lse, heads, bias, heads);
    return HS_OK;
}

int hsmhb_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float* gq_dev, uint64_t ldgq,
                          float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv, float* gbias_dev, uint64_t ldgb) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_bias(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz(), q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev,
                                                     ldb, heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, gbias_dev, ldgb, why))
        return fail(p, rc, why);
    backward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, bias_dev, ldb, gbias_dev, ldgb);
    return HS_OK;
}

int hsmhb_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale,
                   float* gq, float* gk, float* gv, float* gbias) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_bias_host(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz(), q, k, v, gy, lse, bias, heads, d, scale, gq, gk, gv, gbias, why))
        return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    backward(p, q, w, k, w, v, w, gy, w, lse, heads, heads, d, scale, gq, w, gk, w, gv, w, bias, heads, gbias, heads);
    return HS_OK;
}

// ---- include/hisparse_heads_dropout.h: the same object, dropout on the attention weights, a bias or none --------------------------------
int hsmhd_forward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* bias_dev, uint64_t ldb,
                         uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout(p->num_rows, p->num_cols, p->max_heads, p->nnz(), q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, drop_p, y_dev,
                                                       ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    forward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, bias_dev, ldb, &dr);
    return HS_OK;
}

int hsmhd_forward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed,
                  uint64_t offset, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout_host(p->num_rows, p->num_cols, p->max_heads, p->nnz(), q, k, v, bias, heads, d, scale, drop_p, y, lse, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    forward(p, q, w, k, w, v, w, heads, d, scale, y, w, lse, heads, bias, heads, &dr);
    return HS_OK;
}

int hsmhd_backward_device(hsmh_pattern* p, const float* q_dev, uint64_t ldq, const float* k_dev, uint64_t ldk, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset,
                          float* gq_dev, uint64_t ldgq, float* gk_dev, uint64_t ldgk, float* gv_dev, uint64_t ldgv, float* gbias_dev, uint64_t ldgb) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz(), q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, bias_dev,
                                                        ldb, heads, d, scale, drop_p, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, gbias_dev, ldgb, why))
        return fail(p, rc, why);
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    backward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, bias_dev, ldb, gbias_dev, ldgb, &dr);
    return HS_OK;
}

int hsmhd_backward(hsmh_pattern* p, const float* q, const float* k, const float* v, const float* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d, float scale,
                   float drop_p, uint64_t seed, uint64_t offset, float* gq, float* gk, float* gv, float* gbias) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout_host(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz(), q, k, v, gy, lse, bias, heads, d, scale, drop_p, gq, gk, gv, gbias,
                                                             why))
        return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    backward(p, q, w, k, w, v, w, gy, w, lse, heads, heads, d, scale, gq, w, gk, w, gv, w, bias, heads, gbias, heads, &dr);
    return HS_OK;
}

int hsmhd_keep_mask(uint64_t nnz, uint32_t heads, float drop_p, uint64_t seed, uint64_t offset, uint8_t* keep) { return hisparse::hsmh::keep_mask(nnz, heads, drop_p, seed, offset, keep); }

// ---- include/hisparse_heads_dropout_bf16.h: the same object, bf16 operands, dropout on the attention weights, a bias or none -------------
int hsmhd16_forward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const float* bias_dev,
                           uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed, uint64_t offset, uint16_t* y_dev, uint64_t ldy, float* lse_dev,
                           uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout16(p->num_rows, p->num_cols, p->max_heads, p->nnz(), q_dev, ldq, k_dev, ldk, v_dev, ldv, bias_dev, ldb, heads, d, scale, drop_p,
                                                         y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    forward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, heads, d, scale, y_dev, ldy, lse_dev, ldl, bias_dev, ldb, &dr);
    return HS_OK;
}

int hsmhd16_forward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const float* bias, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed,
                    uint64_t offset, uint16_t* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_forward_dropout16_host(p->num_rows, p->num_cols, p->max_heads, p->nnz(), q, k, v, bias, heads, d, scale, drop_p, y, lse, why))
        return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    forward(p, q, w, k, w, v, w, heads, d, scale, y, w, lse, heads, bias, heads, &dr);
    return HS_OK;
}

int hsmhd16_backward_device(hsmh_pattern* p, const uint16_t* q_dev, uint64_t ldq, const uint16_t* k_dev, uint64_t ldk, const uint16_t* v_dev, uint64_t ldv, const uint16_t* gy_dev,
                            uint64_t ldgy, const float* lse_dev, uint64_t ldl, const float* bias_dev, uint64_t ldb, uint32_t heads, uint32_t d, float scale, float drop_p, uint64_t seed,
                            uint64_t offset, uint16_t* gq_dev, uint64_t ldgq, uint16_t* gk_dev, uint64_t ldgk, uint16_t* gv_dev, uint64_t ldgv, float* gbias_dev, uint64_t ldgb) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout16(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz(), q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl,
                                                          bias_dev, ldb, heads, d, scale, drop_p, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, gbias_dev, ldgb, why))
        return fail(p, rc, why);
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    backward(p, q_dev, ldq, k_dev, ldk, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, scale, gq_dev, ldgq, gk_dev, ldgk, gv_dev, ldgv, bias_dev, ldb, gbias_dev, ldgb, &dr);
    return HS_OK;
}

int hsmhd16_backward(hsmh_pattern* p, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* gy, const float* lse, const float* bias, uint32_t heads, uint32_t d,
                     float scale, float drop_p, uint64_t seed, uint64_t offset, uint16_t* gq, uint16_t* gk, uint16_t* gv, float* gbias) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_backward_dropout16_host(p->num_rows, p->num_cols, p->max_heads, p->map, p->nnz(), q, k, v, gy, lse, bias, heads, d, scale, drop_p, gq, gk, gv,
                                                               gbias, why))
        return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    const hisparse::philox::Dropout dr = hisparse::philox::dropout_of(drop_p, seed, offset);
    backward(p, q, w, k, w, v, w, gy, w, lse, heads, heads, d, scale, gq, w, gk, w, gv, w, bias, heads, gbias, heads, &dr);
    return HS_OK;
}

// ---- include/hisparse_gat.h: the same object, additive (GAT) scores from one word per node and head ----------------------------------
int hsgat_forward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, uint32_t heads, uint32_t d,
                         float slope, float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_forward(p->num_rows, p->num_cols, p->max_heads, el_dev, ldel, er_dev, lder, v_dev, ldv, heads, d, slope, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    gat_forward(p, el_dev, ldel, er_dev, lder, v_dev, ldv, heads, d, slope, y_dev, ldy, lse_dev, ldl);
    return HS_OK;
}

int hsgat_forward(hsmh_pattern* p, const float* el, const float* er, const float* v, uint32_t heads, uint32_t d, float slope, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_forward_host(p->num_rows, p->num_cols, p->max_heads, el, er, v, heads, d, slope, y, lse, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    gat_forward(p, el, heads, er, heads, v, w, heads, d, slope, y, w, lse, heads);
    return HS_OK;
}

int hsgat_backward_device(hsmh_pattern* p, const float* el_dev, uint64_t ldel, const float* er_dev, uint64_t lder, const float* v_dev, uint64_t ldv, const float* gy_dev, uint64_t ldgy,
                          const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gel_dev, uint64_t ldgel, float* ger_dev, uint64_t ldger, float* gv_dev,
                          uint64_t ldgv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_backward(p->num_rows, p->num_cols, p->max_heads, p->backward, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d,
                                                    slope, gel_dev, ldgel, ger_dev, ldger, gv_dev, ldgv, why))
        return fail(p, rc, why);
    gat_backward(p, el_dev, ldel, er_dev, lder, v_dev, ldv, gy_dev, ldgy, lse_dev, ldl, heads, d, slope, gel_dev, ldgel, ger_dev, ldger, gv_dev, ldgv);
    return HS_OK;
}

int hsgat_backward(hsmh_pattern* p, const float* el, const float* er, const float* v, const float* gy, const float* lse, uint32_t heads, uint32_t d, float slope, float* gel,
                   float* ger, float* gv) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat_backward_host(p->num_rows, p->num_cols, p->max_heads, p->backward, el, er, v, gy, lse, heads, d, slope, gel, ger, gv, why))
        return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    gat_backward(p, el, heads, er, heads, v, w, gy, w, lse, heads, heads, d, slope, gel, heads, ger, heads, gv, w);
    return HS_OK;
}

// ---- include/hisparse_gatv2.h: the same object, the score a . LeakyReLU(XD[row] + XS[col]) and the gradient of a ----------------------
int hsgat2_forward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev, uint32_t heads, uint32_t d, float slope,
                          float* y_dev, uint64_t ldy, float* lse_dev, uint64_t ldl) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_forward(p->num_rows, p->num_cols, p->max_heads, xd_dev, ldxd, xs_dev, ldxs, a_dev, heads, d, slope, y_dev, ldy, lse_dev, ldl, why))
        return fail(p, rc, why);
    gat2_forward(p, xd_dev, ldxd, xs_dev, ldxs, a_dev, heads, d, slope, y_dev, ldy, lse_dev, ldl);
    return HS_OK;
}

int hsgat2_forward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, uint32_t heads, uint32_t d, float slope, float* y, float* lse) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_forward_host(p->num_rows, p->num_cols, p->max_heads, xd, xs, a, heads, d, slope, y, lse, why)) return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    gat2_forward(p, xd, w, xs, w, a, heads, d, slope, y, w, lse, heads);
    return HS_OK;
}

// the sums of ga, heads * d doubles: this library adds the rows in order on one thread, so it keeps ONE vector
int hsgat2_work_bytes(const hsmh_pattern* p, uint32_t heads, uint32_t d, uint64_t* bytes) {
    if (!p || !bytes) return HS_ERR_BAD_ARG;
    std::string why;
    if (hisparse::hsmh::check_shape(heads, d, p->max_heads, why)) return HS_ERR_BAD_ARG;
    *bytes = uint64_t(heads) * d * 8;
    return HS_OK;
}

int hsgat2_backward_device(hsmh_pattern* p, const float* xd_dev, uint64_t ldxd, const float* xs_dev, uint64_t ldxs, const float* a_dev, const float* gy_dev, uint64_t ldgy,
                           const float* lse_dev, uint64_t ldl, uint32_t heads, uint32_t d, float slope, float* gxd_dev, uint64_t ldgxd, float* gxs_dev, uint64_t ldgxs, float* ga_dev,
                           void* work_dev, uint64_t work_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    uint64_t need = 0;
    (void)hsgat2_work_bytes(p, heads, d, &need);      // a bad shape leaves 0 and is refused by the checks below, with its reason
    if (int rc = hisparse::hsmh::check_gat2_backward(p->num_rows, p->num_cols, p->max_heads, p->backward, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, heads, d, slope,
                                                     gxd_dev, ldgxd, gxs_dev, ldgxs, ga_dev, work_dev, work_bytes, need, why))
        return fail(p, rc, why);
    gat2_backward(p, xd_dev, ldxd, xs_dev, ldxs, a_dev, gy_dev, ldgy, lse_dev, ldl, heads, d, slope, gxd_dev, ldgxd, gxs_dev, ldgxs, ga_dev, static_cast<double*>(work_dev));
    return HS_OK;
}

int hsgat2_backward(hsmh_pattern* p, const float* xd, const float* xs, const float* a, const float* gy, const float* lse, uint32_t heads, uint32_t d, float slope, float* gxd,
                    float* gxs, float* ga) {
    if (!p) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsmh::check_gat2_backward_host(p->num_rows, p->num_cols, p->max_heads, p->backward, xd, xs, a, gy, lse, heads, d, slope, gxd, gxs, ga, why))
        return fail(p, rc, why);
    const uint64_t w = uint64_t(heads) * d;
    std::vector<double> work(w);      // the host form's own transient
    gat2_backward(p, xd, w, xs, w, a, gy, w, lse, heads, heads, d, slope, gxd, w, gxs, w, ga, work.data());
    return HS_OK;
}

}  // extern "C"
