// philox.h — the counter-based generator behind the keep decision of attention dropout (include/hisparse_heads_dropout.h): Philox4x32-10
// with the standard constants, and keep(e, h) as that header fixes it.  Plain C++ inline functions for host and device code alike
// (hsmh_cpu.cpp, hsmh_api.cpp's hsmhd_keep_mask and the kernels of heads_dropout_attention.hip call the same text); integer arithmetic
// only, no state, no tables, no inline assembly.  One call yields the four words of (entry e, heads 4 (h >> 2) ... 4 (h >> 2) + 3).
#ifndef HISPARSE_PHILOX_H_
#define HISPARSE_PHILOX_H_

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HISPARSE_PHILOX_FN __host__ __device__ __forceinline__      // inlined into the kernels: a call would take the address of its arguments
#else
#define HISPARSE_PHILOX_FN inline
#endif

namespace hisparse {
namespace philox {

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;      // the round multipliers
constexpr uint32_t kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;      // the key increments
constexpr uint32_t kRounds = 10;

// four 32-bit words, named (an indexed array in a kernel would be scratch)
struct Words {
    uint32_t a, b, c, d;
};

// the ten rounds in place, on scalars (a kernel keeps them in registers)
HISPARSE_PHILOX_FN void rounds(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t p0 = uint64_t(kMul0) * c0, p1 = uint64_t(kMul1) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c1 = uint32_t(p1);
        c3 = uint32_t(p0);
        c0 = n0;
        c2 = n2;
        k0 += kKey0;
        k1 += kKey1;
    }
}

// Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1)
HISPARSE_PHILOX_FN Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    rounds(c0, c1, c2, c3, k0, k1);
    return Words{c0, c1, c2, c3};
}

// What a call with dropout carries into its loops or its kernels: the key, the two offset words of the counter, the threshold and
// c = 1 / (1 - drop_p), formed in double.  drop_p is finite and in [0, 1) (hsmh_common.h checks it before this is built).
struct Dropout {
    uint32_t key0, key1, off0, off1, thr;
    double c;
};

HISPARSE_PHILOX_FN uint32_t threshold(float drop_p) { return uint32_t(double(drop_p) * 4294967296.0); }      // floor: the product is exact and below 2^32

HISPARSE_PHILOX_FN Dropout dropout_of(float drop_p, uint64_t seed, uint64_t offset) {
    return Dropout{uint32_t(seed), uint32_t(seed >> 32), uint32_t(offset), uint32_t(offset >> 32), threshold(drop_p), 1.0 / (1.0 - double(drop_p))};
}

// x(e, h): word (h & 3) of the draw of entry e (its index in the caller's CSR order) and the heads 4 (h >> 2) ... 4 (h >> 2) + 3, selected
// by value
HISPARSE_PHILOX_FN uint32_t word(const Dropout& dr, uint32_t e, uint32_t h) {
    uint32_t c0 = e, c1 = h >> 2, c2 = dr.off0, c3 = dr.off1;
    rounds(c0, c1, c2, c3, dr.key0, dr.key1);
    const uint32_t lo = (h & 1u) ? c1 : c0, hi = (h & 1u) ? c3 : c2;
    return (h & 2u) ? hi : lo;
}

// keep(e, h) = x(e, h) >= thr
HISPARSE_PHILOX_FN bool keep(const Dropout& dr, uint32_t e, uint32_t h) { return word(dr, e, h) >= dr.thr; }

}  // namespace philox
}  // namespace hisparse

#endif  // HISPARSE_PHILOX_H_
