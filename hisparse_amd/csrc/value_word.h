// value_word.h — the device conversion of a CSR float into the value word the images hold: csr_matrix_convert_from_float
// (sw/data_loader.h:76-84).  Float modes: the float's bits.  Fixed point: the Q8.24 conversion of include/hisparse/q8_24.h (negatives,
// zeros and NaN -> 0; round half up; saturate), all exact in double, so bit-identical to the host.  The ONE device definition: the load-time
// builder (gpu_tiles.hip) and the value update (value_update.hip, hs_update_values) both include it, so an update writes the bytes a
// fresh load of the same values writes.
#ifndef HISPARSE_VALUE_WORD_H_
#define HISPARSE_VALUE_WORD_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hisparse {
namespace dev {

__device__ __forceinline__ uint32_t value_word(float v, bool fixed) {
    if (!fixed) return __float_as_uint(v);
    const double d = double(v);
    if (!(d > 0.0)) return 0u;
    const double scaled = floor(d * 16777216.0 + 0.5);
    return scaled >= 4294967296.0 ? 0xffffffffu : uint32_t(scaled);
}

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_VALUE_WORD_H_
