// wide_schedule.h — the host side of the row schedule of wide_products.h: the sort of a pattern's rows into length classes, done once at
// create time by every object whose kernels use that schedule (hsw_api.cpp, hsat_api.cpp).  Host code only.
#ifndef HISPARSE_WIDE_SCHEDULE_H_
#define HISPARSE_WIDE_SCHEDULE_H_

#include <algorithm>
#include <cstdint>
#include <vector>

#include "wide_products.h"

namespace hisparse {
namespace dev {

// every row class by class (wide_products.h); the long rows (class 0, started first) longest first, the others ascending
inline void schedule(uint32_t rows, const uint32_t* ptr, std::vector<uint32_t>& list, uint32_t (&count)[kWideClasses]) {
    std::fill(count, count + kWideClasses, 0u);
    for (uint32_t r = 0; r < rows; ++r) ++count[wide_class_of(ptr[r + 1] - ptr[r])];
    uint32_t next[kWideClasses];
    for (uint32_t c = 0, at = 0; c < kWideClasses; at += count[c++]) next[c] = at;
    list.resize(rows);
    for (uint32_t r = 0; r < rows; ++r) list[next[wide_class_of(ptr[r + 1] - ptr[r])]++] = r;
    std::stable_sort(list.begin(), list.begin() + count[0], [&](uint32_t a, uint32_t b) { return ptr[a + 1] - ptr[a] > ptr[b + 1] - ptr[b]; });
}

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_WIDE_SCHEDULE_H_
