// wide_schedule.h — the host side of the row schedule of wide_products.h: the sort of a pattern's rows into length classes, done once at
// create time by every object whose kernels use that schedule (hsw_, hsat_, hsab_ and hsmh_api.cpp), and the upload of one side of a
// pattern with it.  Host code only.
#ifndef HISPARSE_WIDE_SCHEDULE_H_
#define HISPARSE_WIDE_SCHEDULE_H_

#include <algorithm>
#include <cstdint>
#include <vector>

#include "pattern_object.h"
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

// one side of a pattern on the device: WideSide's arrays and their owner (view.compute_units is the creator's to set)
struct WideSideBuffers {
    DeviceBuffer<uint32_t> ptr, idx, perm, list;
    WideSide view;
};

// One side's arrays onto the device of p, on its own stream, and into p->device_bytes: `rows` + 1 words of ptr, p->nnz of idx and, where
// `mapped`, as many of perm.  Waits: the host arrays are free again on return.
inline int upload_side(obj::PatternObject* p, WideSideBuffers& s, uint32_t rows, const uint32_t* ptr, const uint32_t* idx, bool mapped, const uint32_t* perm) {
    std::vector<uint32_t> list;
    schedule(rows, ptr, list, s.view.count);
    const size_t ptr_bytes = (size_t(rows) + 1) * 4, entry_bytes = std::max<size_t>(size_t(p->nnz), 1) * 4, list_bytes = size_t(rows) * 4;
    HS_HIP(p, s.ptr.alloc(ptr_bytes));
    HS_HIP(p, s.idx.alloc(entry_bytes));
    HS_HIP(p, s.list.alloc(list_bytes));
    p->device_bytes += ptr_bytes + entry_bytes + list_bytes;
    HS_HIP(p, hipMemcpyAsync(s.ptr.get(), ptr, ptr_bytes, hipMemcpyHostToDevice, p->own_stream));
    HS_HIP(p, hipMemcpyAsync(s.list.get(), list.data(), list_bytes, hipMemcpyHostToDevice, p->own_stream));
    if (p->nnz) HS_HIP(p, hipMemcpyAsync(s.idx.get(), idx, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    if (mapped) {
        HS_HIP(p, s.perm.alloc(entry_bytes));
        p->device_bytes += entry_bytes;
        if (p->nnz) HS_HIP(p, hipMemcpyAsync(s.perm.get(), perm, size_t(p->nnz) * 4, hipMemcpyHostToDevice, p->own_stream));
    }
    HS_HIP(p, hipStreamSynchronize(p->own_stream));
    s.view.ptr = s.ptr.get();
    s.view.idx = s.idx.get();
    s.view.perm = s.perm.get();
    s.view.list = s.list.get();
    s.view.entries = p->nnz;
    return HS_OK;
}

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_WIDE_SCHEDULE_H_
