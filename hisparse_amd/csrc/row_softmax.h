// row_softmax.h — schedule constants and launchers of the row softmax's kernels (row_softmax.hip), called by hsr_api.cpp.
#ifndef HISPARSE_ROW_SOFTMAX_H_
#define HISPARSE_ROW_SOFTMAX_H_

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace hisparse {
namespace dev {

// Launch geometry (as sddmm.h): workgroups of kRowsThreads lanes, the grid never exceeds compute_units * kRowsBlocksPerCu of them and
// strides over the schedule's virtual workgroups from there.  A lane of a group class holds kRowsPerLane scores; a row longer than
// kRowsLong entries is a long row.  hisparse_amd/rows.py restates the four numbers (tests assert that a pattern is larger than two
// trips of the grid from them).
constexpr uint32_t kRowsThreads = 256;
constexpr uint32_t kRowsBlocksPerCu = 8;
constexpr uint32_t kRowsPerLane = 4;
constexpr uint32_t kRowsLong = 256;

// Classes: 0 holds the long rows, 1 ... 5 are the group classes of G = 4 << (c - 1) lanes per row (the smallest G with n <= kRowsPerLane * G).
// Virtual workgroups are laid out in class order, so the long rows -- the most expensive items -- are started first and the short rows
// fill in beside them.
constexpr uint32_t kRowsClasses = 6;
inline uint32_t rows_class_of(uint32_t n) {      // n >= 1
    if (n > kRowsLong) return 0;
    uint32_t c = 1;
    while (n > (kRowsPerLane * 4u << (c - 1))) ++c;
    return c;
}
// rows one virtual workgroup of class c serves
inline uint32_t rows_per_workgroup(uint32_t c) { return c ? kRowsThreads / (4u << (c - 1)) : 1u; }

// The table in device memory, kRowsTableWords words: [c] = the first virtual workgroup of class c (c = 0 ... 5), [6] = all virtual
// workgroups; [8 + c] = where class c starts in the row list, [14] = the length of the list (the non-empty rows); [7], [15] zero.
constexpr uint32_t kRowsTableWords = 16;

struct RowSoftmaxLaunch {
    const uint32_t* indptr = nullptr;      // device: num_rows + 1 words
    const uint32_t* list = nullptr;        // device: the non-empty rows, class by class
    const uint32_t* table = nullptr;       // device: kRowsTableWords words
    uint32_t workgroups = 0;               // table[6]
    uint32_t compute_units = 0;
};
// p = softmax_row(scale * s); p == s is in place
hipError_t launch_row_softmax(const RowSoftmaxLaunch& a, const float* s, float scale, float* p, hipStream_t stream);
// gs = scale * p * (gp - sum_row p gp); gs == gp is in place
hipError_t launch_row_softmax_backward(const RowSoftmaxLaunch& a, const float* p, const float* gp, float scale, float* gs, hipStream_t stream);

}  // namespace dev
}  // namespace hisparse

#endif  // HISPARSE_ROW_SOFTMAX_H_
