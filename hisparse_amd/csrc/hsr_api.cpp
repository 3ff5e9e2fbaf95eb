// hsr_api.cpp — include/hisparse_rows.h on the HIP runtime: the rows object of the row softmax.  One object owns one device, one stream of
// its own and, from hsr_create on, all the device memory its _device calls will ever use (device_buffer.h): indptr, the non-empty rows
// sorted into length classes and the 16-word table that maps virtual workgroups to classes (row_softmax.h).  The schedule is built here,
// on the host, from indptr; the kernels are in row_softmax.hip; what the object shares with the pattern objects, and the host forms'
// transient buffers, are pattern_object.h's.  Nothing here touches a context, a pattern or a numeric mode.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "hsr_common.h"
#include "pattern_object.h"
#include "row_softmax.h"

using namespace hisparse::obj;

struct hsr_rows : PatternObject {
    uint32_t num_rows = 0;
    uint32_t compute_units = 0;
    uint32_t workgroups = 0;      // virtual workgroups of the schedule
    DeviceBuffer<uint32_t> indptr, list, table;
};

namespace {

using namespace hisparse::dev;

// the non-empty rows class by class and the table of row_softmax.h; the long rows (class 0, started first) longest first, the others ascending
void schedule(uint32_t num_rows, const uint32_t* indptr, std::vector<uint32_t>& list, uint32_t (&table)[kRowsTableWords]) {
    uint32_t count[kRowsClasses] = {};
    for (uint32_t r = 0; r < num_rows; ++r)
        if (const uint32_t n = indptr[r + 1] - indptr[r]) ++count[rows_class_of(n)];
    std::memset(table, 0, sizeof table);
    uint32_t next[kRowsClasses];
    for (uint32_t c = 0; c < kRowsClasses; ++c) {
        const uint32_t per = rows_per_workgroup(c);
        next[c] = table[8 + c];
        table[c + 1] = table[c] + (count[c] + per - 1) / per;      // [6]: all of them
        table[8 + c + 1] = table[8 + c] + count[c];                // [14]: the non-empty rows
    }
    list.resize(table[8 + kRowsClasses]);
    for (uint32_t r = 0; r < num_rows; ++r)
        if (const uint32_t n = indptr[r + 1] - indptr[r]) list[next[rows_class_of(n)]++] = r;
    std::stable_sort(list.begin(), list.begin() + count[0], [&](uint32_t a, uint32_t b) { return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b]; });
}

// everything hsr_create does on the device; the caller destroys r when this fails
int build(hsr_rows* r, const uint32_t* indptr) {
    std::vector<uint32_t> list;
    uint32_t table[kRowsTableWords];
    schedule(r->num_rows, indptr, list, table);
    r->workgroups = table[kRowsClasses];
    if (int rc = open_stream(r)) return rc;
    const size_t indptr_bytes = (size_t(r->num_rows) + 1) * 4, list_bytes = std::max<size_t>(list.size(), 1) * 4, table_bytes = kRowsTableWords * 4;
    HS_HIP(r, r->indptr.alloc(indptr_bytes));
    HS_HIP(r, r->list.alloc(list_bytes));
    HS_HIP(r, r->table.alloc(table_bytes));
    r->device_bytes = indptr_bytes + list_bytes + table_bytes;
    HS_HIP(r, hipMemcpyAsync(r->indptr.get(), indptr, indptr_bytes, hipMemcpyHostToDevice, r->own_stream));
    if (!list.empty()) HS_HIP(r, hipMemcpyAsync(r->list.get(), list.data(), list.size() * 4, hipMemcpyHostToDevice, r->own_stream));
    HS_HIP(r, hipMemcpyAsync(r->table.get(), table, table_bytes, hipMemcpyHostToDevice, r->own_stream));
    HS_HIP(r, hipStreamSynchronize(r->own_stream));      // the caller's array, list and table are free again
    return HS_OK;
}

RowSoftmaxLaunch launch_of(const hsr_rows* r) {
    RowSoftmaxLaunch a;
    a.indptr = r->indptr.get();
    a.list = r->list.get();
    a.table = r->table.get();
    a.workgroups = r->workgroups;
    a.compute_units = r->compute_units;
    return a;
}

}  // namespace

extern "C" {

int hsr_create(hsr_rows** out, int device_id, uint32_t num_rows, const uint32_t* indptr) {
    if (!out) return fail<hsr_rows>(nullptr, HS_ERR_BAD_ARG, "null rows pointer");
    *out = nullptr;
    std::string why;
    hipDeviceProp_t prop;
    if (int rc = hisparse::hsr::check_rows(num_rows, indptr, why)) return fail<hsr_rows>(nullptr, rc, why);
    if (int rc = probe_device(device_id, prop, why)) return fail<hsr_rows>(nullptr, rc, why);
    hsr_rows* r = new (std::nothrow) hsr_rows;
    if (!r) return fail<hsr_rows>(nullptr, HS_ERR_NO_MEMORY, "out of memory");
    r->device = device_id;
    r->num_rows = num_rows;
    r->nnz = indptr[num_rows];
    r->compute_units = uint32_t(prop.multiProcessorCount);
    return finish_create(out, r, build(r, indptr));
}

int hsr_destroy(hsr_rows* r) { return destroy(r); }
const char* hsr_last_error(const hsr_rows* r) { return last_error(r); }
int hsr_info(const hsr_rows* r, uint64_t* nnz, uint64_t* device_bytes) { return info(r, nnz, device_bytes); }
int hsr_set_stream(hsr_rows* r, void* hip_stream) { return set_stream(r, hip_stream); }
int hsr_sync(hsr_rows* r) { return sync(r); }

int hsr_softmax_device(hsr_rows* r, const float* s_dev, float scale, float* p_dev) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_forward(r->nnz, s_dev, scale, p_dev, true, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    HS_HIP(r, launch_row_softmax(launch_of(r), s_dev, scale, p_dev, r->stream));
    return HS_OK;
}

int hsr_softmax_backward_device(hsr_rows* r, const float* p_dev, const float* gp_dev, float scale, float* gs_dev) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_backward(r->nnz, p_dev, gp_dev, scale, gs_dev, true, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    HS_HIP(r, launch_row_softmax_backward(launch_of(r), p_dev, gp_dev, scale, gs_dev, r->stream));
    return HS_OK;
}

int hsr_softmax(hsr_rows* r, const float* s, float scale, float* p) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_forward(r->nnz, s, scale, p, false, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    Staging st(r);
    float* d = st.inout(s, p, 1, r->nnz, r->nnz);      // the kernel runs in place, over the copy of s
    return st.finish(st.failed() ? st.failed() : hsr_softmax_device(r, d, scale, d));
}

int hsr_softmax_backward(hsr_rows* r, const float* p, const float* gp, float scale, float* gs) {
    if (!r) return HS_ERR_BAD_ARG;
    std::string why;
    if (int rc = hisparse::hsr::check_backward(r->nnz, p, gp, scale, gs, false, why)) return fail(r, rc, why);
    if (int rc = enter(r)) return rc;
    Staging st(r);
    const float* d_p = st.in(p, 1, r->nnz, r->nnz);
    float* d_g = st.inout(gp, gs, 1, r->nnz, r->nnz);      // the gradient is written over gp's copy
    return st.finish(st.failed() ? st.failed() : hsr_softmax_backward_device(r, d_p, d_g, scale, d_g));
}

}  // extern "C"
