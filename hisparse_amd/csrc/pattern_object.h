// pattern_object.h — what the objects of the pattern C ABIs share on the host (hsp_, hsr_, hsw_, hsat_, hsab_ and hsmh_api.cpp): the
// members every object has, its error record, the device probe of a create call, the bodies of destroy / last_error / info / set_stream /
// sync, and Staging, the owner of a host form's transient device buffers.  HIP runtime API only, no kernels.  The calls are templates on
// the object's own type P (a struct derived from PatternObject): that type is what keeps one family's create-time error text apart from
// another's, and what destroy deletes.
#ifndef HISPARSE_PATTERN_OBJECT_H_
#define HISPARSE_PATTERN_OBJECT_H_

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "device_buffer.h"
#include "hisparse_hip.h"

namespace hisparse {
namespace obj {

struct PatternObject {
    int device = 0;
    uint64_t nnz = 0;
    uint64_t device_bytes = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;      // own_stream, or the caller's (set_stream)
    std::string error;
};

// why the last create call of P's family failed on this thread
template <class P>
std::string& create_error() {
    thread_local std::string text;
    return text;
}

// records msg for last_error (p == nullptr: the creating thread's, fail<P>(nullptr, ...)), returns code
template <class P>
int fail(P* p, int code, const std::string& msg) {
    (p ? p->error : create_error<P>()) = msg;
    return code;
}
template <class P>
int hip_fail(P* p, hipError_t e, const char* what) {
    return fail(p, HS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HS_HIP(p, call)                                                      \
    do {                                                                     \
        const hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return hisparse::obj::hip_fail((p), e_, #call); \
    } while (0)

// the way into a call that touches the device
template <class P>
int enter(P* p) {
    if (!p) return HS_ERR_BAD_ARG;
    HS_HIP(p, hipSetDevice(p->device));
    return HS_OK;
}

// a create call's look at the device: it exists, and it is the one this library carries code for
inline int probe_device(int device_id, hipDeviceProp_t& prop, std::string& why) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        why = "no HIP device visible (this library has no CPU fallback)";
        return HS_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= count) {
        why = "device_id out of range";
        return HS_ERR_BAD_ARG;
    }
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) {
        why = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return HS_ERR_HIP;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        why = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only";
        return HS_ERR_NO_DEVICE;
    }
    return HS_OK;
}

// the first step of every build(): the object's device and a stream of its own
template <class P>
int open_stream(P* p) {
    HS_HIP(p, hipSetDevice(p->device));
    HS_HIP(p, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    p->stream = p->own_stream;
    return HS_OK;
}

// the end of a create call: hands p out when build() returned HS_OK, otherwise keeps its reason for last_error(NULL) and takes it down
template <class P>
int finish_create(P** out, P* p, int rc) {
    if (rc == HS_OK) {
        *out = p;
        return HS_OK;
    }
    create_error<P>() = p->error;
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    delete p;
    return rc;
}

template <class P>
int destroy(P* p) {
    if (!p) return HS_OK;
    (void)hipSetDevice(p->device);
    // only the object's own stream is known to be alive; a caller-owned stream must have been synchronised by its owner
    if (p->own_stream) {
        (void)hipStreamSynchronize(p->own_stream);
        (void)hipStreamDestroy(p->own_stream);
    }
    delete p;
    return HS_OK;
}

template <class P>
const char* last_error(const P* p) {
    return p ? p->error.c_str() : create_error<P>().c_str();
}

inline int info(const PatternObject* p, uint64_t* nnz, uint64_t* device_bytes) {
    if (!p) return HS_ERR_BAD_ARG;
    if (nnz) *nnz = p->nnz;
    if (device_bytes) *device_bytes = p->device_bytes;
    return HS_OK;
}

inline int set_stream(PatternObject* p, void* hip_stream) {
    if (!p) return HS_ERR_BAD_ARG;
    p->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : p->own_stream;
    return HS_OK;
}

template <class P>
int sync(P* p) {
    if (int rc = enter(p)) return rc;
    HS_HIP(p, hipStreamSynchronize(p->stream));
    return HS_OK;
}

// The transient device buffers of one host-form call, on the object's current stream (the host forms are synchronous and may allocate).
// in() and out() take `rows` rows of `words` elements, tight in the caller's array and `ld` elements apart on the device; each buffer is
// max(rows * ld elements, floor) bytes, so with the default floor its pointer is never null.  A null host pointer stands for an optional
// operand the caller left out: a null device pointer, no memory.  The first failure sticks: every later in / out / scratch does nothing
// and returns nullptr, failed() is its code and finish() returns it.  Staging never frees a buffer the stream may still use: finish()
// always waits, and so does the destructor when finish() was not reached.
class Staging {
public:
    explicit Staging(PatternObject* p) : p_(p), stream_(p->stream) {}
    ~Staging() {
        if (!finished_) (void)hipStreamSynchronize(stream_);
    }
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;

    template <class T>
    T* in(const T* host, size_t rows, size_t words, size_t ld, size_t floor = 16) {
        return host ? static_cast<T*>(stage(host, nullptr, rows, words * sizeof(T), ld * sizeof(T), floor)) : nullptr;
    }
    template <class T>
    T* out(T* host, size_t rows, size_t words, size_t ld, size_t floor = 16) {
        return host ? static_cast<T*>(stage(nullptr, host, rows, words * sizeof(T), ld * sizeof(T), floor)) : nullptr;
    }
    // one buffer that is copied in from `from` and, after the call, out to `to` (a kernel that runs in place)
    template <class T>
    T* inout(const T* from, T* to, size_t rows, size_t words, size_t ld, size_t floor = 16) {
        return static_cast<T*>(stage(from, to, rows, words * sizeof(T), ld * sizeof(T), floor));
    }
    // device memory that is neither copied in nor out
    void* scratch(size_t bytes, size_t floor = 16) { return stage(nullptr, nullptr, 1, 0, bytes, floor); }

    int failed() const { return rc_; }

    // rc: what the _device form returned.  The copies out (in the order of their out() calls, none of an empty array) when all went well,
    // then the wait, whatever happened; the first error is the result.
    int finish(int rc) {
        if (rc_ != HS_OK) rc = rc_;
        for (size_t i = 0; rc == HS_OK && i < outs_.size(); ++i) {
            const Out& o = outs_[i];
            const hipError_t e = copy(o.host, o.row_bytes, o.dev, o.pitch, o.row_bytes, o.rows, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = hip_fail(p_, e, "copying the result out");
        }
        finished_ = true;
        const hipError_t e = hipStreamSynchronize(stream_);
        if (rc == HS_OK && e != hipSuccess) rc = hip_fail(p_, e, "hipStreamSynchronize");
        return rc;
    }

private:
    struct Out {
        void* host;
        const void* dev;
        size_t rows, row_bytes, pitch;
    };

    // rows of row_bytes, `pitch` bytes apart on the device: one linear copy when that is the same thing
    hipError_t copy(void* dst, size_t dpitch, const void* src, size_t spitch, size_t row_bytes, size_t rows, hipMemcpyKind kind) {
        if (rows == 0 || row_bytes == 0) return hipSuccess;
        if (rows == 1 || (dpitch == row_bytes && spitch == row_bytes)) return hipMemcpyAsync(dst, src, rows * row_bytes, kind, stream_);
        return hipMemcpy2DAsync(dst, dpitch, src, spitch, row_bytes, rows, kind, stream_);
    }

    void* stage(const void* from, void* to, size_t rows, size_t row_bytes, size_t pitch, size_t floor) {
        if (rc_ != HS_OK) return nullptr;
        buffers_.emplace_back();
        hipError_t e = buffers_.back().alloc(std::max(rows * pitch, floor));
        if (e != hipSuccess) {
            rc_ = hip_fail(p_, e, "allocating a host form's buffer");
            return nullptr;
        }
        void* dev = buffers_.back().get();
        if (from && (e = copy(dev, pitch, from, row_bytes, row_bytes, rows, hipMemcpyHostToDevice)) != hipSuccess) {
            rc_ = hip_fail(p_, e, "copying an operand in");
            return nullptr;
        }
        if (to) outs_.push_back(Out{to, dev, rows, row_bytes, pitch});
        return dev;
    }

    PatternObject* p_;
    hipStream_t stream_;
    int rc_ = HS_OK;
    bool finished_ = false;
    std::vector<Out> outs_;
    std::vector<DeviceBuffer<unsigned char>> buffers_;      // freed as members go, after the destructor's body (and its wait)
};

}  // namespace obj
}  // namespace hisparse

#endif  // HISPARSE_PATTERN_OBJECT_H_
