// What the pattern objects share on the host (hisparse_amd/csrc/pattern_object.h: Staging and the object base) over a fake HIP runtime
// defined here: "device" memory is host memory, every runtime call is logged in order, and the n-th call of a kind can be made to fail.
// No GPU, no HIP runtime linked; meant to be built with -fsanitize=address,undefined, which then checks every copy's bounds.
#undef NDEBUG
#include "pattern_object.h"

#include <cassert>
#include <cstdlib>
#include <iostream>
#include <set>
#include <string>
#include <vector>

using namespace hisparse::obj;

// ---- the fake runtime --------------------------------------------------------------------------------------------------------------------
namespace {

enum Kind { kMalloc, kFree, kCopy, kCopy2D, kSync, kStreamDestroy, kKinds };
struct Event {
    Kind kind;
    const void* ptr;             // the allocation, or the copy's destination
    hipMemcpyKind direction;
};
std::vector<Event> g_log;
std::set<void*> g_live;          // allocations not yet freed
int g_calls[kKinds];             // calls so far, per knob (the two copy forms count together, under kCopy)
int g_fail_at[kKinds];           // the call of that knob that fails; -1: none

void reset_runtime() {
    assert(g_live.empty());
    g_log.clear();
    for (int k = 0; k < kKinds; ++k) g_calls[k] = 0, g_fail_at[k] = -1;
}
bool failing(Kind k) { return g_calls[k]++ == g_fail_at[k]; }
int logged(Kind k) {
    int n = 0;
    for (const Event& e : g_log) n += e.kind == k;
    return n;
}
int copies(hipMemcpyKind direction) {
    int n = 0;
    for (const Event& e : g_log) n += (e.kind == kCopy || e.kind == kCopy2D) && e.direction == direction;
    return n;
}
// in the log, nothing is freed while a copy may still be in flight: a synchronise stands between the last copy and the first free
bool waited_before_freeing() {
    bool in_flight = false;
    for (const Event& e : g_log) {
        if (e.kind == kCopy || e.kind == kCopy2D) in_flight = true;
        if (e.kind == kSync) in_flight = false;
        if (e.kind == kFree && in_flight) return false;
    }
    return true;
}

}  // namespace

extern "C" {

hipError_t hipMalloc(void** ptr, size_t size) {
    if (failing(kMalloc)) return hipErrorOutOfMemory;
    *ptr = size ? std::malloc(size) : nullptr;
    if (*ptr) g_live.insert(*ptr);
    g_log.push_back({kMalloc, *ptr, hipMemcpyDefault});
    return hipSuccess;
}
hipError_t hipFree(void* ptr) {
    assert(g_live.erase(ptr) == 1);      // freed once, and only what was allocated
    g_log.push_back({kFree, ptr, hipMemcpyDefault});
    std::free(ptr);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    if (failing(kCopy)) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    g_log.push_back({kCopy, dst, kind});
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t) {
    if (failing(kCopy)) return hipErrorInvalidValue;
    for (size_t r = 0; r < height; ++r) std::memcpy(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, width);
    g_log.push_back({kCopy2D, dst, kind});
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    g_log.push_back({kSync, stream, hipMemcpyDefault});
    return failing(kSync) ? hipErrorUnknown : hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
    g_log.push_back({kStreamDestroy, stream, hipMemcpyDefault});
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "a failure of the fake runtime"; }

}  // extern "C"

// ---- two families of objects ---------------------------------------------------------------------------------------------------------------
namespace {

struct Apple : PatternObject {};
struct Pear : PatternObject {};

hipStream_t stream_of(uintptr_t n) { return reinterpret_cast<hipStream_t>(n); }

Apple make_object(uint64_t nnz) {
    Apple a;
    a.nnz = nnz;
    a.own_stream = a.stream = stream_of(0x10);
    return a;
}

// A host form with 3 inputs and 2 outputs, as the API files write them: rows x words, ld apart on the device.  The "_device form" adds
// the three inputs into y and sums every row of a into z.
const size_t kRows = 3, kWords = 5;
int form(Apple* p, size_t ld, const float* a, const float* b, const float* c, float* y, float* z, int device_rc = HS_OK) {
    Staging st(p);
    const float* d_a = st.in(a, kRows, kWords, ld);
    const float* d_b = st.in(b, kRows, kWords, ld);
    const float* d_c = st.in(c, kRows, kWords, ld);
    float* d_y = st.out(y, kRows, kWords, ld);
    float* d_z = st.out(z, kRows, 1, 1);
    if (st.failed()) return st.finish(st.failed());
    for (size_t r = 0; r < kRows; ++r) {
        d_z[r] = 0;
        for (size_t j = 0; j < kWords; ++j) d_y[r * ld + j] = d_a[r * ld + j] + d_b[r * ld + j] + d_c[r * ld + j], d_z[r] += d_a[r * ld + j];
    }
    return st.finish(device_rc);
}

struct Operands {
    float a[kRows * kWords], b[kRows * kWords], c[kRows * kWords];
    float y[kRows * kWords + 2], z[kRows + 2];      // two words more than the form writes: they must stay as they are
    Operands() {
        for (size_t i = 0; i < kRows * kWords; ++i) a[i] = float(i), b[i] = float(100 + i), c[i] = float(1000 * i);
        for (float& v : y) v = -1;
        for (float& v : z) v = -1;
    }
    bool results_written() const {
        for (size_t i = 0; i < kRows * kWords; ++i)
            if (y[i] != a[i] + b[i] + c[i]) return false;
        for (size_t r = 0; r < kRows; ++r) {
            float sum = 0;
            for (size_t j = 0; j < kWords; ++j) sum += a[r * kWords + j];
            if (z[r] != sum) return false;
        }
        return tail_untouched();
    }
    bool results_untouched() const {
        for (float v : y)
            if (v != -1) return false;
        for (float v : z)
            if (v != -1) return false;
        return true;
    }
    bool tail_untouched() const { return y[kRows * kWords] == -1 && y[kRows * kWords + 1] == -1 && z[kRows] == -1 && z[kRows + 1] == -1; }
};

void test_round_trips() {
    // ld = 8: every copy of a dense operand is the 2D form (z, one word per row, is linear); ld = words: all linear
    for (size_t ld : {size_t(8), kWords}) {
        reset_runtime();
        Apple p = make_object(7);
        Operands o;
        assert(form(&p, ld, o.a, o.b, o.c, o.y, o.z) == HS_OK && p.error.empty());
        assert(o.results_written());
        assert(logged(kMalloc) == 5 && logged(kFree) == 5 && logged(kSync) == 1 && waited_before_freeing());
        assert(copies(hipMemcpyHostToDevice) == 3 && copies(hipMemcpyDeviceToHost) == 2);
        assert(logged(kCopy2D) == (ld == kWords ? 0 : 4));
        // the copies out come in the order of the out() calls, after every copy in
        std::vector<const void*> to;
        for (const Event& e : g_log)
            if ((e.kind == kCopy || e.kind == kCopy2D) && e.direction == hipMemcpyDeviceToHost) to.push_back(e.ptr);
        assert(to.size() == 2 && to[0] == o.y && to[1] == o.z);
    }
}

void test_nothing_to_copy() {
    // zero rows, and the per-entry arrays of an object without entries: a pointer all the same (the 16-byte floor), no copy, one wait
    reset_runtime();
    Apple p = make_object(0);
    float host[4] = {1, 2, 3, 4};
    {
        Staging st(&p);
        assert(st.in(host, 0, 5, 8) != nullptr);
        assert(st.in(host, p.nnz, 4, 4) != nullptr);
        assert(st.out(host, 0, 5, 8) != nullptr);
        assert(st.out(host, p.nnz, 4, 4) != nullptr);
        assert(st.scratch(0) != nullptr);
        assert(st.finish(HS_OK) == HS_OK);
    }
    assert(logged(kMalloc) == 5 && logged(kFree) == 5 && logged(kCopy) + logged(kCopy2D) == 0 && logged(kSync) == 1);
    assert(host[0] == 1 && host[3] == 4);
    // floor 0: as many bytes as the operand has, nothing for none
    reset_runtime();
    {
        Staging st(&p);
        assert(st.in(host, 0, 4, 4, 0) == nullptr && st.failed() == HS_OK);
        assert(st.finish(HS_OK) == HS_OK);
    }
    assert(logged(kFree) == 0 && logged(kSync) == 1);
}

void test_optional_operands() {
    reset_runtime();
    Apple p = make_object(7);
    {
        Staging st(&p);
        assert(st.in(static_cast<const float*>(nullptr), 3, 5, 8) == nullptr);
        assert(st.out(static_cast<float*>(nullptr), 3, 5, 8) == nullptr);
        assert(st.failed() == HS_OK && st.finish(HS_OK) == HS_OK);
    }
    assert(logged(kMalloc) == 0 && logged(kCopy) + logged(kCopy2D) == 0 && logged(kSync) == 1);
}

void test_refused_device_call() {
    // the _device form refused: nothing is copied out, the wait happens, the code comes back as it is
    reset_runtime();
    Apple p = make_object(7);
    Operands o;
    assert(form(&p, 8, o.a, o.b, o.c, o.y, o.z, HS_ERR_BAD_ARG) == HS_ERR_BAD_ARG);
    assert(o.results_untouched() && copies(hipMemcpyDeviceToHost) == 0 && logged(kSync) == 1 && logged(kFree) == 5 && waited_before_freeing());
}

void test_in_place() {
    // one buffer copied in and copied out: to the same array, or to another
    for (bool same : {true, false}) {
        reset_runtime();
        Apple p = make_object(6);
        float s[6] = {1, 2, 3, 4, 5, 6}, other[6] = {};
        float* to = same ? s : other;
        {
            Staging st(&p);
            float* d = st.inout(static_cast<const float*>(s), to, 1, p.nnz, p.nnz);
            assert(d && st.failed() == HS_OK);
            for (size_t i = 0; i < 6; ++i) d[i] *= 2;
            assert(st.finish(HS_OK) == HS_OK);
        }
        for (size_t i = 0; i < 6; ++i) assert(to[i] == float(2 * (i + 1)) && (same || s[i] == float(i + 1)));
        assert(logged(kMalloc) == 1 && logged(kFree) == 1 && copies(hipMemcpyHostToDevice) == 1 && copies(hipMemcpyDeviceToHost) == 1 && waited_before_freeing());
    }
}

void test_injected_failures() {
    // every allocation and every copy of the form in turn: HS_ERR_HIP with a reason, each allocation freed once (hipFree above asserts
    // it, reset_runtime that none is left), and never a free while a copy may be in flight
    for (Kind kind : {kMalloc, kCopy})
        for (int at = 0; at < 5; ++at)
            for (size_t ld : {size_t(8), kWords}) {
                reset_runtime();
                g_fail_at[kind] = at;
                Apple p = make_object(7);
                Operands o;
                assert(form(&p, ld, o.a, o.b, o.c, o.y, o.z) == HS_ERR_HIP);
                assert(!p.error.empty() && p.error.find("fake runtime") != std::string::npos);
                assert(g_live.empty() && logged(kFree) == logged(kMalloc));
                assert(waited_before_freeing() && logged(kSync) == 1);
                assert(o.tail_untouched());
                if (kind == kMalloc || at < 3) assert(o.results_untouched());
            }
    // an owner that goes out of scope without finish() waits too
    reset_runtime();
    {
        Apple p = make_object(7);
        Operands o;
        Staging st(&p);
        assert(st.in(o.a, kRows, kWords, 8) != nullptr);
    }
    assert(logged(kSync) == 1 && logged(kFree) == 1 && waited_before_freeing());
}

void test_failed_wait() {
    // after a clean run the wait's failure is the result; after an earlier failure that one is kept, code and text
    reset_runtime();
    g_fail_at[kSync] = 0;
    Apple p = make_object(7);
    Operands o;
    assert(form(&p, 8, o.a, o.b, o.c, o.y, o.z) == HS_ERR_HIP && p.error.find("hipStreamSynchronize") == 0);
    reset_runtime();
    g_fail_at[kSync] = 0;
    g_fail_at[kMalloc] = 1;
    Apple q = make_object(7);
    assert(form(&q, 8, o.a, o.b, o.c, o.y, o.z) == HS_ERR_HIP && q.error.find("allocating") == 0);
    reset_runtime();
    g_fail_at[kSync] = 0;
    Apple r = make_object(7);
    r.error = "the refusal of the _device form";
    assert(form(&r, 8, o.a, o.b, o.c, o.y, o.z, HS_ERR_UNSUPPORTED) == HS_ERR_UNSUPPORTED && r.error == "the refusal of the _device form");
}

void test_object_calls() {
    reset_runtime();
    assert(destroy(static_cast<Apple*>(nullptr)) == HS_OK && g_log.empty());
    uint64_t nnz = 1, bytes = 1;
    assert(info(nullptr, &nnz, &bytes) == HS_ERR_BAD_ARG && nnz == 1 && bytes == 1);
    assert(set_stream(nullptr, stream_of(0x20)) == HS_ERR_BAD_ARG);
    assert(sync(static_cast<Apple*>(nullptr)) == HS_ERR_BAD_ARG && enter(static_cast<Apple*>(nullptr)) == HS_ERR_BAD_ARG && g_log.empty());

    Apple* p = new Apple(make_object(7));
    p->device_bytes = 640;
    assert(info(p, &nnz, &bytes) == HS_OK && nnz == 7 && bytes == 640 && info(p, nullptr, nullptr) == HS_OK);
    assert(set_stream(p, stream_of(0x20)) == HS_OK && p->stream == stream_of(0x20) && p->own_stream == stream_of(0x10));
    assert(sync(p) == HS_OK && g_log.size() == 1 && g_log[0].kind == kSync && g_log[0].ptr == stream_of(0x20));      // the caller's stream
    assert(set_stream(p, nullptr) == HS_OK && p->stream == p->own_stream);
    g_fail_at[kSync] = 1;
    assert(sync(p) == HS_ERR_HIP && std::string(last_error(p)).find("hipStreamSynchronize(p->stream)") == 0);
    // destroy waits for the object's own stream, then gives it back
    g_log.clear();
    assert(destroy(p) == HS_OK);
    assert(g_log.size() == 2 && g_log[0].kind == kSync && g_log[1].kind == kStreamDestroy && g_log[0].ptr == stream_of(0x10) && g_log[1].ptr == stream_of(0x10));

    // each family keeps its own create-time text
    assert(std::string(last_error(static_cast<const Apple*>(nullptr))).empty());
    assert(fail<Apple>(nullptr, HS_ERR_BAD_ARG, "an apple was refused") == HS_ERR_BAD_ARG);
    assert(fail<Pear>(nullptr, HS_ERR_NO_DEVICE, "a pear was refused") == HS_ERR_NO_DEVICE);
    assert(std::string(last_error(static_cast<const Apple*>(nullptr))) == "an apple was refused");
    assert(std::string(last_error(static_cast<const Pear*>(nullptr))) == "a pear was refused");
    Pear pear;
    assert(fail(&pear, HS_ERR_BAD_ARG, "this pear") == HS_ERR_BAD_ARG && std::string(last_error(&pear)) == "this pear");
    assert(std::string(last_error(static_cast<const Pear*>(nullptr))) == "a pear was refused");

    // a create call whose build() failed: the reason moves to the family's text, the stream and the object go, nothing is handed out
    reset_runtime();
    Pear* made = new Pear;
    made->own_stream = made->stream = stream_of(0x30);
    made->error = "build failed";
    Pear* out = nullptr;
    assert(finish_create(&out, made, HS_ERR_HIP) == HS_ERR_HIP && out == nullptr);
    assert(std::string(last_error(static_cast<const Pear*>(nullptr))) == "build failed" && logged(kStreamDestroy) == 1);
    assert(std::string(last_error(static_cast<const Apple*>(nullptr))) == "an apple was refused");
    made = new Pear;
    assert(finish_create(&out, made, HS_OK) == HS_OK && out == made);
    assert(destroy(out) == HS_OK);      // no stream of its own: nothing to wait for
    assert(logged(kStreamDestroy) == 1);
}

}  // namespace

int main() {
    test_round_trips();
    test_nothing_to_copy();
    test_optional_operands();
    test_refused_device_call();
    test_in_place();
    test_injected_failures();
    test_failed_wait();
    test_object_calls();
    reset_runtime();
    std::cout << "STAGING OK" << std::endl;
    return 0;
}
