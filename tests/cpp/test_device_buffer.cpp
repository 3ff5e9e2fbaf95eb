// The owner of device memory (hisparse_amd/csrc/device_buffer.h: DeviceBuffer) with a counting `Free` over host addresses: no GPU, no HIP
// runtime linked.  alloc / alloc_count call hipMalloc and are not instantiated here.
#undef NDEBUG
#include "device_buffer.h"
#include <cassert>
#include <iostream>
#include <stdexcept>

static int cells[8];          // the "allocations": &cells[i]
static int freed[8];          // how often each was given back
static hipError_t count_free(void* p) {
    const long i = static_cast<int*>(p) - cells;
    assert(i >= 0 && i < 8);
    ++freed[i];
    return hipSuccess;
}
using Buf = DeviceBuffer<int, count_free>;
static int total() { int n = 0; for (int f : freed) n += f; return n; }
static void clear() { for (int& f : freed) f = 0; }

int main() {
    // destruction frees exactly once; an empty owner frees nothing
    { Buf a; a.adopt(&cells[0]); assert(a && a.get() == &cells[0]); Buf empty; assert(!empty && empty.get() == nullptr); }
    assert(freed[0] == 1 && total() == 1);
    clear();
    // move construction: nothing is freed by the move, the source is empty, one free at the end
    {
        Buf a; a.adopt(&cells[0]);
        Buf b(std::move(a));
        assert(!a && a.get() == nullptr && b.get() == &cells[0] && total() == 0);
    }
    assert(freed[0] == 1 && total() == 1);
    clear();
    // move assignment: the overwritten pointer is freed once, at the assignment; the source is empty
    {
        Buf a, b; a.adopt(&cells[0]); b.adopt(&cells[1]);
        b = std::move(a);
        assert(freed[1] == 1 && total() == 1 && !a && b.get() == &cells[0]);
    }
    assert(freed[0] == 1 && freed[1] == 1 && total() == 2);
    clear();
    // self-move-assignment frees nothing and keeps the pointer
    {
        Buf a; a.adopt(&cells[2]);
        Buf& same = a;
        a = std::move(same);
        assert(total() == 0 && a.get() == &cells[2]);
    }
    assert(freed[2] == 1 && total() == 1);
    clear();
    // adopt over a held pointer frees the old one
    {
        Buf a; a.adopt(&cells[0]);
        a.adopt(&cells[1]);
        assert(freed[0] == 1 && total() == 1 && a.get() == &cells[1]);
    }
    assert(freed[1] == 1 && total() == 2);
    clear();
    // release frees nothing, then or later
    { Buf a; a.adopt(&cells[3]); assert(a.release() == &cells[3] && !a); }
    assert(total() == 0);
    // reset twice frees once
    { Buf a; a.adopt(&cells[4]); a.reset(); a.reset(); assert(freed[4] == 1 && total() == 1 && !a); }
    assert(freed[4] == 1 && total() == 1);
    clear();
    // an array of owners, an exception in their scope: each is freed once
    try {
        Buf many[8];
        for (int i = 0; i < 8; ++i) many[i].adopt(&cells[i]);
        throw std::runtime_error("between allocation and the end of the scope");
    } catch (const std::runtime_error&) {
    }
    for (int f : freed) assert(f == 1);
    std::cout << "DEVICE BUFFER OK" << std::endl;
    return 0;
}
