// test_reuse_tracker.cpp — hisparse_amd/csrc/reuse_tracker.h by itself, as a program of its own: no HIP, no library.  tests/test_reuse_tracker_cpu.py
// compiles it with -fsanitize=address,undefined and runs the result.  Prints one line per failed expectation and returns their count.
#include "reuse_tracker.h"

#include <cstdio>
#include <set>
#include <thread>

using hisparse::ReuseList;
using hisparse::ReuseTracker;

namespace {

constexpr uint64_t kBudget = 256ull << 20;      // stream_tiles.h: kResidentMaxImageBytes
constexpr uint64_t kMB = 1000000;
int failures = 0;

void expect(bool ok, const char* what) {
    if (ok) return;
    std::printf("FAILED: %s\n", what);
    ++failures;
}

bool launch(ReuseTracker& t, uint64_t id, uint64_t bytes) { return t.launch_resident(-1, true, id, bytes, kBudget); }

void consecutive() {
    ReuseTracker t;
    expect(!launch(t, 1, 233 * kMB), "first launch cold");
    expect(launch(t, 1, 233 * kMB), "second consecutive launch warm");
    expect(launch(t, 1, 233 * kMB), "third consecutive launch warm");
    expect(!t.launch_resident(-1, false, 1, 233 * kMB, kBudget), "a warm image that is not eligible stays nt");
}

void two_that_fit() {
    ReuseTracker t;
    expect(!launch(t, 1, 100 * kMB) && !launch(t, 2, 100 * kMB), "A, B: first round cold");
    for (int round = 0; round < 3; ++round) expect(launch(t, 1, 100 * kMB) && launch(t, 2, 100 * kMB), "A, B with 2 x 100 MB: warm from the second round");
}

void three_that_do_not() {
    ReuseTracker t;
    for (int round = 0; round < 4; ++round)
        for (uint64_t id = 1; id <= 3; ++id) expect(!launch(t, id, 233 * kMB), "A, B, C with 3 x 233 MB: never warm");
    // ... and an image launched twice in between counts once: A, B, B, A with 2 x 100 MB is warm
    ReuseTracker u;
    (void)launch(u, 1, 100 * kMB);
    (void)launch(u, 2, 100 * kMB);
    expect(launch(u, 2, 100 * kMB), "B, B warm");
    expect(launch(u, 1, 100 * kMB), "A, B, B, A: B counted once");
}

void too_large() {
    ReuseTracker t;
    for (int i = 0; i < 3; ++i) expect(!launch(t, 1, 257ull << 20), "an image of 257 MiB: never warm");
    ReuseTracker u;
    (void)launch(u, 1, 256ull << 20);
    expect(launch(u, 1, 256ull << 20), "an image of exactly 256 MiB is warm on its second launch");
    ReuseTracker v;
    (void)launch(v, 1, ~0ull - 5);
    (void)launch(v, 2, 10);
    expect(!launch(v, 1, ~0ull - 5), "a distance that overflows 64 bits is not warm");
}

void reload() {
    ReuseTracker t;
    const uint64_t a = hisparse::next_image_id();
    (void)launch(t, a, 50 * kMB);
    expect(launch(t, a, 50 * kMB), "warm before the reload");
    const uint64_t b = hisparse::next_image_id();
    expect(b != a && b != 0, "a reload gets a fresh id");
    expect(!launch(t, b, 50 * kMB), "a new id after a reload is cold");
    expect(launch(t, b, 50 * kMB), "... and warm afterwards");
}

void falls_off() {
    ReuseTracker t;
    (void)launch(t, 1000, 1);
    for (uint64_t id = 1; id < hisparse::kReuseListEntries; ++id) (void)launch(t, id, 1);
    expect(launch(t, 1000, 1), "the last entry of a full list is still warm");
    for (uint64_t id = 1; id <= hisparse::kReuseListEntries; ++id) (void)launch(t, 2000 + id, 1);
    expect(!launch(t, 1000, 1), "falling off the list is cold");
    const ReuseList l = t.snapshot();
    expect(l.count == hisparse::kReuseListEntries && l.entry[0].id == 1000, "a full list stays full, most recent first");
}

void forced() {
    ReuseTracker t;
    expect(t.launch_resident(1, true, 1, 233 * kMB, kBudget), "forced 1 on a cold image is resident");
    expect(!t.launch_resident(0, true, 1, 233 * kMB, kBudget), "forced 0 on a warm image is nt");
    expect(t.launch_resident(1, false, 2, 300ull << 20, kBudget), "forced 1 decides by itself");
    expect(launch(t, 1, 1 * kMB) == false && t.snapshot().entry[0].id == 1, "forced launches were recorded: A is behind the 300 MiB image");
}

void scratch_copy() {
    ReuseTracker t;
    (void)launch(t, 1, 10 * kMB);
    const ReuseList before = t.snapshot();
    ReuseList scratch = t.snapshot();
    expect(!hisparse::launch_resident(scratch, -1, true, 2, 100 * kMB, kBudget), "captured step 1 from a cold state is nt");
    for (int k = 1; k < 4; ++k) expect(hisparse::launch_resident(scratch, -1, true, 2, 100 * kMB, kBudget), "captured steps 2 .. K are resident");
    const ReuseList after = t.snapshot();
    bool same = before.count == after.count;
    for (uint32_t i = 0; same && i < before.count; ++i) same = before.entry[i].id == after.entry[i].id && before.entry[i].bytes == after.entry[i].bytes;
    expect(same && after.count == 1, "the scratch copy used under capture leaves the real state untouched");
    t.touch(2, 100 * kMB);      // one replay
    expect(t.snapshot().entry[0].id == 2 && t.snapshot().count == 2, "a replay touches the real tracker once");
}

void two_devices() {
    ReuseTracker& d0 = hisparse::reuse_tracker_for(0);
    ReuseTracker& d1 = hisparse::reuse_tracker_for(1);
    expect(&d0 != &d1 && &d0 == &hisparse::reuse_tracker_for(0), "one tracker per device, the same one every time");
    (void)launch(d0, 7, 10 * kMB);
    expect(!launch(d1, 7, 10 * kMB), "two devices do not see each other");
    expect(launch(d0, 7, 10 * kMB), "device 0 kept its own state");
}

void four_threads() {
    ReuseTracker t;
    std::thread workers[4];
    for (int w = 0; w < 4; ++w)
        workers[w] = std::thread([&t, w] {
            for (int i = 0; i < 20000; ++i) (void)t.launch_resident(i % 3 - 1, true, uint64_t(w * 16 + i % 16 + 1), uint64_t(i % 5 + 1) * kMB, kBudget);
        });
    for (std::thread& w : workers) w.join();
    const ReuseList l = t.snapshot();
    std::set<uint64_t> ids;
    bool in_range = true;
    for (uint32_t i = 0; i < l.count; ++i) {
        ids.insert(l.entry[i].id);
        in_range = in_range && l.entry[i].id >= 1 && l.entry[i].id <= 64 && l.entry[i].bytes >= kMB && l.entry[i].bytes <= 5 * kMB;
    }
    expect(l.count == hisparse::kReuseListEntries && ids.size() == l.count && in_range, "four threads hammering one tracker finish with a consistent list: full, no id twice");
}

}  // namespace

int main() {
    consecutive();
    two_that_fit();
    three_that_do_not();
    too_large();
    reload();
    falls_off();
    forced();
    scratch_copy();
    two_devices();
    four_threads();
    if (failures) std::printf("%d failed\n", failures);
    else std::printf("REUSE TRACKER OK\n");
    return failures;
}
