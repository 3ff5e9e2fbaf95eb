// reuse_tracker.h — is a stream image still in the Infinity Cache when it is launched again?  Plain C++ (no HIP types: a host program tests it,
// tests/cpp/test_reuse_tracker.cpp), shared by every context of a device.
//
// The row-block and SWEEP kernels exist in two cache policies (spmv_kernels.hip: Ring<kRing | 4>, spmv_sweep.hip): `sc1` stream loads, which leave the image in
// the 256 MiB Infinity Cache for the next step, and `nt` loads, which pass it by.  `sc1` wins 8-9 % on a loop over ONE image that fits the cache and loses as
// much once a caller alternates between images that together exceed it (stream_tiles.h: kRowblockResidentMaxImageBytes).  Which of the two a launch is in
// depends on what was launched since the image's previous launch, and that is known at launch time: hs_api.cpp (launch_args) asks this tracker for every SpMV.
//
// The state is a short most-recently-used list of (image id, stream bytes).  The question at a launch: since this image's previous launch, have the images
// launched since then -- each counted once, however often it ran -- plus this image itself streamed no more than `budget` bytes?  That sum is the image's reuse
// distance in bytes; an image that is not in the list (never launched, or pushed off its end by kReuseListEntries others) is cold.  Every SpMV launch of every
// format records its image, whichever policy it runs with and whether or not its kernel has two: it moves its bytes through the cache all the same.
// An image id is fresh per load (next_image_id); hs_update_values takes a new one too, since it rewrites the image.
#ifndef HISPARSE_REUSE_TRACKER_H_
#define HISPARSE_REUSE_TRACKER_H_

#include <atomic>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

namespace hisparse {

constexpr uint32_t kReuseListEntries = 32;

// The list by itself: a value, so that a stream capture can decide on a copy (ReuseTracker::snapshot) and leave the device's own state alone.
struct ReuseList {
    struct Entry { uint64_t id, bytes; };
    Entry entry[kReuseListEntries] = {};
    uint32_t count = 0;

    // One launch of image `id` streaming `bytes`: was it warm (reuse distance <= budget)?  The image becomes the most recently used one.
    bool touch(uint64_t id, uint64_t bytes, uint64_t budget) {
        uint32_t at = 0;
        uint64_t distance = bytes;      // this image + every image in front of it
        bool sums = true;               // (no overflow: a sum that wrapped would read as small)
        while (at < count && entry[at].id != id) {
            sums = sums && distance + entry[at].bytes >= distance;
            distance += entry[at].bytes;
            ++at;
        }
        const bool warm = at < count && sums && distance <= budget;
        if (at == count && count < kReuseListEntries) ++count;      // a new image; with a full list the least recently used one falls off
        if (at == kReuseListEntries) --at;
        for (; at > 0; --at) entry[at] = entry[at - 1];
        entry[0] = Entry{id, bytes};
        return warm;
    }
};

// The decision of one launch.  `forced`: the caller's stream_resident option, 0 | 1, or < 0 when none is set; `eligible`: the load found the image's
// shape fit to be streamed resident at all (stream_tiles.h: plan_stream_resident).  An option decides by itself -- always `nt` / always `sc1` -- and a
// launch is recorded whatever decides.
inline bool launch_resident(ReuseList& list, int forced, bool eligible, uint64_t id, uint64_t bytes, uint64_t budget) {
    const bool warm = list.touch(id, bytes, budget);
    return forced >= 0 ? forced != 0 : eligible && warm;
}

// One device's list behind a lock: contexts of several threads share it.  Uncontended on the launch path of a single caller.
class ReuseTracker {
public:
    bool launch_resident(int forced, bool eligible, uint64_t id, uint64_t bytes, uint64_t budget) {
        std::lock_guard<std::mutex> hold(lock_);
        return hisparse::launch_resident(list_, forced, eligible, id, bytes, budget);
    }
    // a replayed graph ran the image (again): no decision to take, its launches are frozen
    void touch(uint64_t id, uint64_t bytes) {
        std::lock_guard<std::mutex> hold(lock_);
        (void)list_.touch(id, bytes, 0);
    }
    ReuseList snapshot() const {
        std::lock_guard<std::mutex> hold(lock_);
        return list_;
    }

private:
    mutable std::mutex lock_;
    ReuseList list_;
};

// The tracker of device `device` (>= 0), created on first use and alive until the process ends; a context looks it up once, when it is created.
inline ReuseTracker& reuse_tracker_for(int device) {
    static std::mutex lock;
    static auto& trackers = *new std::vector<std::unique_ptr<ReuseTracker>>;      // never destroyed: a context may outlive the static destructors
    std::lock_guard<std::mutex> hold(lock);
    const size_t at = device < 0 ? 0 : size_t(device);
    if (trackers.size() <= at) trackers.resize(at + 1);
    if (!trackers[at]) trackers[at].reset(new ReuseTracker);
    return *trackers[at];
}

inline uint64_t next_image_id() {
    static std::atomic<uint64_t> last{0};
    return last.fetch_add(1, std::memory_order_relaxed) + 1;      // (0: no image)
}

}  // namespace hisparse

#endif  // HISPARSE_REUSE_TRACKER_H_
