// ht_frame_registry.h — which live context has frames bound where, and the ht_device_alloc buffers that outlived their owner: the
// process-wide bookkeeping behind "never free HBM under a context that has frames bound inside it".  Plain C++17, no HIP: the registry
// decides and returns lists, csrc/ht_frames.hip and ht_destroy free what it lists (release_buffers); tests/host/frame_registry_harness.cc
// compiles the SAME file with g++ under AddressSanitizer + UBSan and, with threads, under ThreadSanitizer.
//
// A context owns one slot.  Its binding is PUBLISHED there by the context's own thread (ht_frames_set, the only writer of c->d_frames)
// with release order; the registry reads it with acquire order under its mutex.  No thread reads another context's fields.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

struct HtFrameSlot {
    int device = 0;                    // written before add(), constant while the slot is registered
    std::atomic<uintptr_t> bound{0};   // address of the first bound frame; 0: nothing bound
};

// a buffer to free (orphan: it outlived its owner, so work of OTHER contexts may still be in flight against it), or one kept as an orphan
struct HtFrameBuffer {
    void *p;
    size_t bytes;
    int device;
    bool orphan;
};

class HtFrameRegistry {
  public:
    void add(HtFrameSlot *s) {
        std::lock_guard<std::mutex> lk(mu_);
        slots_.push_back(s);
    }
    void remove(HtFrameSlot *s) {  // a slot that was never added: nothing happens
        std::lock_guard<std::mutex> lk(mu_);
        slots_.erase(std::remove(slots_.begin(), slots_.end(), s), slots_.end());
    }
    static void publish(HtFrameSlot *s, const void *first_frame) {
        s->bound.store(reinterpret_cast<uintptr_t>(first_frame), std::memory_order_release);
    }

    // is any slot but `except` bound inside [p, p + bytes) on this device?
    bool bound_inside(const HtFrameSlot *except, int device, const void *p, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu_);
        return bound_locked(except, device, p, bytes);
    }

    // An owner (its slot already removed) gives up its allocations: those no slot is bound inside are released now, the others are kept
    // as orphans.  Orphans of earlier owners that have meanwhile become free are released with them.
    std::vector<HtFrameBuffer> retire(int device, const std::vector<std::pair<void *, size_t>> &allocs) {
        std::vector<HtFrameBuffer> release;
        std::lock_guard<std::mutex> lk(mu_);
        for (const auto &a : allocs) {
            if (bound_locked(nullptr, device, a.first, a.second)) orphans_.push_back(HtFrameBuffer{a.first, a.second, device, true});
            else release.push_back(HtFrameBuffer{a.first, a.second, device, false});
        }
        sweep_locked(release);
        return release;
    }

    // the orphans no slot is bound inside any more.  One relaxed load when there are none (the streaming hosts bind per step).
    std::vector<HtFrameBuffer> sweep() {
        std::vector<HtFrameBuffer> release;
        if (orphan_count_.load(std::memory_order_relaxed) == 0) return release;
        std::lock_guard<std::mutex> lk(mu_);
        sweep_locked(release);
        return release;
    }

    std::vector<HtFrameBuffer> orphans() {  // a copy, for the harness
        std::lock_guard<std::mutex> lk(mu_);
        return orphans_;
    }

  private:
    bool bound_locked(const HtFrameSlot *except, int device, const void *p, size_t bytes) const {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        for (const HtFrameSlot *s : slots_) {
            if (s == except || s->device != device) continue;
            const uintptr_t b = s->bound.load(std::memory_order_acquire);
            if (b && b >= lo && b - lo < bytes) return true;
        }
        return false;
    }
    void sweep_locked(std::vector<HtFrameBuffer> &release) {
        auto keep = std::stable_partition(orphans_.begin(), orphans_.end(),
                                          [this](const HtFrameBuffer &o) { return bound_locked(nullptr, o.device, o.p, o.bytes); });
        release.insert(release.end(), keep, orphans_.end());
        orphans_.erase(keep, orphans_.end());
        orphan_count_.store((int)orphans_.size(), std::memory_order_relaxed);
    }

    std::mutex mu_;
    std::vector<HtFrameSlot *> slots_;
    std::vector<HtFrameBuffer> orphans_;
    std::atomic<int> orphan_count_{0};  // orphans_.size(), readable without the lock: the frame-binding calls look at it first
};
