// Host-only harness around headtrackr_amd/csrc/ht_frame_registry.h (which live context is bound where, and the buffers that outlived
// their owner), built by tests/test_frame_registry_cpu.py three times: plain, with g++ -fsanitize=address,undefined and — for the threaded
// mode — with -fsanitize=thread; each a program of its own, run directly.  Pointers are numbers here: the registry never dereferences them.
//
//   frame_registry_harness <script>      one operation per line:
//       add S DEVICE | remove S | publish S ADDRESS | retire DEVICE N (ADDRESS BYTES) x N | sweep | query EXCEPT DEVICE ADDRESS BYTES
//     (S: a slot number of the script's own choosing; EXCEPT: a slot number or -1)
//     one JSON object per line: {"op", "answer" (query: 0 / 1, else -1), "release": [[address, bytes, device, orphan]..],
//     "orphans": [[address, bytes, device]..] (the set kept after the operation)}
//   frame_registry_harness --threads N   two threads publish bindings that move among four buffers N times each and sweep behind every
//     move, as the frame calls do; a third retires the buffers (a fresh one takes each one's place) and sweeps.  After the join every slot
//     is unbound and one last sweep runs: every retired buffer has to have been released exactly once.  One JSON line; exit status 1 if not.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <thread>

#include "ht_frame_registry.h"

static void *ptr_of(unsigned long long v) { return reinterpret_cast<void *>(static_cast<uintptr_t>(v)); }
static unsigned long long num_of(const void *p) { return static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(p)); }

static int run_script(const char *path) {
    HtFrameRegistry reg;
    std::map<long long, std::unique_ptr<HtFrameSlot>> slots;
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op;
        if (!(ls >> op)) continue;
        std::vector<HtFrameBuffer> release;
        int answer = -1;
        long long s, device;
        unsigned long long addr, bytes;
        if (op == "add" && ls >> s >> device) {
            slots[s] = std::make_unique<HtFrameSlot>();
            slots[s]->device = (int)device;
            reg.add(slots[s].get());
        } else if (op == "remove" && ls >> s && slots.count(s)) {
            reg.remove(slots[s].get());
            slots.erase(s);
        } else if (op == "publish" && ls >> s >> addr && slots.count(s)) {
            HtFrameRegistry::publish(slots[s].get(), ptr_of(addr));
        } else if (op == "retire" && ls >> device >> s) {
            std::vector<std::pair<void *, size_t>> allocs;
            for (long long i = 0; i < s; i++) {
                if (!(ls >> addr >> bytes)) return 2;
                allocs.emplace_back(ptr_of(addr), (size_t)bytes);
            }
            release = reg.retire((int)device, allocs);
        } else if (op == "sweep") {
            release = reg.sweep();
        } else if (op == "query" && ls >> s >> device >> addr >> bytes) {
            answer = reg.bound_inside(slots.count(s) ? slots[s].get() : nullptr, (int)device, ptr_of(addr), (size_t)bytes) ? 1 : 0;
        } else {
            return 2;
        }
        std::printf("{\"op\": \"%s\", \"answer\": %d, \"release\": [", op.c_str(), answer);
        for (size_t i = 0; i < release.size(); i++)
            std::printf("%s[%llu, %zu, %d, %d]", i ? ", " : "", num_of(release[i].p), release[i].bytes, release[i].device, (int)release[i].orphan);
        std::printf("], \"orphans\": [");
        const std::vector<HtFrameBuffer> kept = reg.orphans();
        for (size_t i = 0; i < kept.size(); i++) std::printf("%s[%llu, %zu, %d]", i ? ", " : "", num_of(kept[i].p), kept[i].bytes, kept[i].device);
        std::printf("]}\n");
    }
    return 0;
}

static int run_threads(long iterations) {
    constexpr int NBUF = 4;
    constexpr size_t BYTES = 4096;
    HtFrameRegistry reg;
    HtFrameSlot slots[2];
    std::atomic<uintptr_t> buf[NBUF];
    uintptr_t fresh = 0x100000;  // addresses are never used twice
    for (auto &b : buf) b.store(fresh, std::memory_order_relaxed), fresh += 0x10000;
    for (auto &s : slots) reg.add(&s);
    std::vector<HtFrameBuffer> released[3];
    std::vector<uintptr_t> retired;

    auto binder = [&](int t) {
        uint32_t rng = 12345u + 977u * (uint32_t)t;
        for (long i = 0; i < iterations; i++) {
            rng = rng * 1664525u + 1013904223u;
            const uintptr_t base = buf[(rng >> 8) % NBUF].load(std::memory_order_acquire);
            const bool unbind = (rng >> 20) % 16 == 0;
            HtFrameRegistry::publish(&slots[t], unbind ? nullptr : ptr_of(base + ((rng >> 12) % BYTES & ~3u)));
            const std::vector<HtFrameBuffer> r = reg.sweep();
            released[t].insert(released[t].end(), r.begin(), r.end());
        }
    };
    auto retirer = [&] {
        for (long i = 0; i < iterations / 2; i++) {
            const int j = (int)(i % NBUF);
            const uintptr_t old = buf[j].exchange(fresh, std::memory_order_acq_rel);  // the binders move to its successor from here on
            fresh += 0x10000;
            retired.push_back(old);
            std::vector<HtFrameBuffer> r = reg.retire(0, {{ptr_of(old), BYTES}});
            released[2].insert(released[2].end(), r.begin(), r.end());
            r = reg.sweep();
            released[2].insert(released[2].end(), r.begin(), r.end());
            if (i % 64 == 0) std::this_thread::yield();
        }
    };
    std::thread a(binder, 0), b(binder, 1), c(retirer);
    a.join(), b.join(), c.join();
    for (auto &s : slots) HtFrameRegistry::publish(&s, nullptr);
    const std::vector<HtFrameBuffer> last = reg.sweep();
    released[2].insert(released[2].end(), last.begin(), last.end());

    std::map<uintptr_t, int> times;
    size_t as_orphan = 0;
    for (const auto &list : released)
        for (const HtFrameBuffer &r : list) times[reinterpret_cast<uintptr_t>(r.p)]++, as_orphan += r.orphan;
    size_t twice = 0, never = 0, unknown = times.size();
    for (uintptr_t p : retired) {
        const auto it = times.find(p);
        if (it == times.end()) never++;
        else unknown--, twice += it->second != 1;
    }
    const size_t kept = reg.orphans().size();
    std::printf("{\"retired\": %zu, \"released\": %zu, \"as_orphan\": %zu, \"twice\": %zu, \"never\": %zu, \"unknown\": %zu, \"orphans_left\": %zu}\n", retired.size(),
                times.size(), as_orphan, twice, never, unknown, kept);
    return (twice || never || unknown || kept || retired.empty()) ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--threads")) return run_threads(std::atol(argv[2]));
    if (argc == 2) return run_script(argv[1]);
    return 2;
}
