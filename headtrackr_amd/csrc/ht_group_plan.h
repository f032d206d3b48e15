// ht_group_plan.h — the host side of the device grouping (ht_group.hip): the per-frame cap, the layout of the block the collect call
// fetches with one copy, the argument checks of ht_group_hits, the record <-> rect conversion and the host completion of the frames
// the kernel leaves alone (more hits than one workgroup's LDS takes).  Plain C++ (no HIP): the library compiles it as part of
// ht_group.hip, tests/host/group_harness.cc compiles the SAME file with g++ -fsanitize=address,undefined.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ht_hostpost.h"

constexpr uint32_t HT_GRP_CAP_MAX = 1024;  // hits of one frame a k_grp_frames workgroup takes: the largest power of two whose records fit 64 KB of LDS
constexpr uint32_t HT_GRP_CAP_MIN = 64;    // one wavefront
constexpr uint32_t HT_GRP_REC_F64 = 8;     // doubles of one per-frame record (headtrackr_amd/distributed.py)

// status word of a frame
enum : uint32_t {
    HT_GRP_ST_OVER_CAP = 1u,  // more hits than the cap: nothing computed on the device, the collect call finishes the frame on the host
};

// head of the result block (16 bytes), in front of the records
struct HtGrpHead {
    uint32_t nhits;  // the batch's raw hit count (HtCounters::nhits, or n of ht_group_hits)
    uint32_t bad;    // hits whose frame or scale was out of range (skipped)
    uint32_t pad[2];
};
static_assert(sizeof(HtGrpHead) == 16, "HtGrpHead");

// the result block on the device and in pinned host memory: [head][nframes records of 64 B][status][ngrouped][count][start], the four
// per-frame tables nframes u32 each.  Offsets in bytes.
struct HtGrpLayout {
    size_t records, status, ngrouped, count, start, bytes;
};
inline HtGrpLayout ht_grp_layout(uint32_t nframes) {
    HtGrpLayout L;
    L.records = sizeof(HtGrpHead);
    L.status = L.records + (size_t)nframes * HT_GRP_REC_F64 * sizeof(double);
    L.ngrouped = L.status + (size_t)nframes * sizeof(uint32_t);
    L.count = L.ngrouped + (size_t)nframes * sizeof(uint32_t);
    L.start = L.count + (size_t)nframes * sizeof(uint32_t);
    L.bytes = L.start + (size_t)nframes * sizeof(uint32_t);
    return L;
}

// option group_cap=N: the largest power of two <= N inside [HT_GRP_CAP_MIN, HT_GRP_CAP_MAX]
inline uint32_t ht_grp_cap(long long option) {
    if (option >= (long long)HT_GRP_CAP_MAX) return HT_GRP_CAP_MAX;
    uint32_t cap = HT_GRP_CAP_MIN;
    while ((long long)cap * 2 <= option) cap *= 2;
    return cap;
}

// ht_group_hits' arguments: everything the call dereferences, sizes that fit the context
inline ht_status ht_grp_check_hits(const ht_hit *hits, uint32_t n, int32_t nframes, uint32_t hit_capacity, const ht_rect *best, const ht_rect *grouped,
                                   const uint32_t *ngrouped, const char **why) {
    const char *w = nullptr;
    if (nframes <= 0) w = "nframes must be positive";
    else if (!best) w = "best is NULL";
    else if (n && !hits) w = "hits is NULL";
    else if ((grouped == nullptr) != (ngrouped == nullptr)) w = "grouped and ngrouped go together";
    else if (n > hit_capacity) w = "more hits than ht_config.hit_capacity";
    if (why) *why = w;
    return w ? HT_ERR_INVALID : HT_OK;
}

inline void ht_grp_rect_to_record(const ht_rect &r, double frame_index, double *rec) {
    rec[0] = r.x, rec[1] = r.y, rec[2] = r.width, rec[3] = r.height, rec[4] = r.confidence;
    rec[5] = (double)r.neighbors, rec[6] = frame_index, rec[7] = 1.0;
}
inline ht_rect ht_grp_record_to_rect(const double *rec) {
    ht_rect r;
    r.x = rec[0], r.y = rec[1], r.width = rec[2], r.height = rec[3], r.confidence = rec[4];
    r.neighbors = (int32_t)rec[5], r.reserved = 0;
    return r;
}

// One frame on the host, for the frames the kernel flags: `hits` (n of them, any order, modified: put into emission order) -> the
// frame's grouped list (grouped: room for n rects; *ngrouped) and its best face, exactly as ht_post_best_face selects it.
inline ht_status ht_grp_complete_frame(const HtPostCfg &cfg, const double *sx, ht_hit *hits, uint32_t n, int32_t min_neighbors, ht_rect *best,
                                       ht_rect *grouped, uint32_t *ngrouped) {
    if (!best || !ngrouped || (n && (!hits || !grouped))) return HT_ERR_INVALID;
    *ngrouped = 0;
    ht_rect r = {0, 0, 0, 0, -10000.0, 0, 0};  // facetrackr.js:233-241
    if (n) {
        ht_post_sort_frame(hits, 0, n);
        std::vector<ht_rect> seq(n);
        ht_status st = ht_post_hits_to_rects(cfg, sx, hits, n, seq.data());
        if (st != HT_OK) return st;
        uint32_t ng = n;
        if (min_neighbors > 0) {
            if ((st = ht_post_group_rects(seq.data(), n, min_neighbors, grouped, &ng)) != HT_OK) return st;
        } else {
            std::memcpy(grouped, seq.data(), sizeof(ht_rect) * (size_t)n);
        }
        for (uint32_t i = 0; i < ng; i++)  // facetrackr.js:157-165
            if (i == 0 || grouped[i].confidence > r.confidence) r = grouped[i];
        *ngrouped = ng;
    }
    *best = r;
    return HT_OK;
}
