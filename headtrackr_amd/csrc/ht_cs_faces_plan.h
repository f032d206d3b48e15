// ht_cs_faces_plan.h — the rule of ht_camshift_init_faces, without HIP: which grouped face of a frame initialises which of the frame's
// trackers (slots), and the host plan of the call.  Host AND device text, like ht_cs_best_plan.h: k_csf_resolve (ht_cs_faces.hip) compiles
// the predicates, the overlap and the slot fill as device functions and runs the two arg-max loops wave-wide; ht_csf_frame below runs the
// same loops one candidate at a time with the SAME predicates.  tests/host/init_faces_harness.cc compiles this file with
// g++ -fsanitize=address,undefined against tests/init_faces_cases.py, the rule restated in Python.  No library call, no HIP type.
//
// The rule (include/headtrackr_hip.h has the caller's wording): eligible faces by (confidence descending, list index ascending), the
// first k kept; without HT_CSF_ASSOCIATE rank r -> slot r; with it, greedy matching by the largest int64 overlap of a live slot's search
// window with a face's floored rect (ties: lowest slot, then lowest rank), then the remaining faces in rank order into the not-live slots
// and after those into the unmatched live ones.  The slot is the identity: a tracker that overlaps a detection keeps it.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "ht_cs_best_plan.h"  // ht_csb_floor_i32, HT_CSB_ST_OVER_CAP, HT_CSB_* codes through headtrackr_hip.h

static_assert(sizeof(ht_csf_record) == 32, "ht_csf_record");
static_assert(sizeof(ht_rect) == 48, "ht_rect");

// ---- predicates, shared by the kernel and ht_csf_frame -------------------------------------------------------------------------------

// the frame's list is not final on the device: the three conditions of ht_csb_decide
HT_CSB_FN bool ht_csf_not_final(uint32_t status, uint32_t head_nhits, uint32_t head_bad, uint32_t hit_capacity, bool collected) {
    return head_nhits > hit_capacity || head_bad != 0u || (!collected && (status & HT_CSB_ST_OVER_CAP));
}

HT_CSB_FN bool ht_csf_eligible(double confidence, int32_t neighbors, double min_confidence) { return neighbors > 0 && confidence > min_confidence; }

// face (ca, ia) ranks in front of face (cb, ib); both eligible (no NaN), ia != ib
HT_CSB_FN bool ht_csf_face_before(double ca, int32_t ia, double cb, int32_t ib) { return ca > cb || (ca == cb && ia < ib); }

HT_CSB_FN ht_cs_rect ht_csf_rect(double x, double y, double w, double h) {
    ht_cs_rect r;
    r.x = ht_csb_floor_i32(x), r.y = ht_csb_floor_i32(y), r.width = ht_csb_floor_i32(w), r.height = ht_csb_floor_i32(h);
    return r;
}

HT_CSB_FN bool ht_csf_live(const int32_t *sw) { return sw[2] > 0 && sw[3] > 0; }

// area of the intersection of window sw = {x, y, width, height} with rect r, entirely in int64: x + width of saturated int32 values stays
// below 2^32 in magnitude, a side of the intersection is at most 2^31 - 1 (the smaller of two widths), the product below 2^62
HT_CSB_FN int64_t ht_csf_overlap(const int32_t *sw, const ht_cs_rect &r) {
    if (sw[2] <= 0 || sw[3] <= 0 || r.width <= 0 || r.height <= 0) return 0;
    const int64_t ax0 = sw[0], ax1 = ax0 + (int64_t)sw[2], ay0 = sw[1], ay1 = ay0 + (int64_t)sw[3];
    const int64_t bx0 = r.x, bx1 = bx0 + (int64_t)r.width, by0 = r.y, by1 = by0 + (int64_t)r.height;
    const int64_t w = (ax1 < bx1 ? ax1 : bx1) - (ax0 > bx0 ? ax0 : bx0), h = (ay1 < by1 ? ay1 : by1) - (ay0 > by0 ? ay0 : by0);
    return (w > 0 && h > 0) ? w * h : 0;
}

// matching candidate (oa; table position ea = slot * HT_CSF_MAX_SLOTS + rank) is taken in front of (ob, eb): the larger overlap, then the
// lowest slot, then the lowest rank = the lowest table position
HT_CSB_FN bool ht_csf_match_before(int64_t oa, int32_t ea, int64_t ob, int32_t eb) { return oa > ob || (oa == ob && ea < eb); }

// after the matching: the faces without a slot, in rank order, into the slots without a face — not-live ones ascending, then live ones
// ascending.  slot_rank[j]: rank of slot j's face or -1; live / face_taken: bit j / bit r
HT_CSB_FN void ht_csf_fill(int32_t k, int32_t q, uint32_t live, uint32_t face_taken, int32_t *slot_rank) {
    int32_t r = 0;
    for (int32_t pass = 0; pass < 2; pass++)
        for (int32_t j = 0; j < k; j++) {
            if (slot_rank[j] >= 0 || ((live >> j) & 1u) != (uint32_t)pass) continue;
            while (r < q && ((face_taken >> r) & 1u)) r++;
            if (r >= q) return;
            slot_rank[j] = r, face_taken |= 1u << r;
        }
}

HT_CSB_FN ht_csf_record ht_csf_make_record(int32_t code, int32_t face, const ht_cs_rect &rect, int32_t dropped) {
    ht_csf_record o;
    o.code = code, o.face = face, o.rect = rect, o.dropped = dropped, o.reserved = 0;
    return o;
}

// ---- one frame, one candidate at a time ----------------------------------------------------------------------------------------------

// G[0 .. m): the frame's grouped list; sw: k search windows of 4 int32, in slot order; out: k records
HT_CSB_FN void ht_csf_frame(const ht_rect *G, uint32_t m, const int32_t *sw, int32_t k, bool not_final, double min_confidence, uint32_t flags, ht_csf_record *out) {
    const ht_cs_rect zero = {0, 0, 0, 0};
    if (not_final) {
        for (int32_t j = 0; j < k; j++) out[j] = ht_csf_make_record(HT_CSB_DEFERRED, -1, zero, 0);
        return;
    }
    int32_t face[HT_CSF_MAX_SLOTS], slot_rank[HT_CSF_MAX_SLOTS];
    ht_cs_rect rect[HT_CSF_MAX_SLOTS];
    int32_t q = 0, eligible = 0;
    for (uint32_t i = 0; i < m; i++) eligible += ht_csf_eligible(G[i].confidence, G[i].neighbors, min_confidence) ? 1 : 0;
    for (; q < k; q++) {  // round q: the first eligible face behind the one of round q - 1
        int32_t b = -1;
        for (uint32_t i = 0; i < m; i++) {
            if (!ht_csf_eligible(G[i].confidence, G[i].neighbors, min_confidence)) continue;
            if (q > 0 && !ht_csf_face_before(G[face[q - 1]].confidence, face[q - 1], G[i].confidence, (int32_t)i)) continue;
            if (b < 0 || ht_csf_face_before(G[i].confidence, (int32_t)i, G[b].confidence, b)) b = (int32_t)i;
        }
        if (b < 0) break;
        face[q] = b, rect[q] = ht_csf_rect(G[b].x, G[b].y, G[b].width, G[b].height);
    }
    const int32_t dropped = eligible - q;
    for (int32_t j = 0; j < k; j++) slot_rank[j] = -1;
    if (flags & HT_CSF_ASSOCIATE) {
        uint32_t live = 0, slot_taken = 0, face_taken = 0;
        for (int32_t j = 0; j < k; j++) live |= ht_csf_live(sw + 4 * j) ? 1u << j : 0u;
        for (int32_t round = 0; round < k; round++) {
            int64_t bo = 0;
            int32_t be = -1;
            for (int32_t j = 0; j < k; j++)
                for (int32_t r = 0; r < q; r++) {
                    if (!((live >> j) & 1u) || ((slot_taken >> j) & 1u) || ((face_taken >> r) & 1u)) continue;
                    const int64_t o = ht_csf_overlap(sw + 4 * j, rect[r]);
                    const int32_t e = j * HT_CSF_MAX_SLOTS + r;
                    if (o > 0 && (be < 0 || ht_csf_match_before(o, e, bo, be))) bo = o, be = e;
                }
            if (be < 0) break;
            slot_rank[be / HT_CSF_MAX_SLOTS] = be % HT_CSF_MAX_SLOTS;
            slot_taken |= 1u << (be / HT_CSF_MAX_SLOTS), face_taken |= 1u << (be % HT_CSF_MAX_SLOTS);
        }
        ht_csf_fill(k, q, live, face_taken, slot_rank);
    } else {
        for (int32_t j = 0; j < q; j++) slot_rank[j] = j;
    }
    for (int32_t j = 0; j < k; j++) {
        const int32_t r = slot_rank[j];
        out[j] = r >= 0 ? ht_csf_make_record(HT_CSB_FACE, face[r], rect[r], dropped) : ht_csf_make_record(HT_CSB_UNTOUCHED, -1, zero, dropped);
    }
}

// ---- the host plan -------------------------------------------------------------------------------------------------------------------

// the per-frame group table the kernel reads: groups of {frame, first, count}, then the call's pair indices ordered by frame, list order kept
// (group g's slots are order[first .. first + count), in list order)
struct HtCsfPlan {
    std::vector<int32_t> groups;  // 3 per distinct frame, ascending frame
    std::vector<int32_t> order;   // n
    int32_t ngroups() const { return (int32_t)(groups.size() / 3); }
};

// The checks ht_camshift_init_faces adds to the rules of ht_camshift_init_pairs, and the group table.  The pair list has passed csp_plan
// (ht_cs_pairs.hip: the range of n, an unreserved or duplicate stream, a frame that is not bound) — those rules are stated there only.
// Refused here: unknown flag bits, a NaN min_confidence, a frame outside the grouped batch (a negative one included: this function
// indexes by frame), more than HT_CSF_MAX_SLOTS slots on one frame.  Returns HT_OK or HT_ERR_INVALID with *why.
inline ht_status ht_csf_plan(const ht_cs_pair *pairs, int32_t n, int32_t grouped_frames, double min_confidence, uint32_t flags, HtCsfPlan *plan, std::string *why) {
    auto fail = [&](const std::string &w) {
        if (why) *why = w;
        return HT_ERR_INVALID;
    };
    if (flags & ~(uint32_t)HT_CSF_ASSOCIATE) return fail("unknown flag bits " + std::to_string(flags & ~(uint32_t)HT_CSF_ASSOCIATE));
    if (!(min_confidence == min_confidence)) return fail("min_confidence is NaN");
    for (int32_t i = 0; i < n; i++)
        if (pairs[i].frame < 0 || pairs[i].frame >= grouped_frames)
            return fail("pair " + std::to_string(i) + ": frame " + std::to_string(pairs[i].frame) + " is outside the device-grouped batch");
    // bucket the pairs by frame, keeping list order inside a frame: counts, then the groups in ascending frame, then the scatter
    std::vector<int32_t> group_of((size_t)(grouped_frames > 0 ? grouped_frames : 0), 0);
    for (int32_t i = 0; i < n; i++)
        if (++group_of[(size_t)pairs[i].frame] > HT_CSF_MAX_SLOTS)
            return fail("frame " + std::to_string(pairs[i].frame) + " has more than " + std::to_string(HT_CSF_MAX_SLOTS) + " slots (pair " + std::to_string(i) + ")");
    plan->groups.clear();
    int32_t first = 0;
    for (int32_t f = 0; f < grouped_frames; f++) {
        const int32_t count = group_of[(size_t)f];
        if (!count) continue;
        group_of[(size_t)f] = plan->ngroups();
        plan->groups.insert(plan->groups.end(), {f, first, 0});  // the count doubles as the scatter cursor
        first += count;
    }
    plan->order.assign((size_t)n, 0);
    for (int32_t i = 0; i < n; i++) {
        int32_t *g = &plan->groups[3 * (size_t)group_of[(size_t)pairs[i].frame]];
        plan->order[(size_t)(g[1] + g[2]++)] = i;
    }
    return HT_OK;
}
