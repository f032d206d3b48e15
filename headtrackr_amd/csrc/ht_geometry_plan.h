// ht_geometry_plan.h — the plan of one geometry, computed on the host: level sizes and arena offsets, the resample jobs by generation
// with their k_resample / k_resample_bands tile records in launch order, the tail kernel's jobs and tap tables, the scan scales and
// tile records, the early-scan split and the survivor queue's capacity.  Plain C++ (no HIP, no device call): ht_context.hip calls
// ht_plan_geometry and uploads the tables as they are; tests/host/geometry_plan_harness.cc compiles the SAME file with
// g++ -fsanitize=address,undefined, compares its tables with the recorded ones and checks what the kernels rely on.
// Compiled with -ffp-contract=off like the kernels, so no binary64 operation is fused.
//
// Reference behaviour restated here:
//   geometry            ccv.js:110-147      (scale, scale_upto, level sizes, variant planes)
//   scan scales         ccv.js:154-160
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ht_hostpost.h"  // ht_scale_pow
#include "ht_plan_types.h"

static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// rs_tap (ht_resample_tap.h) on the host: the same binary64 operations in the same order (this file is compiled with
// -ffp-contract=off like the kernels, so nothing is fused)
static HtTap ht_host_tap(int i, double r, int s, int origin) {
    double f = ((double)i + 0.5) * r;
    f = f + (-0.5);
    f = f < 0.0 ? 0.0 : f;
    const double fmax = (double)(s - 1);
    f = f > fmax ? fmax : f;
    const double af = std::floor(f);
    HtTap tp;
    tp.a = origin + (int)af;
    tp.b = origin + std::min((int)af + 1, s - 1);
    tp.t = f - af;
    tp.u = 1.0 - tp.t;
    return tp;
}

// level_dims as ht_set_geometry takes them (n levels, 2 n values; checked on the host before the current geometry is torn down):
// level 0 is the frame, no level is negative or larger than the frame, and level i + next is at most HALF of level i, floor(size / 2) in
// both directions — ccv's own rule (ccv.js:126-127) with "at most" in place of "equal".  The scan relies on the last one and nothing on the
// device clamps it: scale i takes its windows from level i + 2 next (qw = its width - cw / 4) and reads the same window at twice the
// coordinates on level i + next and at four times on level i.  k_scan_simple, k_scan_deep and k_scan_deep_lds address those bytes straight
// from the window origin (HT_WIN_SETUP: o0 = off + (4 y + 2 dy) stride + 4 x + 2 dx, ...), with no test against the plane's width or
// height, so a level i + next wider or taller than half of level i puts the last windows' rows past the end of level i: into the planes
// behind it, and for the last frame of a batch past the arena.  k_scan_tiles stages only rows and columns inside the planes (its loads are
// predicated on L0.h / L1.h / the strides and clamped into L2), so there the same windows would read LDS bytes no load has written.
// The resample kernels need no such relation: every tap is clamped into its source rect.
static ht_status ht_check_level_dims(int next, int width, int height, const int32_t *level_dims, int n, std::string *why) {
    for (int i = 0; i < n; i++) {
        const int lw = level_dims[2 * i], lh = level_dims[2 * i + 1];
        if (lw < 0 || lh < 0 || lw > width || lh > height || (i == 0 && (lw != width || lh != height)))
            return *why = "ht_set_geometry: bad level_dims", HT_ERR_INVALID;
    }
    for (int i = 0; i + next < n; i++) {
        const int j = i + next;
        if (level_dims[2 * j] > level_dims[2 * i] / 2 || level_dims[2 * j + 1] > level_dims[2 * i + 1] / 2) {
            *why = "ht_set_geometry: level_dims: level " + std::to_string(j) + " (" + std::to_string(level_dims[2 * j]) + "x" + std::to_string(level_dims[2 * j + 1]) +
                   ") is larger than half of level " + std::to_string(i) + " (" + std::to_string(level_dims[2 * i]) + "x" + std::to_string(level_dims[2 * i + 1]) +
                   "): the scan reads a window on levels i, i + next, i + 2 next at 4, 2 and 1 times its coordinates";
            return HT_ERR_INVALID;
        }
    }
    return HT_OK;
}

// level sizes, arena offsets, pyr_bytes and arena_stride
static ht_status ht_plan_levels(const HtPlanInputs &in, int width, int height, const int32_t *level_dims, int n, HtGeometryPlan *p, std::string *why) {
    const int next = in.next;
    uint64_t off = 0;
    p->pyr_bytes = 0;
    for (int i = 0; i < n; i++) {
        HtDevLevel &L = p->levels[i];
        if (level_dims) {  // validated by ht_set_geometry (ht_check_level_dims)
            L.w = level_dims[2 * i];
            L.h = level_dims[2 * i + 1];
        } else if (i == 0) {
            L.w = width;
            L.h = height;
        } else if (i <= in.interval) {  // ccv.js:119-120
            L.w = (int)std::floor((double)width / ht_scale_pow(in.interval, i));
            L.h = (int)std::floor((double)height / ht_scale_pow(in.interval, i));
        } else {  // ccv.js:126-127
            L.w = p->levels[i - next].w / 2;
            L.h = p->levels[i - next].h / 2;
        }
        L.stride = (int)align_up((uint64_t)L.w, 4);
        for (int s = 0; s < 4; s++) {
            if (s == 0 || i >= 2 * next) {  // ccv.js:131
                if (off > 0xfffffff0ull) return *why = "ht_set_geometry: frame too large", HT_ERR_INVALID;
                L.off[s] = (uint32_t)off;
                off = align_up(off + (uint64_t)L.stride * L.h, 256);
                p->pyr_bytes += (uint64_t)L.w * L.h;
            } else {
                L.off[s] = 0xffffffffu;
            }
        }
    }
    p->arena_stride = align_up(off + 256, 256);
    return HT_OK;
}

// resample jobs by dependency generation (generation 0 = the gray plane itself); gen[i] = generation of level i
static void ht_plan_jobs(const HtPlanInputs &in, int n, HtGeometryPlan *p, std::vector<int> &gen) {
    const int next = in.next;
    gen.assign(n, 0);
    int ngen = 1;
    for (int i = 1; i < n; i++) {
        gen[i] = (i <= in.interval) ? 1 : gen[i - next] + 1;
        ngen = std::max(ngen, gen[i] + 1);
    }
    p->gens.assign(ngen, {});
    auto add_job = [&](int g, int src, int dst, int slot, int sx, int sy, int sw, int sh, int dw, int dh) {
        const HtDevLevel &S = p->levels[src], &D = p->levels[dst];
        if (D.w <= 0 || D.h <= 0) return;
        HtResampleJob j;
        std::memset(&j, 0, sizeof(j));
        j.src_off = S.off[0];
        j.dst_off = D.off[slot];
        j.src_stride = S.stride;
        j.dst_stride = D.stride;
        j.sx = sx, j.sy = sy, j.sw = sw, j.sh = sh;
        j.dw = dw, j.dh = dh;
        j.cw = D.w, j.ch = D.h;
        if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0) {  // nothing is drawn: the canvas stays transparent black
            j.dw = j.dh = 0;
            j.sw = j.sh = 1;
            j.rx = j.ry = 1;
        } else {
            j.rx = (double)sw / (double)dw;
            j.ry = (double)sh / (double)dh;
        }
        p->gens[g].push_back(j);
    };
    for (int i = 1; i < n; i++) {
        const HtDevLevel &D = p->levels[i];
        if (i <= in.interval) {  // ccv.js:121
            add_job(gen[i], 0, i, 0, 0, 0, p->levels[0].w, p->levels[0].h, D.w, D.h);
        } else {  // ccv.js:128
            const HtDevLevel &S = p->levels[i - next];
            add_job(gen[i], i - next, i, 0, 0, 0, S.w, S.h, D.w, D.h);
            if (i >= 2 * next) {  // ccv.js:135,140,145
                add_job(gen[i], i - next, i, 1, 1, 0, S.w - 1, S.h, D.w - 2, D.h);
                add_job(gen[i], i - next, i, 2, 0, 1, S.w, S.h - 1, D.w, D.h - 2);
                add_job(gen[i], i - next, i, 3, 1, 1, S.w - 1, S.h - 1, D.w - 2, D.h - 2);
            }
        }
    }
}

// k_resample tile records of one generation's jobs, in launch order: 64 columns x np passes of 16 rows.  np is bounded by the LDS source
// window (the rows a tile touches: ~16 np ry + 3 <= HT_RS_SRC_ROWS; the kernel falls back to HBM taps if a tile still does not fit)
// and by rs_rpt; a canvas of P = ceil(ch / 16) passes is then cut into ceil(P / np) tiles of near-equal pass counts.
static std::vector<HtResampleJob> ht_plan_gen_tiles(const HtPlanInputs &in, const std::vector<HtResampleJob> &jobs) {
    std::vector<HtResampleJob> tiles;
    for (auto &j : jobs) {
        int npmax = 1;
        for (int t = 2; t <= std::min(in.rs_rpt, HT_RS_MAX_PASSES); t++)
            if ((int)std::ceil(16.0 * t * j.ry) + 3 <= HT_RS_SRC_ROWS) npmax = t;
        const int passes = (j.ch + 15) / 16, nby = (passes + npmax - 1) / npmax, nbx = (j.cw + 63) / 64;
        int pass0 = 0;
        for (int y = 0; y < nby; y++) {
            const int np = passes / nby + (y < passes % nby ? 1 : 0);
            for (int x = 0; x < nbx; x++) {
                HtResampleJob t = j;
                t.bx = (uint16_t)x, t.pass0 = (uint16_t)pass0, t.np = (uint16_t)np;
                // bit 0: exact 2:1 in both directions (2x2 box mean, see the BOX rows of k_resample); option rs_nofast keeps
                // every pixel on the declared binary64 sequence (A/B and cross-check)
                t.pad = in.rs_nofast ? 2 : (uint16_t)((j.dw > 0 && j.sw == 2 * j.dw && j.sh == 2 * j.dh) ? 1 : 0);
                const int X0 = 64 * x, Y0 = 16 * pass0, ncols = std::min(64, j.dw - X0), nrows = std::min(16 * np, j.dh - Y0);
                if (ncols > 0 && nrows > 0) {  // the source extent k_resample stages into LDS (same expressions as in the kernel)
                    t.ex_xa = ht_host_tap(X0, j.rx, j.sw, j.sx).a & ~15;
                    t.ex_ya = ht_host_tap(Y0, j.ry, j.sh, j.sy).a;
                    t.ex_sw16 = (ht_host_tap(X0 + ncols - 1, j.rx, j.sw, j.sx).b - t.ex_xa) / 16 + 1;
                    t.ex_sh = ht_host_tap(Y0 + nrows - 1, j.ry, j.sh, j.sy).b - t.ex_ya + 1;
                    // k_resample_bands: the source rows of each wavefront's quarter of the tile (rows beyond the drawn ones read the
                    // last drawn row's taps, as in the kernel)
                    bool fit = t.ex_sw16 * 16 <= 160;
                    for (int w = 0; w < 4; w++) {
                        const int r0 = std::min(4 * np * w, nrows - 1), r1 = std::min(4 * np * (w + 1) - 1, nrows - 1);
                        const int bya = ht_host_tap(Y0 + r0, j.ry, j.sh, j.sy).a - t.ex_ya;
                        const int bsh = ht_host_tap(Y0 + r1, j.ry, j.sh, j.sy).b - (t.ex_ya + bya) + 1;
                        if (bya < 0 || bya > 255 || bsh < 1 || bsh > HT_RSB_ROWS) fit = false;
                        t.band_ya4 |= (uint32_t)(bya & 0xff) << (8 * w), t.band_sh4 |= (uint32_t)(bsh & 0xff) << (8 * w);
                    }
                    if (fit) t.pad |= 4;
                }
                tiles.push_back(t);
            }
            pass0 += np;
        }
    }
    // launch order = source order: tiles of different drawImage calls that read the same rows of the same source
    // plane (levels 1..6 all read level 0; the four variants of a level read the same parent) run back to back on
    // an XCD, so the source band is fetched from HBM once and then served by that XCD's L2
    if (!in.rs_nosort)
        std::stable_sort(tiles.begin(), tiles.end(), [](const HtResampleJob &a, const HtResampleJob &b) {
            if (a.src_off != b.src_off) return a.src_off < b.src_off;
            const int ya = (int)(16.0 * a.pass0 * a.ry), yb = (int)(16.0 * b.pass0 * b.ry);
            if (ya / 32 != yb / 32) return ya < yb;
            return a.bx < b.bx;
        });
    return tiles;
}

// tail plan: from the first generation g0 on which every generation has <= HT_TAIL_MAX_JOBS jobs and all of them
// together <= tail_cap destination pixels per frame, one workgroup per frame does the rest of the pyramid in one launch
// (k_resample_tail) instead of one nearly empty launch per generation.
static void ht_plan_tail(const HtPlanInputs &in, int max_batch, HtGeometryPlan *p) {
    const int ngen = (int)p->gens.size();
    constexpr int HT_SMALL_BATCH = 48;
    // Small batches (a live feed's frame, the 8 feeds of a streaming step) are latency chains, not throughput: the tail kernel is ONE
    // workgroup per frame walking its generations behind barriers — 21 us for 17 k pixels of a single 320x240 frame, the longest kernel
    // of the call —, while a k_resample_bands launch of the same generation is 4.5 us on the otherwise idle chip.  rocprofv3 kernel
    // trace of single-frame calls (tools/gpu_one_frame_trace.sh, round 6): cap 32 768 -> 4 000 pixels takes 74.1 -> 63.5 us off the
    // device span at 320x240 (generation 4 as a launch, generations 5 - 7 in the tail) and 92.9 -> 79.3 us at 1920x1080 (no tail at all);
    // batches that fill the chip keep the large cap (C2: cap 4 000 costs +3 % on the pyramid, no tail at all +19 %).  Where it ends, pipelined
    // (three batches of 320x240 in flight / two of 1280x720, small plan against large): 24 frames +11 %, 32 +10.6 %, 48 +9.5 %, 64 +-0 %, 128 +-0 %;
    // 720p: 16 frames +2 %, 32 +3 %.
    const uint64_t tail_cap = in.rs_tailcap_forced ? in.rs_tailcap : (max_batch <= HT_SMALL_BATCH ? 4000u : in.rs_tailcap);
    // which tail kernel: measured (3 batches in flight), the table-driven binary32 tail (68 VGPRs, 35 KB LDS) is worth +4-5 % at
    // 128 x 720p but costs 3 % at 256 x 320x240, where its grid puts a 1024-thread workgroup on EVERY CU and its footprint keeps
    // the other batches' kernels from sharing them; the round-1 binary64 tail (41 VGPRs) is kept for batches that cover the chip.
    // Larger caps (generation 3 of C2 = 54 k pixels in the tail) lose with either kernel.
    // ... and for a handful of frames: 7.6 us against the table form's 10.3 for generations 5 - 7 of a single 320x240 frame (the same trace)
    p->tail_table = in.tail_table_forced ? in.tail_table : ((max_batch <= 128 && max_batch > HT_SMALL_BATCH) ? 1 : 0);
    p->tail_first_gen = 0;
    if (in.rs_notail) return;
    int g0 = ngen;
    uint64_t px = 0;
    for (int g = ngen - 1; g >= 1; g--) {
        uint64_t gp = 0;
        for (auto &j : p->gens[g]) gp += (uint64_t)j.cw * j.ch;
        if (p->gens[g].size() > (size_t)HT_TAIL_MAX_JOBS || px + gp > tail_cap) break;
        px += gp;
        g0 = g;
    }
    if (!(ngen - g0 >= 2 && ngen - g0 <= HT_TAIL_MAX_GENS)) return;
    std::vector<HtResampleJob> &tj = p->tail_jobs;
    std::vector<uint32_t> &pref = p->tail_prefix;
    HtTailGens &T = p->tail;
    std::memset(&T, 0, sizeof(T));
    T.ngen = ngen - g0;
    for (int g = g0; g < ngen; g++) {
        T.job_begin[g - g0] = (int32_t)tj.size();
        uint32_t groups = 0;
        for (auto &j : p->gens[g]) {
            tj.push_back(j);
            pref.push_back(groups);
            groups += (uint32_t)((j.cw + 3) / 4) * (uint32_t)j.ch;
        }
        T.groups[g - g0] = groups;
    }
    T.job_begin[T.ngen] = (int32_t)tj.size();
    if (tj.empty()) return;
    // tap tables: the geometry is the same for every frame, so the taps are computed once here
    std::vector<HtTap> &taps = p->tail_taps;
    std::vector<HtTapFast> &fast = p->tail_taps_fast;
    std::vector<HtTailTapRef> &refs = p->tail_tapref;
    const bool nofast = in.rs_nofast;
    size_t jidx = 0;
    for (auto &j : tj) {
        for (int g = 0; g <= T.ngen; g++)
            if ((size_t)T.job_begin[g] == jidx) T.tap_begin[g] = (uint32_t)taps.size();
        jidx++;
        HtTailTapRef r;
        r.col = (uint32_t)taps.size();
        const int ncol = std::max(j.dw, 1), nrow = std::max(j.dh, 1);
        for (int i = 0; i < ncol + 3; i++) taps.push_back(ht_host_tap(std::min(i, ncol - 1), j.rx, j.sw, j.sx));
        r.row = (uint32_t)taps.size();
        for (int i = 0; i < nrow; i++) taps.push_back(ht_host_tap(i, j.ry, j.sh, j.sy));
        r.mode = nofast ? 2u : ((j.dw > 0 && j.sw == 2 * j.dw && j.sh == 2 * j.dh) ? 1u : 0u);
        r.pad = 0;
        refs.push_back(r);
    }
    T.tap_begin[T.ngen] = (uint32_t)taps.size();
    fast.resize(taps.size());
    for (size_t i = 0; i < taps.size(); i++) fast[i].a = taps[i].a, fast[i].tf = (float)taps[i].t;
    p->tail_first_gen = g0;
}

// per-scale tiling of the scan: scales, k_scan_tiles tile records and their magic divisors
static ht_status ht_plan_scan_tiles(const HtPlanInputs &in, int upto, HtGeometryPlan *p, std::string *why) {
    constexpr int TXH = HT_SCAN_TXH, TYH = HT_SCAN_TYH;
    p->scales.clear();
    p->windows_per_frame = 0;
    uint32_t tiles = 0;
    for (int i = 0; i < upto; i++) {  // ccv.js:154
        HtScanScale S;
        std::memset(&S, 0, sizeof(S));
        S.l0 = i;
        S.l1 = i + in.next;
        S.l2 = i + 2 * in.next;
        S.qw = p->levels[S.l2].w - (int)(in.cw / 4);  // ccv.js:155
        S.qh = p->levels[S.l2].h - (int)(in.ch / 4);  // ccv.js:156
        if (S.qw <= 0 || S.qh <= 0) continue;
        S.ntx = (2 * S.qw + TXH - 1) / TXH;
        S.tw2 = (2 * S.qw + S.ntx - 1) / S.ntx;
        S.tw2 = (S.tw2 + 7) & ~7;  // multiple of 8 half-steps: tile rows start on 16 / 8 / 4-byte boundaries of the three planes' rows
        S.nty = (2 * S.qh + TYH - 1) / TYH;
        S.th2 = (2 * S.qh + S.nty - 1) / S.nty;
        S.th2 += S.th2 & 1;
        S.ntx = (2 * S.qw + S.tw2 - 1) / S.tw2;
        S.nty = (2 * S.qh + S.th2 - 1) / S.th2;
        S.tile_begin = tiles;
        S.div_magic = ((1u << 20) + (uint32_t)S.tw2 - 1) / (uint32_t)S.tw2;
        if (p->windows_per_frame + 4ull * S.qw * S.qh > 0xffffffffull) return *why = "frame too large", HT_ERR_INVALID;
        S.win_begin = (uint32_t)p->windows_per_frame;
        tiles += (uint32_t)(S.ntx * S.nty);
        p->windows_per_frame += 4ull * (uint64_t)S.qw * (uint64_t)S.qh;
        p->scales.push_back(S);
    }
    p->tiles_per_frame = tiles;
    std::vector<HtTileRec> &recs = p->tile_recs;
    for (const HtScanScale &S : p->scales) {
        const HtDevLevel &A = p->levels[S.l0], &B = p->levels[S.l1], &Cq = p->levels[S.l2];
        if (A.stride > 0xffff || A.h > 0xffff) return *why = "frame too large", HT_ERR_INVALID;
        for (int y = 0; y < S.nty; y++)
            for (int x = 0; x < S.ntx; x++) {
                HtTileRec r;
                std::memset(&r, 0, sizeof(r));
                const int X0 = x * S.tw2, Y0 = y * S.th2;
                r.off0 = A.off[0], r.off1 = B.off[0];
                for (int q = 0; q < 4; q++) r.off2[q] = Cq.off[q];
                r.sh0 = (uint32_t)A.stride | (uint32_t)A.h << 16;
                r.sh1 = (uint32_t)B.stride | (uint32_t)B.h << 16;
                r.sh2 = (uint32_t)Cq.stride | (uint32_t)Cq.h << 16;
                r.origin = (uint32_t)X0 | (uint32_t)Y0 << 16;
                r.size = (uint32_t)std::min(S.tw2, 2 * S.qw - X0) | (uint32_t)std::min(S.th2, 2 * S.qh - Y0) << 16;
                r.tw2_l0 = (uint32_t)S.tw2 | (uint32_t)S.l0 << 16;
                r.div_magic = S.div_magic;
                {  // n / (4 * th) == (n * magic) >> 24 for every pair index n of the tile (n <= 1024, 4 * th <= 128: error term n * 127 < 2^24 / 128); checked anyway
                    const uint32_t th = r.size >> 16, d = 4u * th;
                    r.strip_magic = ((1u << 24) + d - 1u) / d;
                    for (uint32_t n = 0; n < (uint32_t)(S.tw2 / 2) * th; n++)
                        if (((n * r.strip_magic) >> 24) != n / d) return *why = "tile plan: strip_magic is not exact", HT_ERR_INVALID;
                }
                recs.push_back(r);
            }
    }
    return HT_OK;
}

// early scan plan: scale i needs levels i, i + next, i + 2 next; the leading scales whose last plane is finished after
// generation 2 (interval 5: scale 0 = ~30 % of the windows) can start while generations 3.. are still being built
static void ht_plan_early_split(const HtPlanInputs &in, const std::vector<int> &gen, HtGeometryPlan *p) {
    const int ngen = (int)p->gens.size();
    p->early_gen = 0;
    p->early_tiles = 0;
    if (in.early_scan && in.aux_stream && ngen > 3 && (p->tail_first_gen == 0 || p->tail_first_gen > 2)) {
        uint32_t tiles = 0;
        for (auto &S : p->scales) {
            if (gen[S.l2] > 2) break;
            tiles += (uint32_t)(S.ntx * S.nty);
        }
        if (tiles > 0 && tiles < p->tiles_per_frame) p->early_gen = 2, p->early_tiles = tiles;
    }
}

// Plans one geometry: n levels (level_dims: their sizes, or nullptr for ccv's), scan scales [0, upto).  *plan is rebuilt from nothing;
// on a status other than HT_OK *why says what is wrong and the plan is of no use.
static ht_status ht_plan_geometry(const HtPlanInputs &in, int width, int height, int max_batch, const int32_t *level_dims, int n, int upto,
                                  HtGeometryPlan *plan, std::string *why) {
    *plan = HtGeometryPlan();
    ht_status st = ht_plan_levels(in, width, height, level_dims, n, plan, why);
    if (st != HT_OK) return st;
    std::vector<int> gen;
    ht_plan_jobs(in, n, plan, gen);
    const int ngen = (int)plan->gens.size();
    plan->gen_tiles.assign(ngen, {});
    plan->gen_blocks.assign(ngen, 0);
    for (int g = 1; g < ngen; g++) {
        plan->gen_tiles[g] = ht_plan_gen_tiles(in, plan->gens[g]);
        plan->gen_blocks[g] = (uint32_t)plan->gen_tiles[g].size();
    }
    ht_plan_tail(in, max_batch, plan);
    if ((st = ht_plan_scan_tiles(in, upto, plan, why)) != HT_OK) return st;
    ht_plan_early_split(in, gen, plan);
    // survivor queue between the tile kernel and the deep kernel: 1/8 of all windows unless configured
    uint64_t qc = in.queue_capacity_cfg ? in.queue_capacity_cfg : std::max<uint64_t>(1u << 16, plan->windows_per_frame * (uint64_t)max_batch / 8);
    qc = std::min<uint64_t>(qc, 1ull << 28);
    plan->queue_capacity = (uint32_t)qc;
    return HT_OK;
}
