// ht_cascade_plan.h — the host side of a cascade: the "HTCB" blob checked and turned into the tables the scan kernels read
// (ht_cascade_types.h).  Plain C++17, no HIP: ht_create (ht_context.hip) plans and uploads, tests/host/cascade_plan_harness.cc compiles
// this header with g++ and the sanitizers.  Two calls, because the deep tail depends on ht_config.options and a bad blob is reported
// before a bad option string:
//   ht_plan_cascade        the blob -> everything that does not depend on the hand-off stage
//   ht_plan_cascade_split  whether the blob is the built-in one + option split -> split_stage and the packed tail
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "ht_cascade_types.h"

// ---------------------------------------------------------------------------------------------------------
// The blob: header {magic, version, nstages, cw, ch, nfeat, maxpts, 0}, stage rows, feature rows.
inline bool ht_parse_cascade(const uint8_t *blob, size_t len, HtCascadePlan *c, std::string &why) {
    if (!blob || len < 32 || std::memcmp(blob, "HTCB", 4) != 0) {
        why = "cascade blob: bad magic";
        return false;
    }
    uint32_t h[8];
    std::memcpy(h, blob, 32);
    if (h[1] != 1 || h[6] != HT_MAXPTS) {
        why = "cascade blob: unsupported version";
        return false;
    }
    c->nstages = h[2];
    c->cw = h[3];
    c->ch = h[4];
    c->nfeat = h[5];
    if (c->nstages == 0 || c->nstages > 63 || c->cw < 4 || c->ch < 4 || c->cw > 64 || c->ch > 64) {
        why = "cascade blob: unsupported stage count or window size";
        return false;
    }
    if (len != 32 + (size_t)c->nstages * sizeof(HtBlobStage) + (size_t)c->nfeat * sizeof(HtBlobFeature)) {
        why = "cascade blob: truncated";
        return false;
    }
    c->stages.resize(c->nstages);
    c->feats.resize(c->nfeat);
    std::memcpy(c->stages.data(), blob + 32, c->nstages * sizeof(HtBlobStage));
    if (c->nfeat) std::memcpy(c->feats.data(), blob + 32 + c->nstages * sizeof(HtBlobStage), c->nfeat * sizeof(HtBlobFeature));
    uint32_t first = 0;
    for (uint32_t j = 0; j < c->nstages; j++) {
        if (c->stages[j].first != first || first + c->stages[j].count > c->nfeat) {
            why = "cascade blob: inconsistent stage table";
            return false;
        }
        first += c->stages[j].count;
    }
    for (uint32_t k = 0; k < c->nfeat; k++) {
        const HtBlobFeature &f = c->feats[k];
        // the reference reads slot 0 of both polarities unconditionally (ccv.js:191-192)
        if (f.size == 0 || f.size > HT_MAXPTS || f.pz[0] < 0 || f.nz[0] < 0) {
            why = "cascade blob: feature without a valid first point";
            return false;
        }
        for (int q = 0; q < f.size; q++) {
            const int lim[3] = {(int)c->cw, (int)c->cw / 2, (int)c->cw / 4};
            const int limy[3] = {(int)c->ch, (int)c->ch / 2, (int)c->ch / 4};
            if (f.pz[q] > 2 || f.nz[q] > 2 ||
                (f.pz[q] >= 0 && (f.px[q] < 0 || f.py[q] < 0 || f.px[q] >= lim[f.pz[q]] || f.py[q] >= limy[f.pz[q]])) ||
                (f.nz[q] >= 0 && (f.nx[q] < 0 || f.ny[q] < 0 || f.nx[q] >= lim[f.nz[q]] || f.ny[q] >= limy[f.nz[q]]))) {
                why = "cascade blob: feature point outside the window";
                return false;
            }
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// The pieces every table is made of.

// The valid points (z >= 0) of one polarity of a feature, in slot order: what ccv.js:189-220 looks at.  n >= 1 (the parser insists on slot 0).
struct HtPoints {
    int n = 0;
    int x[HT_MAXPTS], y[HT_MAXPTS], z[HT_MAXPTS];
};
inline HtPoints ht_points(const HtBlobFeature &f, bool negative) {
    HtPoints p;
    const int8_t *x = negative ? f.nx : f.px, *y = negative ? f.ny : f.py, *z = negative ? f.nz : f.pz;
    for (int q = 0; q < f.size; q++)
        if (z[q] >= 0) p.x[p.n] = x[q], p.y[p.n] = y[q], p.z[p.n] = z[q], p.n++;
    return p;
}
// out[0, slots) = of(point): the slots past the last point repeat slot 0 (min / max are idempotent, the kernels read them all)
template <typename T, typename Of>
inline void ht_fill_slots(T *out, int slots, const HtPoints &p, Of of) {
    for (int q = 0; q < slots; q++) {
        const int j = q < p.n ? q : 0;
        out[q] = (T)of(p.x[j], p.y[j], p.z[j]);
    }
}

// k_scan_tiles: byte offset of a point from its window's base in the unified-base tile
inline uint16_t ht_tile_off(int x, int y, int z) { return (uint16_t)(z == 0 ? HT_O0(x, y) : z == 1 ? HT_O1(x, y) : HT_O2(x, y)); }
// k_scan_deep / k_scan_deep_lds: byte offset of a point in the window patch of a cw-wide window
inline uint16_t ht_patch_off(int x, int y, int z, int cw) {
    return (uint16_t)(z == 0 ? y * cw + x : z == 1 ? HT_PATCH1 + y * (cw / 2) + x : HT_PATCH2 + y * (cw / 4) + x);
}

// v * 1e8 as an integer: s the product, k = s rounded, exact iff (double)k / 1e8 == v — which holds iff the decimal literal had <= 8
// fractional digits
struct HtE8 {
    double s;
    int64_t k;
    bool exact;
};
inline HtE8 ht_e8(double v) {
    HtE8 e;
    e.s = v * 1e8;
    e.k = (int64_t)std::llround(e.s);
    e.exact = std::fabs(e.s) < 9.0e15 && (double)e.k / 1e8 == v;
    return e;
}
// The two 32-bit forms carry k in an int32_t, each under a range test of its own:
//   fp (tile offsets, the sparse phase adds a1i only):   0 < k1 < 2^31 and k0 == -k1
//   packed (patch offsets, both alphas are recovered):   |s| < 2.0e9

// ---------------------------------------------------------------------------------------------------------
// Everything that does not depend on the hand-off stage.  false: *why says what is wrong with the blob.
inline bool ht_plan_cascade(const uint8_t *blob, size_t len, HtCascadePlan *c, std::string *why) {
    if (!ht_parse_cascade(blob, len, c, *why)) return false;
    c->decimal_alphas = true;
    c->deep.resize(c->nfeat), c->tile.resize(c->nfeat), c->patch.resize(c->nfeat), c->fp.resize(c->nfeat);
    bool fp_ok = true;
    for (uint32_t k = 0; k < c->nfeat; k++) {
        const HtBlobFeature &f = c->feats[k];
        const HtPoints P = ht_points(f, false), N = ht_points(f, true);
        const HtE8 e0 = ht_e8(f.alpha[0]), e1 = ht_e8(f.alpha[1]);
        if (!e0.exact || !e1.exact) c->decimal_alphas = false;

        // coordinate form (k_scan_simple).  The integers are only read when the whole cascade is decimal; a1i stays 0 behind an alpha[0]
        // that is not exact
        HtDeepFeature &d = c->deep[k];
        ht_fill_slots(d.px, HT_MAXPTS, P, [](int x, int, int) { return x; });
        ht_fill_slots(d.py, HT_MAXPTS, P, [](int, int y, int) { return y; });
        ht_fill_slots(d.pz, HT_MAXPTS, P, [](int, int, int z) { return z; });
        ht_fill_slots(d.nx, HT_MAXPTS, N, [](int x, int, int) { return x; });
        ht_fill_slots(d.ny, HT_MAXPTS, N, [](int, int y, int) { return y; });
        ht_fill_slots(d.nz, HT_MAXPTS, N, [](int, int, int z) { return z; });
        d.a0 = f.alpha[0], d.a1 = f.alpha[1];
        d.a0i = e0.exact ? e0.k : 0;
        d.a1i = e0.exact && e1.exact ? e1.k : 0;

        // LDS-offset form for k_scan_tiles (unified-base layout, see ht_scan.hip): the valid points first, the other slots 0
        HtTileFeature &t = c->tile[k];
        t = HtTileFeature{};
        for (int q = 0; q < P.n; q++) t.po[q >> 1] |= (uint32_t)ht_tile_off(P.x[q], P.y[q], P.z[q]) << (16 * (q & 1));
        for (int q = 0; q < N.n; q++) t.no[q >> 1] |= (uint32_t)ht_tile_off(N.x[q], N.y[q], N.z[q]) << (16 * (q & 1));
        t.np = (uint32_t)P.n, t.nn = (uint32_t)N.n;
        std::memcpy(&t.a[0], &f.alpha[0], 8);
        std::memcpy(&t.a[2], &f.alpha[1], 8);

        // packed per-lane form of the same offsets for the tile kernel's feature-parallel sparse phase, alpha[2k+1] * 1e8 as the integer
        // the generated stages add
        if (P.n > 5 || N.n > 5 || !(e1.k > 0 && e1.k < (1ll << 31) && e0.k == -e1.k)) fp_ok = false;
        if (fp_ok) {
            HtPackedFeature &q = c->fp[k];
            q = HtPackedFeature{};
            ht_fill_slots(q.off, 5, P, ht_tile_off);
            ht_fill_slots(q.off + 5, 5, N, ht_tile_off);
            q.a0i = (int32_t)e0.k, q.a1i = (int32_t)e1.k;
        }

        // patch-offset form for k_scan_deep; its integers are the rounded products whatever the alphas are
        HtPatchFeature &p = c->patch[k];
        p = HtPatchFeature{};
        const int cw = (int)c->cw;
        ht_fill_slots(p.poff, HT_MAXPTS, P, [cw](int x, int y, int z) { return ht_patch_off(x, y, z, cw); });
        ht_fill_slots(p.noff, HT_MAXPTS, N, [cw](int x, int y, int z) { return ht_patch_off(x, y, z, cw); });
        p.a0 = f.alpha[0], p.a1 = f.alpha[1];
        p.a0i = e0.k, p.a1i = e1.k;
    }
    c->dev_stages.resize(c->nstages);
    for (uint32_t j = 0; j < c->nstages; j++) {
        HtDevStage &s = c->dev_stages[j];
        s.first = c->stages[j].first;
        s.count = c->stages[j].count;
        s.threshold = c->stages[j].threshold;
        s.pad = 0;
        const HtE8 e = ht_e8(s.threshold);
        s.thri = e.exact ? e.k : 0;
        if (!e.exact) c->decimal_alphas = false;
        s.maxpts = 1;
        // The integer decision "S < thri  <=>  the reference's binary64 sum < threshold" (off an exact tie) needs the
        // rounding error of the reference's SEQUENTIAL sum to stay below half the 1e-8 grid: |err| <= count * 2^-52 *
        // sum|alpha|.  True for the trained cascade (alphas O(1): bound ~1e-11); a custom cascade with huge alphas takes
        // the sequential binary64 path everywhere instead of silently diverging from ccv.js:186-222.
        double sabs = 0.0;
        for (uint32_t k = 0; k < s.count; k++) {
            s.maxpts = std::max(s.maxpts, std::max(c->tile[s.first + k].np, c->tile[s.first + k].nn));
            const HtBlobFeature &f = c->feats[s.first + k];
            sabs += std::max(std::fabs(f.alpha[0]), std::fabs(f.alpha[1]));
        }
        if (!((double)s.count * 2.220446049250313e-16 * (sabs + std::fabs(s.threshold)) < 0.5e-8)) c->decimal_alphas = false;
    }
    if (!fp_ok || !c->decimal_alphas) c->fp.clear();
    return true;
}

// The hand-off stage and the LDS-resident deep table: the features of stages [split, nstages) in HtPackedFeature form; `packed` stays
// empty when the cascade does not fit the format (then k_scan_deep is used).
inline void ht_plan_cascade_split(HtCascadePlan *c, bool builtin, int opt_split) {
    // stages [0, split) always run in the tile kernel: the generated straight-line stages for the built-in cascade
    c->split_stage = std::min<uint32_t>(builtin ? 8u : 4u, c->nstages);
    if (opt_split > 0)  // option split: hand-off stage (<= 8 for the generated stage code)
        c->split_stage = std::min<uint32_t>((uint32_t)opt_split, std::min<uint32_t>(builtin ? 8u : c->nstages, c->nstages));
    c->packed.clear();
    c->packed_first = 0;
    if (!c->decimal_alphas || c->split_stage >= c->nstages || c->cw != 24 || c->ch != 24) return;
    const uint32_t first = c->stages[c->split_stage].first;
    const uint32_t n = c->nfeat - first;
    if (n == 0 || n * sizeof(HtPackedFeature) > HT_DEEP_LDS_TABLE_BYTES) return;
    std::vector<HtPackedFeature> pk(n);
    for (uint32_t k = 0; k < n; k++) {
        const HtBlobFeature &f = c->feats[first + k];
        const HtPoints P = ht_points(f, false), N = ht_points(f, true);
        const HtE8 e0 = ht_e8(f.alpha[0]), e1 = ht_e8(f.alpha[1]);  // exact: the cascade is decimal
        if (P.n > 5 || N.n > 5 || !(std::fabs(e0.s) < 2.0e9) || !(std::fabs(e1.s) < 2.0e9)) return;
        HtPackedFeature &t = pk[k];
        t = HtPackedFeature{};
        ht_fill_slots(t.off, 5, P, [](int x, int y, int z) { return ht_patch_off(x, y, z, 24); });
        ht_fill_slots(t.off + 5, 5, N, [](int x, int y, int z) { return ht_patch_off(x, y, z, 24); });
        t.a0i = (int32_t)e0.k, t.a1i = (int32_t)e1.k;
    }
    c->packed.swap(pk);
    c->packed_first = first;
}
