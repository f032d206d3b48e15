// Host-only harness around headtrackr_amd/csrc/ht_cascade_plan.h (the cascade plan of ht_create), built by tests/test_cascade_plan_cpu.py
// with g++ -fsanitize=address,undefined.
//
//   cascade_plan_harness <cases>   one case per line: name blob-file builtin split   (tests/cascade_cases.py: manifest)
//     plans every case as ht_create does (ht_plan_cascade, then ht_plan_cascade_split), checks what the kernels rely on (check_plan below)
//     and prints one JSON object per line: status and message, the scalars, and the record count and CRC32 of each table as ht_create
//     uploads it; "inexact" counts the alphas and thresholds that are no multiple of 1e-8 (not part of the recorded results: it tells a
//     test which of the two reasons switched the integer decisions off)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>

#include "ht_cascade_plan.h"

static uint32_t crc32(const void *p, size_t n) {  // zlib's
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            tab[i] = c;
        }
    uint32_t c = 0xffffffffu;
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ b[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}
template <typename T>
static uint32_t crc_of(const std::vector<T> &v) {
    return v.empty() ? 0u : crc32(v.data(), v.size() * sizeof(T));
}

static std::string g_case;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "%s: %s: ", g_case.c_str(), #cond);  \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
            exit(3);                                              \
        }                                                         \
    } while (0)

struct Pt {
    int x, y, z;
    bool operator==(const Pt &o) const { return x == o.x && y == o.y && z == o.z; }
};
// the blob's valid points of one polarity, read here and not through the planner's ht_points
static std::vector<Pt> blob_points(const HtBlobFeature &f, bool negative) {
    std::vector<Pt> out;
    for (int q = 0; q < f.size; q++) {
        const Pt p = negative ? Pt{f.nx[q], f.ny[q], f.nz[q]} : Pt{f.px[q], f.py[q], f.pz[q]};
        if (p.z >= 0) out.push_back(p);
    }
    return out;
}
// what k_scan_tiles reads at window base + off: the tile layout of ht_scan.hip's header comment, inverted
static Pt tile_point(uint32_t off) {
    if (off < (uint32_t)HT_SCAN_P12_BASE) return Pt{(int)(off % HT_SCAN_PITCH0), (int)(off / HT_SCAN_PITCH0), 0};
    const uint32_t r = off - HT_SCAN_P12_BASE;
    if (r & 1) return Pt{(int)((r - 1) % (4 * HT_SCAN_PITCH0) / 4), (int)((r - 1) / (4 * HT_SCAN_PITCH0)), 2};
    return Pt{(int)(r % HT_SCAN_G_PITCH / 2), (int)(r / HT_SCAN_G_PITCH), 1};
}
// what the deep kernels read at patch + off.  The three regions only keep apart for windows up to 24x24 (the only ones the deep kernels
// run for: ht_launch_scan); for larger ones the plane is taken from the blob and the coordinates must still come back
static Pt patch_point(uint32_t off, int cw, int z_of_blob) {
    const int z = cw <= 24 ? (off < (uint32_t)HT_PATCH1 ? 0 : off < (uint32_t)HT_PATCH2 ? 1 : 2) : z_of_blob;
    const int base = z == 0 ? 0 : z == 1 ? HT_PATCH1 : HT_PATCH2, pitch = cw >> z;
    return Pt{(int)(off - base) % pitch, (int)(off - base) / pitch, z};
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// What the kernels rely on without checking it.
static void check_plan(const HtCascadePlan &P) {
    const bool w24 = P.cw == 24 && P.ch == 24, small = P.cw <= 24 && P.ch <= 24;
    CHECK(P.stages.size() == P.nstages && P.feats.size() == P.nfeat && P.dev_stages.size() == P.nstages, "rows");
    CHECK(P.deep.size() == P.nfeat && P.tile.size() == P.nfeat && P.patch.size() == P.nfeat && (P.fp.empty() || P.fp.size() == P.nfeat), "one record per feature");
    // the stages tile [0, nfeat), maxpts is the largest point count of the stage (the deep kernels read that many slots of every feature)
    uint32_t at = 0;
    for (uint32_t j = 0; j < P.nstages; j++) {
        const HtDevStage &s = P.dev_stages[j];
        CHECK(s.first == at && s.first == P.stages[j].first && s.count == P.stages[j].count && same_bits(s.threshold, P.stages[j].threshold) && s.pad == 0, "stage %u", j);
        at += s.count;
        uint32_t mp = 1;
        for (uint32_t k = 0; k < s.count; k++)
            mp = std::max<uint32_t>(mp, (uint32_t)std::max(blob_points(P.feats[s.first + k], false).size(), blob_points(P.feats[s.first + k], true).size()));
        CHECK(s.maxpts == mp, "stage %u: maxpts %u, the blob has %u", j, s.maxpts, mp);
        if (P.decimal_alphas) CHECK(same_bits((double)s.thri / 1e8, s.threshold), "stage %u: thri", j);
    }
    CHECK(at <= P.nfeat, "stages overrun the features");
    for (uint32_t k = 0; k < P.nfeat; k++) {
        const HtBlobFeature &f = P.feats[k];
        for (int neg = 0; neg < 2; neg++) {
            const std::vector<Pt> pts = blob_points(f, neg);
            const int n = (int)pts.size();
            CHECK(n >= 1 && n <= HT_MAXPTS, "feature %u: %d points", k, n);
            // tile form: np / nn points, the other slots 0
            const HtTileFeature &t = P.tile[k];
            CHECK((neg ? t.nn : t.np) == (uint32_t)n, "feature %u: tile count", k);
            const uint32_t *words = neg ? t.no : t.po;
            for (int q = 0; q < HT_MAXPTS; q++) {
                const uint32_t off = (words[q >> 1] >> (16 * (q & 1))) & 0xffffu;
                if (q >= n) {
                    CHECK(off == 0, "feature %u: tile slot %d past the points", k, q);
                    continue;
                }
                CHECK(tile_point(off) == pts[q], "feature %u: tile slot %d (offset %u) reads (%d, %d, %d), the blob has (%d, %d, %d)", k, q, off, tile_point(off).x, tile_point(off).y, tile_point(off).z, pts[q].x, pts[q].y, pts[q].z);
                if (w24) CHECK(off < (uint32_t)HT_SCAN_LDS_TILE_BYTES, "feature %u: tile slot %d outside the tile", k, q);
                if (!P.fp.empty()) CHECK(q >= 5 || P.fp[k].off[5 * neg + q] == off, "feature %u: fp slot %d", k, q);
            }
            // every slot of the forms whose kernels read them all: point q, past the points point 0
            const uint16_t *patch_off = neg ? P.patch[k].noff : P.patch[k].poff;
            for (int q = 0; q < HT_MAXPTS; q++) {
                const Pt want = pts[q < n ? q : 0];
                const HtDeepFeature &d = P.deep[k];
                const Pt got = neg ? Pt{d.nx[q], d.ny[q], d.nz[q]} : Pt{d.px[q], d.py[q], d.pz[q]};
                CHECK(got == want, "feature %u: deep slot %d", k, q);
                const uint32_t off = patch_off[q];
                CHECK(patch_point(off, (int)P.cw, want.z) == want, "feature %u: patch slot %d reads another point", k, q);
                if (small) CHECK(off < (uint32_t)HT_PATCH_BYTES, "feature %u: patch slot %d outside the patch", k, q);
            }
            if (!P.fp.empty()) {
                CHECK(n <= 5, "feature %u: fp with %d points", k, n);
                for (int q = n; q < 5; q++) CHECK(P.fp[k].off[5 * neg + q] == P.fp[k].off[5 * neg], "feature %u: fp slot %d does not repeat slot 0", k, q);
            }
        }
        CHECK(std::memcmp(&P.tile[k].a[0], &f.alpha[0], 8) == 0 && std::memcmp(&P.tile[k].a[2], &f.alpha[1], 8) == 0, "feature %u: tile alphas", k);
        CHECK(same_bits(P.deep[k].a0, f.alpha[0]) && same_bits(P.deep[k].a1, f.alpha[1]) && same_bits(P.patch[k].a0, f.alpha[0]) && same_bits(P.patch[k].a1, f.alpha[1]), "feature %u: alphas", k);
        // integers are read as the alphas wherever a kernel is told it may: the coordinate and patch forms under decimal_alphas, ...
        if (P.decimal_alphas) {
            CHECK(same_bits((double)P.deep[k].a0i / 1e8, f.alpha[0]) && same_bits((double)P.deep[k].a1i / 1e8, f.alpha[1]), "feature %u: deep integers", k);
            CHECK(same_bits((double)P.patch[k].a0i / 1e8, f.alpha[0]) && same_bits((double)P.patch[k].a1i / 1e8, f.alpha[1]), "feature %u: patch integers", k);
        }
        // ... fp whenever it exists (the sparse phase adds a1i for a fired feature and nothing otherwise: alpha[0] == -alpha[1])
        if (!P.fp.empty()) {
            CHECK(P.decimal_alphas && P.fp[k].a1i > 0 && P.fp[k].a0i == -P.fp[k].a1i && P.fp[k].pad == 0, "feature %u: fp alphas", k);
            CHECK(same_bits((double)P.fp[k].a1i / 1e8, f.alpha[1]) && same_bits((double)P.fp[k].a0i / 1e8, f.alpha[0]), "feature %u: fp integers", k);
        }
    }
    // ... and the packed tail whenever it exists: stages [split, nstages) from packed_first on, within the LDS the deep kernel sets aside
    CHECK(P.split_stage >= 1 && P.split_stage <= P.nstages, "split %u", P.split_stage);
    if (P.packed.empty()) {
        CHECK(P.packed_first == 0, "packed_first without a table");
    } else {
        CHECK(P.decimal_alphas && w24 && P.split_stage < P.nstages, "packed tail of a cascade the deep LDS kernel cannot run");
        CHECK(P.packed_first == P.stages[P.split_stage].first && P.packed.size() == P.nfeat - P.packed_first, "packed tail: first %u, %zu records", P.packed_first, P.packed.size());
        CHECK(P.packed.size() * sizeof(HtPackedFeature) <= 64 * 1024, "packed tail: %zu records", P.packed.size());
        for (size_t i = 0; i < P.packed.size(); i++) {
            const HtBlobFeature &f = P.feats[P.packed_first + i];
            const HtPackedFeature &t = P.packed[i];
            for (int neg = 0; neg < 2; neg++) {
                const std::vector<Pt> pts = blob_points(f, neg);
                CHECK(pts.size() <= 5, "packed %zu: %zu points", i, pts.size());
                for (int q = 0; q < 5; q++) {
                    const Pt want = pts[q < (int)pts.size() ? q : 0];
                    CHECK(patch_point(t.off[5 * neg + q], 24, want.z) == want && t.off[5 * neg + q] < HT_PATCH_BYTES, "packed %zu: slot %d", i, 5 * neg + q);
                }
            }
            CHECK(same_bits((double)t.a0i / 1e8, f.alpha[0]) && same_bits((double)t.a1i / 1e8, f.alpha[1]) && t.pad == 0, "packed %zu: integers", i);
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s <cases>\n", argv[0]), 2;
    std::ifstream cases(argv[1]);
    std::string line;
    while (std::getline(cases, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string path;
        int builtin, split;
        ss >> g_case >> path >> builtin >> split;
        if (!ss) return fprintf(stderr, "bad case line: %s\n", line.c_str()), 2;
        std::ifstream bf(path, std::ios::binary);
        if (!bf) return fprintf(stderr, "%s: cannot read %s\n", g_case.c_str(), path.c_str()), 2;
        const std::vector<char> file((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
        // a heap copy of exactly the blob's size: AddressSanitizer sees any read past either end
        uint8_t *blob = (uint8_t *)malloc(file.size() ? file.size() : 1);
        std::memcpy(blob, file.data(), file.size());
        HtCascadePlan P;
        std::string why;
        const bool ok = ht_plan_cascade(blob, file.size(), &P, &why);
        printf("{\"name\":\"%s\",\"status\":%d,\"message\":\"%s\"", g_case.c_str(), ok ? (int)HT_OK : (int)HT_ERR_INVALID, why.c_str());
        if (ok) {
            ht_plan_cascade_split(&P, builtin != 0, split);
            check_plan(P);
            int inexact = 0;
            for (auto &f : P.feats) inexact += !ht_e8(f.alpha[0]).exact + !ht_e8(f.alpha[1]).exact;
            for (auto &s : P.stages) inexact += !ht_e8(s.threshold).exact;
            printf(",\"cw\":%u,\"ch\":%u,\"nstages\":%u,\"nfeat\":%u,\"decimal_alphas\":%d,\"split_stage\":%u,\"packed_first\":%u,\"inexact\":%d", P.cw, P.ch, P.nstages, P.nfeat,
                   (int)P.decimal_alphas, P.split_stage, P.packed_first, inexact);
            printf(",\"crc_blob_stages\":%u,\"crc_blob_feats\":%u", crc_of(P.stages), crc_of(P.feats));
            printf(",\"n_stages\":%zu,\"crc_stages\":%u,\"n_deep\":%zu,\"crc_deep\":%u,\"n_tile\":%zu,\"crc_tile\":%u,\"n_fp\":%zu,\"crc_fp\":%u", P.dev_stages.size(),
                   crc_of(P.dev_stages), P.deep.size(), crc_of(P.deep), P.tile.size(), crc_of(P.tile), P.fp.size(), crc_of(P.fp));
            printf(",\"n_patch\":%zu,\"crc_patch\":%u,\"n_packed\":%zu,\"crc_packed\":%u", P.patch.size(), crc_of(P.patch), P.packed.size(), crc_of(P.packed));
        }
        printf("}\n");
        free(blob);
    }
    return 0;
}
