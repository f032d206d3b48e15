// Host-only harness around headtrackr_amd/csrc/ht_group_plan.h — the SAME code the device-grouped collect runs on the host: the cap
// option, the layout of the result block, ht_group_hits' argument checks, the record <-> rect conversion and the completion of the
// frames the kernel leaves to the host.  Built by tests/test_group_cases_cpu.py with  g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all  and run as a program:
//     group_harness <in.bin> <out.bin>
// in.bin : u32 nframes, u32 n, i32 min_neighbors, i32 interval, then n x ht_hit (24 B, arrival order: frames interleaved)
// out.bin: u32 ok, nframes x ht_rect (best), nframes x u32 (ngrouped), then the grouped lists back to back in frame order
// Every frame goes through ht_grp_complete_frame with buffers of exactly its size (an overrun is a heap overflow ASan reports).  The plan
// checks run first and end the program with exit status 3 when one fails.  TEST INFRASTRUCTURE: not part of the product.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ht_group_plan.h"

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "plan check failed: %s\n", #cond);      \
            return 3;                                                     \
        }                                                                 \
    } while (0)

static int plan_checks() {
    CHECK(ht_grp_cap(1 << 30) == 1024 && ht_grp_cap(1024) == 1024 && ht_grp_cap(1023) == 512 && ht_grp_cap(65) == 64 && ht_grp_cap(64) == 64);
    CHECK(ht_grp_cap(1) == 64 && ht_grp_cap(0) == 64 && ht_grp_cap(-5) == 64 && ht_grp_cap(1ll << 40) == 1024);
    for (uint32_t nfr : {1u, 2u, 3u, 257u, 4096u}) {
        const HtGrpLayout L = ht_grp_layout(nfr);
        CHECK(L.records == 16 && L.records % 16 == 0 && L.status == 16 + (size_t)nfr * 64 && L.ngrouped == L.status + 4u * nfr);
        CHECK(L.count == L.ngrouped + 4u * nfr && L.start == L.count + 4u * nfr && L.bytes == L.start + 4u * nfr && L.status % 4 == 0);
    }
    ht_hit h[2] = {};
    ht_rect r[2] = {};
    uint32_t ng[2] = {};
    const char *why = nullptr;
    CHECK(ht_grp_check_hits(h, 2, 1, 16, r, r, ng, &why) == HT_OK && why == nullptr);
    CHECK(ht_grp_check_hits(nullptr, 0, 1, 16, r, nullptr, nullptr, &why) == HT_OK);
    CHECK(ht_grp_check_hits(nullptr, 2, 1, 16, r, r, ng, &why) == HT_ERR_INVALID && why);
    CHECK(ht_grp_check_hits(h, 2, 0, 16, r, r, ng, &why) == HT_ERR_INVALID);
    CHECK(ht_grp_check_hits(h, 2, -1, 16, r, r, ng, &why) == HT_ERR_INVALID);
    CHECK(ht_grp_check_hits(h, 2, 1, 16, nullptr, r, ng, &why) == HT_ERR_INVALID);
    CHECK(ht_grp_check_hits(h, 2, 1, 16, r, r, nullptr, &why) == HT_ERR_INVALID);
    CHECK(ht_grp_check_hits(h, 2, 1, 16, r, nullptr, ng, &why) == HT_ERR_INVALID);
    CHECK(ht_grp_check_hits(h, 17, 1, 16, r, r, ng, nullptr) == HT_ERR_INVALID);
    const ht_rect a = {1.5, 2.25, 24, 30.238105197476955, -3.75, 7, 0};
    double rec[HT_GRP_REC_F64];
    ht_grp_rect_to_record(a, 1234567.0, rec);
    const ht_rect b = ht_grp_record_to_rect(rec);
    CHECK(std::memcmp(&a, &b, sizeof(a)) == 0 && rec[5] == 7.0 && rec[6] == 1234567.0 && rec[7] == 1.0);
    ht_rect best;
    uint32_t n = 9;
    const HtPostCfg cfg = {5, 24u, 24u};
    double sx[HT_MAX_LEVELS];
    ht_post_level_scales(cfg, sx);
    CHECK(ht_grp_complete_frame(cfg, sx, nullptr, 0, 1, &best, nullptr, &n) == HT_OK && n == 0 && best.confidence == -10000.0 && best.neighbors == 0);
    CHECK(ht_grp_complete_frame(cfg, sx, nullptr, 1, 1, &best, r, &n) == HT_ERR_INVALID);
    CHECK(ht_grp_complete_frame(cfg, sx, h, 1, 1, nullptr, r, &n) == HT_ERR_INVALID);
    h[0].scale = HT_MAX_LEVELS;  // never indexes the level scales
    CHECK(ht_grp_complete_frame(cfg, sx, h, 1, 1, &best, r, &n) == HT_ERR_INVALID);
    return 0;
}

int main(int argc, char **argv) {
    if (const int rc = plan_checks()) return rc;
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[4];
    if (std::fread(hdr, 4, 4, f) != 4) return 2;
    const uint32_t nfr = hdr[0], n = hdr[1];
    const int32_t min_neighbors = (int32_t)hdr[2];
    const HtPostCfg cfg = {(int)hdr[3], 24u, 24u};
    std::vector<ht_hit> raw(n);
    if (n && std::fread(raw.data(), sizeof(ht_hit), n, f) != n) return 2;
    std::fclose(f);
    double sx[HT_MAX_LEVELS];
    ht_post_level_scales(cfg, sx);
    std::vector<ht_hit> dst(n);
    std::vector<uint32_t> end, counts(nfr);
    uint32_t ok = ht_post_bucket_by_frame(raw.data(), n, nfr, dst.data(), end, counts.data()) ? 1u : 0u;
    std::vector<ht_rect> best(nfr), all;
    std::vector<uint32_t> ngrouped(nfr);
    for (uint32_t fr = 0; fr < nfr && ok; fr++) {
        const uint32_t b = fr ? end[fr - 1] : 0u, cnt = counts[fr];
        std::vector<ht_hit> fh(dst.begin() + b, dst.begin() + b + cnt);  // exactly the frame's hits
        std::vector<ht_rect> g(cnt);
        if (ht_grp_complete_frame(cfg, sx, cnt ? fh.data() : nullptr, cnt, min_neighbors, &best[fr], cnt ? g.data() : nullptr, &ngrouped[fr]) != HT_OK) ok = 0;
        else all.insert(all.end(), g.begin(), g.begin() + ngrouped[fr]);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(&ok, 4, 1, f);
    if (ok) {
        if (nfr) std::fwrite(best.data(), sizeof(ht_rect), nfr, f), std::fwrite(ngrouped.data(), 4, nfr, f);
        if (!all.empty()) std::fwrite(all.data(), sizeof(ht_rect), all.size(), f);
    }
    std::fclose(f);
    return 0;
}
