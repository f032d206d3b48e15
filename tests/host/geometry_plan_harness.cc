// Host-only harness around headtrackr_amd/csrc/ht_geometry_plan.h (the geometry plan of ht_set_geometry), built by
// tests/test_geometry_plan_cpu.py with g++ -fsanitize=address,undefined.
//
//   geometry_plan_harness plan <cases>   one case per line:
//       name W H max_batch interval rs_rpt rs_nofast rs_nosort rs_notail rs_tailcap rs_tailcap_forced tail_table tail_table_forced
//       early_scan aux_stream queue_capacity_cfg nlevel_dims [w h]... [cw ch]
//     (cw ch: the cascade's window, 24 24 when left out)
//     plans every case, checks what the kernels rely on (check_plan below) and prints one JSON object per line: the scalar results, one
//     CRC32 per table as ht_set_geometry uploads it, the level sizes, and the largest bx / pass0 / scan-tile origin of the tile records
//   geometry_plan_harness dims <cases>   one "name W H interval nlevel_dims [w h]..." per line: prints {"name", "status", "why"} of ht_check_level_dims,
//     the validation ht_set_geometry runs on level_dims before it touches the current geometry
//   geometry_plan_harness taps <tuples>  one "i r s origin" per line (r as a C hex float): prints "a b t u" of ht_host_tap (t, u as hex floats)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "ht_geometry_plan.h"

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

// What the kernels rely on without checking it.
static void check_plan(const HtPlanInputs &in, const HtGeometryPlan &P) {
    // k_resample / k_resample_bands: the tiles of a job cover every destination pixel of its canvas exactly once, ...
    for (size_t g = 1; g < P.gens.size(); g++) {
        CHECK(P.gen_blocks[g] == P.gen_tiles[g].size(), "generation %zu", g);
        std::map<uint32_t, std::vector<uint8_t>> cover;  // by dst_off: one canvas per job
        for (auto &j : P.gens[g]) CHECK(cover.emplace(j.dst_off, std::vector<uint8_t>((size_t)j.cw * j.ch, 0)).second, "two jobs draw canvas %u", j.dst_off);
        for (auto &t : P.gen_tiles[g]) {
            auto it = cover.find(t.dst_off);
            CHECK(it != cover.end(), "tile of no job (canvas %u)", t.dst_off);
            CHECK(t.np >= 1 && t.np <= HT_RS_MAX_PASSES && t.np <= std::max(in.rs_rpt, 1), "np %d", t.np);
            const int X0 = 64 * t.bx, Y0 = 16 * t.pass0;
            for (int y = Y0; y < std::min(Y0 + 16 * t.np, t.ch); y++)
                for (int x = X0; x < std::min(X0 + 64, t.cw); x++) it->second[(size_t)y * t.cw + x]++;
            // ... its ex_* rectangle contains the a and b of every tap of the tile, ...
            const int ncols = std::min(64, t.dw - X0), nrows = std::min(16 * t.np, t.dh - Y0);
            if (ncols <= 0 || nrows <= 0) {
                CHECK(t.ex_sw16 == 0 && !(t.pad & 4), "extent of a tile that draws nothing");
                continue;
            }
            CHECK(t.ex_sw16 >= 1 && t.ex_sh >= 1 && (t.ex_xa & 15) == 0, "extent %d %d %d", t.ex_xa, t.ex_sw16, t.ex_sh);
            for (int x = X0; x < X0 + ncols; x++) {
                const HtTap c = ht_host_tap(x, t.rx, t.sw, t.sx);
                CHECK(c.a >= t.ex_xa && c.b >= c.a && c.b < t.ex_xa + 16 * t.ex_sw16, "column %d: taps %d %d outside [%d, +%d)", x, c.a, c.b, t.ex_xa, 16 * t.ex_sw16);
            }
            for (int y = Y0; y < Y0 + nrows; y++) {
                const HtTap r = ht_host_tap(y, t.ry, t.sh, t.sy);
                CHECK(r.a >= t.ex_ya && r.b >= r.a && r.b < t.ex_ya + t.ex_sh, "row %d: taps %d %d outside [%d, +%d)", y, r.a, r.b, t.ex_ya, t.ex_sh);
            }
            // ... and pad & 4 says that every wavefront's band has 1 <= rows <= HT_RSB_ROWS, starts at most 255 rows into the extent and holds
            // the taps of the wavefront's rows
            if (t.pad & 4)
                for (int w = 0; w < 4; w++) {
                    const int bya = (t.band_ya4 >> (8 * w)) & 0xff, bsh = (t.band_sh4 >> (8 * w)) & 0xff;
                    CHECK(bsh >= 1 && bsh <= HT_RSB_ROWS, "band %d: %d rows", w, bsh);
                    const int r0 = std::min(4 * t.np * w, nrows - 1), r1 = std::min(4 * t.np * (w + 1) - 1, nrows - 1);
                    CHECK(ht_host_tap(Y0 + r0, t.ry, t.sh, t.sy).a - t.ex_ya == bya, "band %d: first row does not fit a byte", w);
                    for (int y = Y0 + r0; y <= Y0 + r1; y++) {
                        const HtTap r = ht_host_tap(y, t.ry, t.sh, t.sy);
                        CHECK(r.a >= t.ex_ya + bya && r.b < t.ex_ya + bya + bsh, "band %d row %d", w, y);
                    }
                }
        }
        for (auto &c : cover)
            for (size_t i = 0; i < c.second.size(); i++) CHECK(c.second[i] == 1, "generation %zu canvas %u: pixel %zu covered %d times", g, c.first, i, c.second[i]);
    }
    // k_scan_tiles: the tiles of a scale cover its 2 qw x 2 qh half-steps exactly once; tile_begin and win_begin are prefix sums
    uint32_t tiles = 0;
    uint64_t wins = 0;
    for (auto &S : P.scales) {
        CHECK(S.tile_begin == tiles && S.win_begin == wins, "scale %d: begins %u %u, expected %u %llu", S.l0, S.tile_begin, S.win_begin, tiles, (unsigned long long)wins);
        CHECK(S.tw2 <= HT_SCAN_TXH && S.th2 <= HT_SCAN_TYH && S.tw2 % 8 == 0 && S.th2 % 2 == 0, "scale %d: tile %d x %d", S.l0, S.tw2, S.th2);
        std::vector<uint8_t> cover((size_t)4 * S.qw * S.qh, 0);
        for (int k = 0; k < S.ntx * S.nty; k++) {
            CHECK(tiles + k < P.tile_recs.size(), "tile list too short");
            const HtTileRec &r = P.tile_recs[tiles + k];
            const int X0 = r.origin & 0xffff, Y0 = r.origin >> 16, tw = r.size & 0xffff, th = r.size >> 16;
            CHECK((int)(r.tw2_l0 >> 16) == S.l0 && (int)(r.tw2_l0 & 0xffff) == S.tw2 && tw >= 1 && th >= 1 && tw <= S.tw2 && th <= S.th2, "tile %u", tiles + k);
            CHECK(X0 + tw <= 2 * S.qw && Y0 + th <= 2 * S.qh, "tile %u leaves the scale", tiles + k);
            for (int y = Y0; y < Y0 + th; y++)
                for (int x = X0; x < X0 + tw; x++) cover[(size_t)y * 2 * S.qw + x]++;
        }
        for (size_t i = 0; i < cover.size(); i++) CHECK(cover[i] == 1, "scale %d: half-step %zu covered %d times", S.l0, i, cover[i]);
        tiles += (uint32_t)(S.ntx * S.nty);
        wins += 4ull * S.qw * S.qh;
    }
    CHECK(tiles == P.tiles_per_frame && tiles == P.tile_recs.size() && wins == P.windows_per_frame, "totals");
    CHECK(P.early_tiles < std::max(P.tiles_per_frame, 1u), "early tiles");
    // k_resample_tail: the generations' job ranges and the jobs' tap ranges are contiguous, a generation's taps begin with its first job's
    if (P.tail_first_gen > 0) {
        const HtTailGens &T = P.tail;
        const size_t nj = P.tail_jobs.size();
        CHECK(T.ngen >= 2 && T.ngen <= HT_TAIL_MAX_GENS && P.tail_first_gen + T.ngen == (int)P.gens.size(), "tail generations");
        CHECK(T.job_begin[0] == 0 && (size_t)T.job_begin[T.ngen] == nj && P.tail_prefix.size() == nj && P.tail_tapref.size() == nj, "tail jobs");
        CHECK(P.tail_taps.size() == P.tail_taps_fast.size() && T.tap_begin[T.ngen] == P.tail_taps.size(), "tail taps");
        uint32_t at = 0;
        for (int g = 0; g < T.ngen; g++) {
            CHECK(T.job_begin[g] <= T.job_begin[g + 1] && T.job_begin[g + 1] - T.job_begin[g] <= HT_TAIL_MAX_JOBS, "tail generation %d", g);
            // (a generation without jobs — levels of size 0 — reads no taps: its tap_begin is left 0 and means nothing)
            if (T.job_begin[g] < T.job_begin[g + 1]) CHECK(T.tap_begin[g] == at, "tail generation %d: taps begin at %u, expected %u", g, T.tap_begin[g], at);
            uint32_t groups = 0;
            for (int k = T.job_begin[g]; k < T.job_begin[g + 1]; k++) {
                const HtResampleJob &j = P.tail_jobs[k];
                const HtTailTapRef &r = P.tail_tapref[k];
                CHECK(P.tail_prefix[k] == groups, "tail job %d: prefix", k);
                groups += (uint32_t)((j.cw + 3) / 4) * (uint32_t)j.ch;
                CHECK(r.col == at && r.row == at + (uint32_t)std::max(j.dw, 1) + 3, "tail job %d: taps at %u %u, expected %u", k, r.col, r.row, at);
                at = r.row + (uint32_t)std::max(j.dh, 1);
            }
            CHECK(T.groups[g] == groups, "tail generation %d: groups", g);
        }
        CHECK(at == P.tail_taps.size(), "tail taps end");
        for (size_t i = 0; i < P.tail_taps.size(); i++)
            CHECK(P.tail_taps_fast[i].a == P.tail_taps[i].a && P.tail_taps_fast[i].tf == (float)P.tail_taps[i].t, "compact tap %zu", i);
    } else {
        CHECK(P.tail_jobs.empty() && P.tail_taps.empty(), "tail tables without a tail");
    }
}

static int run_plan(const char *path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        HtPlanInputs in;
        int W, H, mb, nofast, nosort, notail, tcf, ttf, es, aux, nd;
        unsigned long long tailcap, qcfg;
        ss >> g_case >> W >> H >> mb >> in.interval >> in.rs_rpt >> nofast >> nosort >> notail >> tailcap >> tcf >> in.tail_table >> ttf >> es >> aux >> qcfg >> nd;
        std::vector<int32_t> dims(2 * (size_t)nd);
        for (auto &d : dims) ss >> d;
        if (!ss) return fprintf(stderr, "bad case line: %s\n", line.c_str()), 2;
        in.next = in.interval + 1, in.cw = in.ch = 24;
        {
            uint32_t cw, ch;
            if (ss >> cw >> ch) in.cw = cw, in.ch = ch;
        }
        in.rs_nofast = nofast, in.rs_nosort = nosort, in.rs_notail = notail, in.rs_tailcap = tailcap, in.rs_tailcap_forced = tcf, in.tail_table_forced = ttf;
        in.early_scan = es, in.aux_stream = aux, in.queue_capacity_cfg = (uint32_t)qcfg;
        const int upto = (int)std::floor(std::log((double)std::min(in.cw, in.ch)) / std::log(ht_scale_of(in.interval)));  // as ht_set_geometry, ccv.js:112
        const int n = upto + in.next * 2;                                                                                  // ccv.js:113
        if (n > HT_MAX_LEVELS || (nd && nd != n)) return fprintf(stderr, "%s: %d levels\n", g_case.c_str(), n), 2;
        HtGeometryPlan P;
        std::string why;
        const ht_status st = ht_plan_geometry(in, W, H, mb, nd ? dims.data() : nullptr, n, upto, &P, &why);
        printf("{\"name\":\"%s\",\"status\":%d,\"why\":\"%s\"", g_case.c_str(), (int)st, why.c_str());
        if (st == HT_OK) {
            check_plan(in, P);
            printf(",\"nlevels\":%d,\"arena_stride\":%llu,\"pyr_bytes\":%llu,\"windows_per_frame\":%llu,\"tiles_per_frame\":%u,\"tail_first_gen\":%d,\"tail_table\":%d,"
                   "\"early_gen\":%d,\"early_tiles\":%u,\"queue_capacity\":%u",
                   n, (unsigned long long)P.arena_stride, (unsigned long long)P.pyr_bytes, (unsigned long long)P.windows_per_frame, P.tiles_per_frame, P.tail_first_gen,
                   P.tail_table, P.early_gen, P.early_tiles, P.queue_capacity);
            printf(",\"crc_levels\":%u,\"crc_gen_tiles\":[", crc32(P.levels, sizeof(HtDevLevel) * n));
            for (size_t g = 0; g < P.gen_tiles.size(); g++) printf("%s%u", g ? "," : "", crc_of(P.gen_tiles[g]));
            printf("],\"gen_blocks\":[");
            for (size_t g = 0; g < P.gen_blocks.size(); g++) printf("%s%u", g ? "," : "", P.gen_blocks[g]);
            printf("],\"crc_tail_jobs\":%u,\"crc_tail_prefix\":%u,\"crc_tail_taps\":%u,\"crc_tail_taps_fast\":%u,\"crc_tail_tapref\":%u,\"crc_tail_gens\":%u,"
                   "\"crc_scales\":%u,\"crc_tile_recs\":%u,\"levels\":[",
                   crc_of(P.tail_jobs), crc_of(P.tail_prefix), crc_of(P.tail_taps), crc_of(P.tail_taps_fast), crc_of(P.tail_tapref), crc32(&P.tail, sizeof(P.tail)),
                   crc_of(P.scales), crc_of(P.tile_recs));
            for (int i = 0; i < n; i++) printf("%s[%d,%d]", i ? "," : "", P.levels[i].w, P.levels[i].h);
            // the largest values the 16-bit tile-record fields bx and pass0 take, and the largest scan-tile origin
            int max_bx = 0, max_pass0 = 0, max_x0 = 0, max_y0 = 0;
            for (auto &g : P.gen_tiles)
                for (auto &t : g) max_bx = std::max(max_bx, (int)t.bx), max_pass0 = std::max(max_pass0, (int)t.pass0);
            for (auto &r : P.tile_recs) max_x0 = std::max(max_x0, (int)(r.origin & 0xffff)), max_y0 = std::max(max_y0, (int)(r.origin >> 16));
            printf("],\"max_bx\":%d,\"max_pass0\":%d,\"max_tile_x0\":%d,\"max_tile_y0\":%d", max_bx, max_pass0, max_x0, max_y0);
        }
        printf("}\n");
    }
    return 0;
}

static int run_dims(const char *path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        int W, H, interval, nd;
        ss >> g_case >> W >> H >> interval >> nd;
        std::vector<int32_t> dims(2 * (size_t)std::max(nd, 0));
        for (auto &d : dims) ss >> d;
        if (!ss) return fprintf(stderr, "bad case line: %s\n", line.c_str()), 2;
        std::string why;
        const ht_status st = ht_check_level_dims(interval + 1, W, H, dims.data(), nd, &why);
        printf("{\"name\":\"%s\",\"status\":%d,\"why\":\"%s\"}\n", g_case.c_str(), (int)st, why.c_str());
    }
    return 0;
}

static int run_taps(const char *path) {
    std::ifstream f(path);
    std::string rs;
    int i, s, origin;
    while (f >> i >> rs >> s >> origin) {
        const HtTap t = ht_host_tap(i, std::strtod(rs.c_str(), nullptr), s, origin);
        printf("%d %d %a %a\n", t.a, t.b, t.t, t.u);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "plan") return run_plan(argv[2]);
    if (argc == 3 && std::string(argv[1]) == "dims") return run_dims(argv[2]);
    if (argc == 3 && std::string(argv[1]) == "taps") return run_taps(argv[2]);
    fprintf(stderr, "usage: %s plan <cases> | dims <cases> | taps <tuples>\n", argv[0]);
    return 2;
}
