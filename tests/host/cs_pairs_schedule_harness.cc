// Host-only harness around the pair-call decisions of headtrackr_amd/csrc/ht_cs_schedule.h (ht_cs_plan_track_pairs,
// ht_cs_plan_init_pairs), built by tests/test_cs_pairs_cluster_cpu.py with g++ -fsanitize=address,undefined and run directly.
//
//   cs_pairs_schedule_harness <cases>   one case per line, one JSON object per line out:
//       track  n nd W H num_cus cs_pairs_cluster cs_cluster cs_cluster_min_px cs_iters cs_region
//       init   cs_pairs_cluster n tallest_rect num_cus
//     every `track` also checks what the launches rely on: the cluster grid is at most one workgroup per CU, LUT and exchange slots hold
//     the call's pairs, and the chunk plan is the one of the DISTINCT frames.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "ht_cs_schedule.h"

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

static void print_launch(const char *key, const HtCsLaunch &l) {
    printf(", \"%s\": {\"grid\": [%u, %u], \"block\": %u, \"lds\": %zu, \"timer\": \"%s\"}", key, l.grid_x, l.grid_y, l.block, l.lds, l.timer ? l.timer : "");
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        g_case = line;
        std::istringstream is(line);
        std::string kind;
        is >> kind;
        if (kind == "track") {
            HtCspTrackIn in;
            int opt = 0, cluster = 0;
            is >> in.n >> in.nd >> in.W >> in.H >> in.num_cus >> opt >> cluster >> in.cs_cluster_min_px >> in.dbg_cs_iters >> in.cs_region_cap;
            CHECK(!is.fail(), "bad case");
            in.cs_pairs_cluster = opt != 0, in.cs_cluster = cluster != 0;
            const HtCspTrackPlan p = ht_cs_plan_track_pairs(in);
            const bool cl = p.form == HT_CSP_CLUSTER;
            CHECK(cl == (p.lut.block != 0), "k_csp_lut belongs to the cluster form");
            CHECK(p.hist.block == (uint32_t)HIST_NT && p.meanshift.block != 0, "both forms launch the histogram pass and a mean-shift kernel");
            uint32_t chunk_px = 0, nchunks = 0;
            ht_cs_hist_plan(p.npix, in.nd, &chunk_px, &nchunks);
            CHECK(p.chunk_px == chunk_px && p.nchunks == nchunks && p.hist.grid_x == nchunks && p.hist.grid_y == (uint32_t)in.nd, "chunk plan of the distinct frames");
            CHECK(chunk_px % (4u * HIST_NT) == 0 && (uint64_t)nchunks * chunk_px >= p.npix, "%u x %u < %u", nchunks, chunk_px, p.npix);
            if (cl) {
                CHECK((int)p.meanshift.grid_x == in.n * p.G && (int)p.meanshift.grid_x <= in.num_cus, "cluster grid %u of %d CUs", p.meanshift.grid_x, in.num_cus);
                CHECK(p.G >= 4 && p.G <= CL_MAXG && in.n <= CL_MAX_STREAMS, "G %d, n %d", p.G, in.n);
                CHECK(p.lut.grid_x == 64 && p.lut.grid_y == (uint32_t)in.n && p.lut.block == (uint32_t)CS_LUT_NT, "one LUT per pair");
                CHECK(p.meanshift.block == (uint32_t)CL_NT && p.meanshift.lds == 0, "cluster workgroup");
                // LUT and exchange slots of a reservation that holds the call's pairs (n <= reserved is checked by the call itself)
                const HtCsReserveSizes s = ht_cs_reserve_sizes(in.n);
                CHECK(s.lut >= sizeof(double) * 4096 * (size_t)in.n && s.parts >= sizeof(double) * CL_SLOTS * CL_MAXG * 6 * (size_t)in.n, "LUT / exchange slots for %d pairs", in.n);
            } else {
                CHECK((int)p.meanshift.grid_x == in.n && p.meanshift.block == (uint32_t)CS_NT && p.meanshift.lds == (size_t)CS_REGION_CAP * 2, "one workgroup per pair");
                CHECK(p.region_cap == in.cs_region_cap && (size_t)p.region_cap * 2 <= p.meanshift.lds, "region of %d px", p.region_cap);
            }
            printf("{\"form\": \"%s\", \"G\": %d, \"region_cap\": %d, \"npix\": %u, \"chunk_px\": %u, \"nchunks\": %u", cl ? "CLUSTER" : "PER_PAIR", p.G, p.region_cap, p.npix,
                   p.chunk_px, p.nchunks);
            print_launch("hist", p.hist);
            print_launch("lut", p.lut);
            print_launch("meanshift", p.meanshift);
            printf("}\n");
        } else if (kind == "init") {
            int opt = 0, n = 0, tallest = 0, num_cus = 0;
            is >> opt >> n >> tallest >> num_cus;
            CHECK(!is.fail(), "bad case");
            const HtCsInitPlan p = ht_cs_plan_init_pairs(opt != 0, n, tallest, num_cus);
            const HtCsInitPlan b = ht_cs_plan_init(n, tallest, num_cus);
            CHECK(p.rows == (opt != 0 && b.rows), "the batch rule under the option");
            CHECK(p.rows ? (p.G == b.G && p.G >= 2 && p.G <= 32) : p.G == 1, "G %d", p.G);
            printf("{\"G\": %d, \"rows\": %s}\n", p.G, p.rows ? "true" : "false");
        } else if (!kind.empty()) {
            CHECK(false, "unknown case kind");
        }
    }
    return 0;
}
