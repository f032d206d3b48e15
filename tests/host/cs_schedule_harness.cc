// Host-only harness around headtrackr_amd/csrc/ht_cs_schedule.h (the host-side decisions of the camshift calls), built by
// tests/test_cs_schedule_cpu.py with g++ -fsanitize=address,undefined.
//
//   cs_schedule_harness <cases>   one case per line, one JSON object per line out:
//       chunks  npix nstreams
//       track   n reserved W H num_cus cs_fused_min cs_cluster cs_cluster_min_px cs_iters cs_region cs_fused_nt other_busy
//       init    n tallest_rect num_cus
//       reserve nstreams
//     `chunks` and every `track` that plans a histogram pass also check what the kernels rely on without checking it (check_chunks).
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

// k_cs_hist: workgroup k takes pixels [k chunk_px, (k + 1) chunk_px) in sweeps of 4 * HIST_NT, the grid's chunks cover the frame, none of
// them is empty, and the chunk histograms fit the buffer ht_camshift_reserve sized with max_chunks
static void check_chunks(uint32_t npix, uint32_t max_chunks, uint32_t chunk_px, uint32_t nchunks) {
    CHECK(chunk_px % (4u * HIST_NT) == 0 && chunk_px > 0, "chunk_px %u", chunk_px);
    CHECK((uint64_t)nchunks * chunk_px >= npix, "%u x %u < %u", nchunks, chunk_px, npix);
    CHECK(npix == 0 || npix > (uint64_t)(nchunks - 1) * chunk_px, "last chunk empty: %u x %u, %u", nchunks, chunk_px, npix);
    CHECK(nchunks >= 1 && nchunks <= max_chunks, "%u chunks of %u", nchunks, max_chunks);
}

static const char *form_name(HtCsForm f) {
    switch (f) {
    case HT_CS_FUSED_1024: return "FUSED_1024";
    case HT_CS_FUSED_512: return "FUSED_512";
    case HT_CS_CLUSTER: return "CLUSTER";
    default: return "PER_STREAM";
    }
}
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
        if (kind == "chunks") {
            uint32_t npix = 0, chunk_px = 0, nchunks = 0;
            int nstreams = 0;
            is >> npix >> nstreams;
            CHECK(!is.fail(), "bad case");
            ht_cs_hist_plan(npix, nstreams, &chunk_px, &nchunks);
            check_chunks(npix, hist_max_chunks(nstreams), chunk_px, nchunks);
            printf("{\"max_chunks\": %u, \"chunk_px\": %u, \"nchunks\": %u}\n", hist_max_chunks(nstreams), chunk_px, nchunks);
        } else if (kind == "track") {
            HtCsTrackIn in;
            int cluster = 0, forced_nt = 0, other_busy = 0;
            is >> in.n >> in.cs_streams >> in.W >> in.H >> in.num_cus >> in.cs_fused_min_streams >> cluster >> in.cs_cluster_min_px >> in.dbg_cs_iters >>
                in.cs_region_cap >> forced_nt >> other_busy;
            CHECK(!is.fail(), "bad case");
            in.cs_cluster = cluster != 0;
            if (ht_cs_takes_fused(in.n, in.cs_fused_min_streams)) in.fused_nt = ht_cs_fused_form(forced_nt, in.n, in.num_cus, other_busy != 0);
            const HtCsTrackPlan p = ht_cs_plan_track(in);
            const bool fused = p.form == HT_CS_FUSED_1024 || p.form == HT_CS_FUSED_512;
            CHECK(fused == (p.fused.block != 0) && fused == (p.hist.block == 0) && fused == (p.meanshift.block == 0), "launches of the form");
            CHECK((p.form == HT_CS_CLUSTER) == (p.lut.block != 0), "k_cs_lut belongs to the cluster form");
            if (!fused) check_chunks(p.npix, hist_max_chunks(in.cs_streams), p.chunk_px, p.nchunks);
            // the cluster grid is co-resident: at most one workgroup per CU, and the exchange slots hold G partial sums per pass
            if (p.form == HT_CS_CLUSTER) CHECK((int)p.meanshift.grid_x <= in.num_cus && p.G <= CL_MAXG && in.n <= CL_MAX_STREAMS, "cluster grid %u", p.meanshift.grid_x);
            CHECK(p.region_cap <= CS_REGION_CAP && (size_t)p.region_cap * 2 <= p.fused.lds + p.meanshift.lds, "region of %d px in %zu B", p.region_cap, p.fused.lds + p.meanshift.lds);
            printf("{\"form\": \"%s\", \"G\": %d, \"region_cap\": %d, \"npix\": %u, \"chunk_px\": %u, \"nchunks\": %u", form_name(p.form), p.G, p.region_cap, p.npix,
                   p.chunk_px, p.nchunks);
            print_launch("fused", p.fused);
            print_launch("hist", p.hist);
            print_launch("lut", p.lut);
            print_launch("meanshift", p.meanshift);
            printf("}\n");
        } else if (kind == "init") {
            int n = 0, tallest = 0, num_cus = 0;
            is >> n >> tallest >> num_cus;
            CHECK(!is.fail(), "bad case");
            const HtCsInitPlan p = ht_cs_plan_init(n, tallest, num_cus);
            CHECK(p.G >= 0 && p.G <= 32 && (!p.rows || p.G >= 2), "G %d", p.G);
            printf("{\"G\": %d, \"rows\": %s}\n", p.G, p.rows ? "true" : "false");
        } else if (kind == "reserve") {
            int nstreams = 0;
            is >> nstreams;
            CHECK(!is.fail(), "bad case");
            const HtCsReserveSizes s = ht_cs_reserve_sizes(nstreams);
            printf("{\"states\": %zu, \"hist\": %zu, \"out\": %zu, \"lut\": %zu, \"parts\": %zu, \"err_word\": %zu, \"ring_out\": %zu, \"ring_flags\": %zu}\n", s.states,
                   s.hist, s.out, s.lut, s.parts, s.err_word, s.ring_out, s.ring_flags);
        } else if (!kind.empty()) {
            CHECK(false, "unknown case kind");
        }
    }
    return 0;
}
