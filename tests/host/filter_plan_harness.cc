// filter_plan_harness.cc — the rule of the prefiltered face crops (headtrackr_amd/csrc/ht_filter_plan.h: the very lines k_cut_mean and
// k_upright_mean compile for the device) on the host, plain and under AddressSanitizer + UBSan (tests/test_filter_cpu.py builds and runs it).
//   filter_plan_harness in.bin out.bin
// in.bin: cases of 64 bytes {i64 a, b, vx, vy; i32 kind, P, Q, max_factor, code, sum, n, pad}: kind 0 a crop record of rect width a and
//         height b, kind 1 an align record of vectors (a, b) and (vx, vy)
// out.bin: per case i64 Nx, Ny (through the record functions: 0, 0 for an empty record), ht_filter_mean(sum, n), and — align, not empty — the
//          first and the last column term of the FINE patch, ht_align_term(i, Nx P, a) at i = 0 and Nx P - 1 (crop or empty: 0, 0)
#include <cstdio>
#include <vector>

#include "ht_align_plan.h"
#include "ht_filter_plan.h"

struct Case {
    int64_t a, b, vx, vy;
    int32_t kind, P, Q, max_factor, code, sum, n, pad;
};
static_assert(sizeof(Case) == 64, "Case");

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Case> cases;
    Case c;
    while (std::fread(&c, sizeof(c), 1, f) == 1) cases.push_back(c);
    std::fclose(f);
    std::vector<int64_t> out;
    out.reserve(cases.size() * 5);
    for (const Case &k : cases) {
        int32_t nx = -1, ny = -1;
        int64_t first = 0, last = 0;
        if (!ht_filter_args_ok(k.P, k.Q, k.max_factor)) return 6;
        if (k.kind == 0) {
            ht_crop_record r = {};
            r.code = k.code, r.rect.width = (int32_t)k.a, r.rect.height = (int32_t)k.b;
            ht_filter_crop_record_factors(r, k.P, k.Q, k.max_factor, &nx, &ny);
        } else {
            ht_align_record r = {};
            r.code = k.code, r.ux = k.a, r.uy = k.b, r.vx = k.vx, r.vy = k.vy;
            ht_filter_align_record_factors(r, k.P, k.Q, k.max_factor, &nx, &ny);
            if (k.code == HT_ALIGN_FACE) first = ht_align_term(0, nx * k.P, k.a), last = ht_align_term(nx * k.P - 1, nx * k.P, k.a);
        }
        out.push_back(nx), out.push_back(ny), out.push_back(ht_filter_mean((uint32_t)k.sum, (uint32_t)k.n));
        out.push_back(first), out.push_back(last);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = out.empty() || std::fwrite(out.data(), sizeof(int64_t), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("cases %zu\n", cases.size());
    return ok ? 0 : 5;
}
