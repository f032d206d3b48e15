// ht_draw_filter.hip — the draw list with a prefilter for strong downscales (ht_draw_list_filtered_device / ht_draw_filter_factors): each
// canvas pixel the mean of an Nx x Ny block of the UNFILTERED draw's samples.  ht_draw_filter_plan.h states the rule and plans a call on the
// host; the rounding is ht_filter_plan.h's.  Included by ht_ingest.hip behind the face-patch kernels: same code object as k_draw_list and k_cut_mean, whose
// helpers (fm_add, fm_finish, LpDwordStore) and shared text it takes.  The entry points and every other route into this kernel: ht_draw_calls.hip.
//
// k_draw_list_mean_tile<RPT>: grid (tile column, tile row, entry), 256 threads; a tile is 64 columns by RPT * 4 rows, RPT rows per thread
// (the library launches RPT 1, a 64 x 4 tile, at every max_factor: see dm_rpt_of).  A
// workgroup reads its entry's 112-byte descriptor — HtDrawDesc with the FINE ratios, then Nx, Ny — with scalar loads (blockIdx.z is uniform,
// the table const __restrict__).  The taps of the tile's fine columns and rows go to LDS, Nx * 64 + Ny * 4 RPT of them laid out [a][column]
// and [b][row] (the arrays hold factor 8: 15 KB at RPT 4, 13 KB at RPT 1); one barrier; then for every (b, a) of the block — a
// workgroup-uniform loop — the format's pixel body of ht_ingest_bodies.inc runs on tap slice a / b, through ht_list_parts.inc's scaffold,
// with an IG_STORE that ADDS the sample's four bytes to the thread's sums.  A fine sample is therefore the unfiltered rule's byte by
// construction: the binary64 blend of ig_channel, never contracted, rounded half to even; YUV taps converted first.  ht_filter_pixel
// rounds the sums and the dword is stored.  Source rows are not staged in LDS: a block's Nx fine taps of one output pixel lie side by side
// in the source, and the vector cache serves the neighbours (DESIGN.md §2.3.8 has the measurement).
#include "ht_draw_filter_plan.h"

namespace {

typedef HtDrawMeanDescT<dl_gptr> DmDesc;
static_assert(sizeof(DmDesc) == sizeof(HtDrawMeanDesc) && alignof(DmDesc) == alignof(HtDrawMeanDesc), "the kernel's view of a descriptor is the host's");

#undef IG_STORE
#define IG_STORE(o, x, y) ((void)out, (void)(x), (void)(y), fm_add(acc[k], o))  // k: the bodies' row index of the thread, a constant once unrolled

// (the name: k_draw_list_mean with the tile behind it.  In a listing of the code object the kernels that END in _mean<..> are the face
// crops' — tests/test_filter_cpu.py names them all — and a thin k_draw_list_mean over a tile function template was tried: it reordered
// k_cut_mean<-1, 1>'s epilogue, which shares fm_finish.  As a kernel template of its own it leaves every neighbour's instructions alone.)
template <int RPT>
__global__ __launch_bounds__(IG_NT) void k_draw_list_mean_tile(const DmDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh) {
    constexpr int IG_RPT = RPT, IG_TH = RPT * FM_ROWS;  // the tile of THIS kernel: the shared text reads these two names
    __shared__ RsTap s_colf[FM_MAXF * IG_TW], s_rowf[FM_MAXF * IG_TH];
    const DmDesc &m = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const DlDesc &d = m.d;
    const int sx = d.sx, sy = d.sy, sw = d.sw, sh = d.sh, format = d.format;
    const int nx = min(max(m.nx, 1), FM_MAXF), ny = min(max(m.ny, 1), FM_MAXF);  // the plan's 1 .. 8; the clamp keeps the LDS index in bounds whatever the table holds
    const double rx = d.rx, ry = d.ry;  // the fine frame's: sw / (nx dw), sh / (ny dh), divided on the host
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * IG_TH;
    for (int t = threadIdx.x; t < nx * IG_TW; t += IG_NT)  // [a][column]: fine column nx * x + a
        s_colf[t] = rs_tap(nx * min(X0 + (t & (IG_TW - 1)), dw - 1) + t / IG_TW, rx, sw, sx);
    for (int t = threadIdx.x; t < ny * IG_TH; t += IG_NT)  // [b][row]
        s_rowf[t] = rs_tap(ny * min(Y0 + (t & (IG_TH - 1)), dh - 1) + t / IG_TH, ry, sh, sy);
    __syncthreads();
    uint32_t acc[IG_RPT][4] = {};
    // every (b, a) of the block runs the format's body on tap slice a / b
#define LP_EACH_PASS                                   \
    _Pragma("unroll 1") for (int b = 0; b < ny; b++)   \
    _Pragma("unroll 1") for (int a = 0; a < nx; a++)   \
    if (const RsTap *s_col = s_colf + a * IG_TW, *s_row = s_rowf + b * IG_TH; true)
    // the 64 x 16 form draws YUYV / UYVY entries too: every draw of a packed 4:2:2 source is k_draw_list_mean_tile<IG_RPT>'s (dm_launch).  The
    // 64 x 4 form, which every other filtered call takes, stays the instructions it was: with the branch it measured 10 - 17 % slower on lists
    // WITHOUT a packed entry (81 against 74 us at max_factor 8, 57 against 49 us at 4)
#define LP_PACKED_422 (RPT == 4)
#define LP_PART 4  // LP_SCAFFOLD
#include "ht_list_parts.inc"
    fm_finish<RPT>(acc, (uint32_t)(nx * ny), LpDwordStore{reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride), dw}, dw, dh);
}

#undef IG_STORE
#define IG_STORE IG_STORE_DWORD  // the default again, for whatever is compiled behind this file

// the tile of a call: 64 x 4 (RPT 1) at every max_factor.  Unlike the face crops' 112 x 112 patches a canvas has tiles enough for either form, and
// the short workgroups won at every factor: on eight feeds -> 320 x 240, 74 against 100 us at max_factor 8, 18.5 against 20.9 us at 2, 9.2
// against 10.0 us at 1 (profiles/draw_filter.txt).  The 64 x 16 form stays compiled behind the context option draw_filter_rows = 16, for
// tools/gpu_draw_filter.py's comparison and the tests that pin both forms to the same bytes.
int dm_rpt_of(const ht_ctx *c) { return c->draw_filter_rows ? c->draw_filter_rows / FM_ROWS : 1; }

// dw x dh: the destination frames' size — the canvas, or (dm_unpack_sources, ht_draw_calls.hip) a source's own size
ht_status dm_launch(ht_ctx *c, const char *fn, const std::vector<HtDrawMeanDesc> &desc, uint8_t *dst, size_t dstride, int dw = 0, int dh = 0) {
    ht_status st = dl_upload(c, fn, desc);  // the draw list's staged table (ht_draw_list.hip)
    if (st != HT_OK) return st;
    HtProfScope ps(c, "draw_list_mean");
    if (!dw) dw = c->W, dh = c->H;
    const bool packed = std::any_of(desc.begin(), desc.end(), [](const HtDrawMeanDesc &m) { return ht_yuv_is_422(m.d.format); });
    const int rpt = packed ? IG_RPT : dm_rpt_of(c);  // (LP_PACKED_422: the 64 x 16 form alone holds the packed pixel body)
    const dim3 grid((dw + IG_TW - 1) / IG_TW, (dh + rpt * FM_ROWS - 1) / (rpt * FM_ROWS), (unsigned)desc.size());
    const DmDesc *tab = reinterpret_cast<const DmDesc *>(c->dl_tab.d);
    hipLaunchKernelGGL(rpt == 1 ? k_draw_list_mean_tile<1> : k_draw_list_mean_tile<IG_RPT>, grid, dim3(IG_NT), 0, c->stream, tab, dst, dstride, dw, dh);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

}  // namespace
