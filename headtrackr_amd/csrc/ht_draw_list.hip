// ht_draw_list.hip — the K-feed form of the video -> canvas draw: ONE launch draws a list of sources that share nothing (the reference's
// loop is one drawImage per feed, main.js:170).  Every entry has its own device allocation(s), size, pitches, format (RGBA, NV12, I420; YUYV and UYVY: see dl_launch),
// matrix and source rect; entry i goes onto destination frame i with the bytes ht_draw_frames_device / ht_draw_frames_yuv_device give for
// it alone.  Included by ht_ingest.hip, so it is part of the same code object and shares that file's and ht_ingest_yuv.hip's
// text: the tile constants, ig_channel, ig_chroma_read and, through ht_ingest_bodies.inc, the taps and the three pixel bodies.
//
// k_draw_list: grid (tile column, tile row, entry), 64 x 16 destination pixels and 256 threads per workgroup.  A workgroup reads its
// entry's 104-byte descriptor (ht_draw_list_plan.h) — blockIdx.z is uniform and the table is const __restrict__, so these are scalar
// loads —, computes the tile's 80 taps from that entry's ratios and rect into LDS, and behind the barrier takes a workgroup-uniform branch
// into one of the three bodies.  The table reaches the device
// through a staged table (HtStagedTable, ht_internal.h: a ring of pinned slots and one hipMemcpyAsync on the ctx stream per call), as
// every list call's table does.  DESIGN.md §2.3.2 gives the reasoning and the registers.
//
// A list with an ORIENTED entry (an orientation in bits 8..10 of its format: ht_orient_plan.h) is not k_draw_list's: the second half of this
// file loads the oriented draw's kernels from a code object of their own and launches them.  The entry point itself — one
// function with ht_draw_list_filtered_device — is ht_draw_calls.hip, the draw family's one host path.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "ht_draw_list_plan.h"
#include "ht_orient_plan.h"

namespace {

// a plane pointer out of the table is a GLOBAL address (ht_draw_list_device takes device pointers), and the kernel's view of the table
// says so in the member type: the bodies' reads are then global_load like the single-source kernels', whose pointers are kernel
// arguments, and not flat_load (a generic pointer loaded from memory says nothing about its address space).  Same bytes, same layout.
typedef const __attribute__((address_space(1))) uint8_t *dl_gptr;
typedef HtDrawDescT<dl_gptr> DlDesc;
static_assert(sizeof(DlDesc) == sizeof(HtDrawDesc) && alignof(DlDesc) == alignof(HtDrawDesc), "the kernel's view of a descriptor is the host's");

// every piece below is ht_ingest_bodies.inc: the text k_draw_frames and k_draw_yuv<> compile, with their parameter names bound to the entry
__global__ __launch_bounds__(IG_NT) void k_draw_list(const DlDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
    const DlDesc &d = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const int sx = d.sx, sy = d.sy, sw = d.sw, sh = d.sh, format = d.format;
    const double rx = d.rx, ry = d.ry;
#define IG_BODY_PART 1  // IG_BODY_TAPS
#include "ht_ingest_bodies.inc"
    __syncthreads();
    if (format == HT_DRAW_RGBA) {
        const uint8_t *__restrict__ src = (const uint8_t *)d.p0;
        const size_t src_pitch = d.pitch0, src_stride = 0;
#define IG_BODY_PART 2  // IG_BODY_RGBA
#include "ht_ingest_bodies.inc"
    } else {
        const uint8_t *__restrict__ yp = (const uint8_t *)d.p0, *__restrict__ up = (const uint8_t *)d.p1, *__restrict__ vp = (const uint8_t *)d.p2;
        const size_t y_pitch = d.pitch0, c_pitch = d.pitch1, stride = 0;
        const int cw = d.cw;
        const HtYuvCoef kc = d.kc;
        if (format == HT_YUV_FMT_NV12) {
            constexpr int FMT = HT_YUV_FMT_NV12;
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
        } else {
            constexpr int FMT = HT_YUV_FMT_I420;
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
        }
    }
}

// the table of a call on the device: through the context's staged descriptor table (HtStagedTable, ht_internal.h).  DESC: HtDrawDesc, or
// the filtered draw's wider descriptor (ht_draw_filter.hip) — both calls are the draw list and share the table
template <class DESC>
ht_status dl_upload(ht_ctx *c, const char *fn, const std::vector<DESC> &desc) {
    const size_t need = desc.size() * sizeof(DESC);
    ht_status st = ht_stage_reserve(c, &c->dl_tab, need, 64 * sizeof(HtDrawDesc), std::string(fn) + ": allocation of the descriptor table failed");
    if (st != HT_OK) return st;
    uint8_t *slot = nullptr;
    if ((st = ht_stage_take(c, &c->dl_tab, &slot)) != HT_OK) return st;
    std::memcpy(slot, desc.data(), need);
    return ht_stage_commit(c, &c->dl_tab, need);
}

// (a list with a packed 4:2:2 entry is not this kernel's: draw_list_call, ht_draw_calls.hip)
ht_status dl_launch(ht_ctx *c, const char *fn, const std::vector<HtDrawDesc> &desc, uint8_t *dst, size_t dstride) {
    ht_status st = dl_upload(c, fn, desc);
    if (st != HT_OK) return st;
    HtProfScope ps(c, "draw_list");
    const dim3 grid((c->W + IG_TW - 1) / IG_TW, (c->H + IG_TH - 1) / IG_TH, (unsigned)desc.size());
    hipLaunchKernelGGL(k_draw_list, grid, dim3(IG_NT), 0, c->stream, reinterpret_cast<const DlDesc *>(c->dl_tab.d), dst, dstride, c->W, c->H);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The oriented draw (ht_orient_plan.h).  Its device code is NOT in this library: the code objects here are held to the kernels and registers
// they have, so k_draw_list_oriented lives in a code object of its own, libheadtrackr_hip_orient.hsaco next to this library
// (csrc/ht_orient_kernels.hip, built by build.py).  It is found through dladdr on a symbol of this library, loaded with hipModuleLoad on the
// first oriented call — once per device and process, under a mutex, never reloaded or unloaded — and launched with hipModuleLaunchKernel on
// the context's stream.  Without the file an oriented call is HT_ERR_STATE with the path in its message; nothing else depends on it.
struct OrModule {
    hipModule_t mod = nullptr;
    hipFunction_t plain = nullptr, turn = nullptr;  // k_draw_list_oriented, k_draw_list_oriented_turn
};
constexpr int OR_MAX_DEVICES = 64;
std::mutex or_mutex;
OrModule or_modules[OR_MAX_DEVICES];

std::string or_module_path() {
    Dl_info info;
    std::string dir = ".";
    if (dladdr(reinterpret_cast<const void *>(&ht_draw_list_device), &info) && info.dli_fname) {
        const std::string lib(info.dli_fname);
        const size_t slash = lib.rfind('/');
        if (slash != std::string::npos) dir = lib.substr(0, slash);
    }
    return dir + "/libheadtrackr_hip_orient.hsaco";
}

// the module of the context's device (the device is current)
ht_status or_module(ht_ctx *c, const char *fn, const OrModule **out) {
    if (c->device < 0 || c->device >= OR_MAX_DEVICES) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": the oriented draw serves devices 0..63");
    std::lock_guard<std::mutex> lock(or_mutex);
    OrModule &m = or_modules[c->device];
    if (!m.mod) {
        const std::string path = or_module_path();
        FILE *fp = std::fopen(path.c_str(), "rb");
        if (!fp) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": an oriented source needs the module " + path + ", which is missing (python -m headtrackr_amd.build makes it)");
        std::fclose(fp);
        OrModule l;
        hipError_t e = hipModuleLoad(&l.mod, path.c_str());
        if (e == hipSuccess) e = hipModuleGetFunction(&l.plain, l.mod, "k_draw_list_oriented");
        if (e == hipSuccess) e = hipModuleGetFunction(&l.turn, l.mod, "k_draw_list_oriented_turn");
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (l.mod) (void)hipModuleUnload(l.mod);
            return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": the module " + path + " could not be loaded: " + hipGetErrorString(e));
        }
        m = l;
    }
    *out = &m;
    return HT_OK;
}

// dw x dh: the destination frames' size — the canvas (dw == 0), or a source's own oriented size (the orient-first pass of the filtered draw
// and the face-patch calls); first .. first + count: the descriptors of the table this launch takes
ht_status or_launch_part(ht_ctx *c, const OrModule &m, bool turn, size_t first, size_t count, uint8_t *dst, size_t dstride, int dw, int dh) {
    if (!count) return HT_OK;
    const uint8_t *tab = c->dl_tab.d + first * sizeof(HtOrientDesc);
    void *args[] = {&tab, &dst, &dstride, &dw, &dh};
    const unsigned tw = turn ? 32 : IG_TW, th = turn ? 32 : IG_TH;
    HT_HIP(c, hipModuleLaunchKernel(turn ? m.turn : m.plain, (dw + tw - 1) / tw, (dh + th - 1) / th, (unsigned)count, IG_NT, 1, 1, 0, c->stream, args, nullptr));
    return HT_OK;
}

// entries of odd rot take the kernel that turns its tile through LDS when the context says so (option orient_lanes; OR_TURN_SHIPPED: what
// the measurement of DESIGN.md §2.3.9 chose); even rot never transposes.  The table is ordered plain entries first — an entry names its
// destination frame itself — and each kind is one launch
constexpr bool OR_TURN_SHIPPED = true;
ht_status or_launch(ht_ctx *c, const char *fn, std::vector<HtOrientDesc> &desc, uint8_t *dst, size_t dstride, int dw = 0, int dh = 0) {
    const OrModule *m = nullptr;
    ht_status st = or_module(c, fn, &m);
    if (st != HT_OK) return st;
    const bool use_turn = c->orient_lanes ? c->orient_lanes == 2 : OR_TURN_SHIPPED;
    const auto plain = [use_turn](const HtOrientDesc &o) { return !(use_turn && (o.orient & 1)); };
    const size_t nplain = (size_t)(std::stable_partition(desc.begin(), desc.end(), plain) - desc.begin());
    if ((st = dl_upload(c, fn, desc)) != HT_OK) return st;
    HtProfScope ps(c, "draw_list_oriented");
    if (!dw) dw = c->W, dh = c->H;
    if ((st = or_launch_part(c, *m, false, 0, nplain, dst, dstride, dw, dh)) != HT_OK) return st;
    return or_launch_part(c, *m, true, nplain, desc.size() - nplain, dst, dstride, dw, dh);
}

// ORIENT FIRST (dm_unpack_sources, ht_draw_calls.hip): each job's whole frame drawn 1 : 1 (ht_orient_whole) onto frames[i], orw x orh packed
// rows.  One table, one launch per job (the frames have sizes of their own)
ht_status or_upright(ht_ctx *c, const char *fn, std::vector<HtOrientDesc> &jobs, const std::vector<uint8_t *> &frames) {
    if (jobs.empty()) return HT_OK;
    const OrModule *m = nullptr;
    ht_status st = or_module(c, fn, &m);
    if (st != HT_OK) return st;
    if ((st = dl_upload(c, fn, jobs)) != HT_OK) return st;
    HtProfScope ps(c, "draw_list_oriented");
    const bool use_turn = c->orient_lanes ? c->orient_lanes == 2 : OR_TURN_SHIPPED;
    for (size_t i = 0; i < jobs.size(); i++)
        if ((st = or_launch_part(c, *m, use_turn && (jobs[i].orient & 1), i, 1, frames[i], 0, jobs[i].orw, jobs[i].orh)) != HT_OK) return st;
    return HT_OK;
}

}  // namespace
