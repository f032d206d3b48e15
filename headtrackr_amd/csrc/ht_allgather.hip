// ht_allgather.hip — multi-GPU: in-place all-gather of fixed-size records over RCCL (xGMI), single-process form for the Node host.
// (bench.py / torch.distributed use one process per GPU and call RCCL through torch instead.)  Host code only: no kernel, no code
// object, like ht_context.hip.
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: librccl.so is opened lazily (dlopen) the first time ht_allgather_records runs

#include "ht_internal.h"

namespace {
struct CommSet {
    std::vector<int> devs;
    std::vector<ncclComm_t> comms;
};
std::map<std::vector<int>, CommSet> g_comms;

struct Rccl {
    void *h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
Rccl &rccl() {
    static Rccl r;
    if (r.h) return r;
    r.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!r.h) r.h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!r.h) r.h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!r.h) return r;
    r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(r.h, "ncclCommInitAll"));
    r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.h, "ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.h, "ncclGroupEnd"));
    r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.h, "ncclAllGather"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.h, "ncclGetErrorString"));
    r.ok = r.CommInitAll && r.GroupStart && r.GroupEnd && r.AllGather && r.GetErrorString;
    return r;
}
}  // namespace

extern "C" ht_status ht_allgather_records(ht_ctx *const *ctxs, int32_t nranks, void *const *records_dev, size_t bytes_per_rank) {
    if (!ctxs || !records_dev || nranks <= 0 || bytes_per_rank == 0) return HT_ERR_INVALID;
    if (nranks == 1 && ctxs[0] && !ctxs[0]->force_rccl) return HT_OK;  // (option force_rccl runs RCCL with one rank: dlopen + ncclCommInitAll + ncclAllGather on a 1-GPU box)
    std::vector<int> devs(nranks);
    for (int i = 0; i < nranks; i++) {
        if (!ctxs[i] || !records_dev[i]) return HT_ERR_INVALID;
        devs[i] = ctxs[i]->device;
    }
    Rccl &R = rccl();
    if (!R.ok) return ht_fail(ctxs[0], HT_ERR_HIP, "ht_allgather_records: librccl.so could not be loaded");
    auto it = g_comms.find(devs);
    if (it == g_comms.end()) {
        CommSet cs;
        cs.devs = devs;
        cs.comms.resize(nranks);
        if (R.CommInitAll(cs.comms.data(), nranks, devs.data()) != ncclSuccess)
            return ht_fail(ctxs[0], HT_ERR_HIP, "ht_allgather_records: ncclCommInitAll failed");
        it = g_comms.emplace(devs, cs).first;
    }
    ncclResult_t r = R.GroupStart();
    for (int i = 0; i < nranks && r == ncclSuccess; i++) {
        char *buf = static_cast<char *>(records_dev[i]);
        r = R.AllGather(buf + (size_t)i * bytes_per_rank, buf, bytes_per_rank, ncclChar, it->second.comms[i], ctxs[i]->stream);
    }
    if (r == ncclSuccess) r = R.GroupEnd();
    if (r != ncclSuccess) return ht_fail(ctxs[0], HT_ERR_HIP, std::string("ht_allgather_records: ") + R.GetErrorString(r));
    for (int i = 0; i < nranks; i++) {
        HT_HIP(ctxs[i], hipSetDevice(ctxs[i]->device));
        HT_HIP(ctxs[i], hipStreamSynchronize(ctxs[i]->stream));
    }
    return HT_OK;
}

extern "C" int32_t ht_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// Single-process multi-GPU exchange of the per-frame bounding boxes: rank i's ht_best_faces output goes into slot i of a
// device buffer on ITS GPU, one ncclAllGather per rank over xGMI, then every rank's gathered table is read back and compared —
// all ranks must hold the same table — and the table is returned.
extern "C" ht_status ht_allgather_best_faces(ht_ctx *const *ctxs, int32_t nranks, const ht_rect *const *best, int32_t frames_per_rank, ht_rect *gathered) {
    if (!ctxs || !best || !gathered || nranks <= 0 || frames_per_rank <= 0) return HT_ERR_INVALID;
    const size_t per = sizeof(ht_rect) * (size_t)frames_per_rank, total = per * (size_t)nranks;
    std::vector<void *> bufs(nranks, nullptr);
    for (int i = 0; i < nranks; i++) {
        ht_ctx *c = ctxs[i];
        if (!c || !best[i]) return HT_ERR_INVALID;
        HT_HIP(c, hipSetDevice(c->device));
        if (c->d_gather_bytes < total) {
            HT_HIP(c, hipStreamSynchronize(c->stream));
            if (c->d_gather) (void)hipFree(c->d_gather);
            c->d_gather = nullptr;
            c->d_gather_bytes = 0;
            if (hipMalloc(&c->d_gather, total) != hipSuccess) return ht_fail(c, HT_ERR_NOMEM, "ht_allgather_best_faces: hipMalloc failed");
            c->d_gather_bytes = total;
        }
        HT_HIP(c, hipMemsetAsync(c->d_gather, 0, total, c->stream));
        HT_HIP(c, hipMemcpyAsync(static_cast<char *>(c->d_gather) + (size_t)i * per, best[i], per, hipMemcpyHostToDevice, c->stream));
        HT_HIP(c, hipStreamSynchronize(c->stream));  // best[i] is the caller's pageable memory
        bufs[i] = c->d_gather;
    }
    ht_status st = ht_allgather_records(ctxs, nranks, bufs.data(), per);
    if (st != HT_OK) return st;
    std::vector<char> other(total);
    for (int i = 0; i < nranks; i++) {
        ht_ctx *c = ctxs[i];
        HT_HIP(c, hipSetDevice(c->device));
        HT_HIP(c, hipMemcpy(i == 0 ? reinterpret_cast<char *>(gathered) : other.data(), c->d_gather, total, hipMemcpyDeviceToHost));
        if (i > 0 && std::memcmp(other.data(), gathered, total) != 0)
            return ht_fail(ctxs[0], HT_ERR_HIP, "ht_allgather_best_faces: rank " + std::to_string(i) + " holds a different table than rank 0 after the all-gather");
    }
    return HT_OK;
}
