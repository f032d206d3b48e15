"""The camshift schedule table (headtrackr_amd/csrc/ht_cs_schedule.h) restated in Python, for two users: tests/test_cs_schedule_cpu.py
holds it against the header itself (compiled into tests/host/cs_schedule_harness.cc) on every recorded case, and
tests/test_gpu_camshift_paths.py computes from the device's CU count which timers a default-option track() call must report.
Integer arithmetic only; `//` on non-negative operands is C's `/`."""

HIST_NT, HIST_MAXCHUNKS, HIST_TARGET_WGS = 1024, 128, 256
FUSED_NT, FUSED_NT_SMALL = 1024, 512
REGION_CAP, REGION_CAP_SMALL = 40960, 22528
CL_MAXG, CL_MAX_STREAMS = 32, 64
DEFAULTS = dict(num_cus=256, cs_fused_min=192, cs_cluster=1, cs_cluster_min_px=10000, cs_iters=10, cs_region=REGION_CAP, cs_fused_nt=0, other_busy=0)


def max_chunks(nstreams):
    return min(HIST_MAXCHUNKS, max(8, HIST_TARGET_WGS // max(nstreams, 1)))


def chunk_plan(npix, nstreams):
    """(max_chunks, chunk_px, nchunks) of the histogram pass for npix pixels per frame and nstreams frames"""
    mc = max_chunks(nstreams)
    n = max(min((npix + 16383) // 16384, mc), 1)
    q = 4 * HIST_NT
    chunk_px = max(((npix + n - 1) // n + q - 1) // q * q, q)
    return mc, chunk_px, max((npix + chunk_px - 1) // chunk_px, 1)


def track_plan(n, w, h, reserved=None, **opts):
    """form ("FUSED_1024" | "FUSED_512" | "CLUSTER" | "PER_STREAM"), G, region_cap, dynamic LDS bytes and timers of one track() call"""
    o = dict(DEFAULTS, **opts)
    npix = w * h
    if n >= o["cs_fused_min"]:
        nt = o["cs_fused_nt"] if o["cs_fused_nt"] in (FUSED_NT, FUSED_NT_SMALL) else (FUSED_NT_SMALL if n > o["num_cus"] or o["other_busy"] else FUSED_NT)
        small = nt == FUSED_NT_SMALL
        return dict(form="FUSED_512" if small else "FUSED_1024", G=0, grid=n, block=nt, lds=2 * (REGION_CAP_SMALL if small else REGION_CAP),
                    region_cap=min(o["cs_region"], REGION_CAP_SMALL) if small else o["cs_region"], timers=["cs_track_512" if small else "cs_track"])
    G = min(CL_MAXG, o["num_cus"] // max(n, 1))
    cluster = bool(o["cs_cluster"]) and n <= CL_MAX_STREAMS and G >= 4 and npix >= o["cs_cluster_min_px"] and o["cs_iters"] > 0
    _mc, chunk_px, nchunks = chunk_plan(npix, n if reserved is None else reserved)
    if cluster:
        return dict(form="CLUSTER", G=G, grid=n * G, block=512, lds=0, region_cap=0, chunk_px=chunk_px, nchunks=nchunks, timers=["cs_hist", "cs_lut", "cs_meanshift"])
    return dict(form="PER_STREAM", G=G, grid=n, block=512, lds=2 * REGION_CAP, region_cap=o["cs_region"], chunk_px=chunk_px, nchunks=nchunks,
                timers=["cs_hist", "cs_meanshift"])


def init_plan(n, tallest, num_cus=256):
    """(G, rows form?) of initTracker for n streams whose tallest rect has `tallest` rows"""
    G = min(min(32, max(1, num_cus * 2 // max(n, 1))), (tallest + 15) // 16)
    return G, n < 64 and G >= 2
