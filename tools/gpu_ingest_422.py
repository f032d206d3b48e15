#!/usr/bin/env python3
"""tools/gpu_ingest_422.py [out] — what taking packed YUV 4:2:2 frames (YUYV / UYVY) directly costs and buys, on the shape the path exists
for (8 resident 1920x1080 feeds).  Sets no pass mark; writes what it measured to `out` (default: stdout only).  The committed output is
profiles/ingest_422.txt.  Reads nothing outside the tree.

Part 1, device time (HIP events on the context's stream: ht_profile / ht_kernel_times), one process, median of CALLS single calls after a
warm-up: the packed draw (ht_draw_frames_yuv_device with YUYV and UYVY: k_draw_list_mean_tile<4> at factors (1, 1), timer `draw_list_mean`)
next to k_draw_yuv<NV12> (`draw_yuv`) and k_draw_frames (`draw_frames`) on the SAME content — the packed frames are the NV12 frames with
every chroma row written twice, the RGBA frames their declared conversion — at 8 x 1920x1080 -> 320x240 and -> 1920x1080.  The results are
compared byte for byte first.

Part 2, wall clock of host upload + draw (a call that ends in a wait) for the same eight feeds as YUYV (4.1 MB per frame over the link)
against NV12 (3.1 MB) and RGBA (8.3 MB), from pinned host memory, in alternating blocks in one process: per-block medians, then the median
over blocks and the spread between blocks of one route."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv422_cases as y4  # noqa: E402  (the numpy restatement of the packed layout)
import yuv_cases as yc  # noqa: E402
from headtrackr_amd import native, synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
CALLS, WARM, BLOCKS, PER_BLOCK = 60, 10, 6, 20
K, SW, SH = 8, 1920, 1080
MATRIX = 1
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def medians(c, call, name):
    for _ in range(WARM):
        call()
    c.synchronize()
    c.profile(True)
    c.kernel_times(reset=True)
    rows = []
    for _ in range(CALLS):
        call()
        c.synchronize()
        rows.append(c.kernel_times(reset=True)[name]["ms"] * 1e3)
    c.profile(False)
    return float(np.median(rows)), float(np.min(rows)), float(np.max(rows))


say(f"# tools/gpu_ingest_422.py: {K} x {SW}x{SH} feeds, matrix {yc.MATRIX_NAMES[MATRIX]}; GPU: {torch.cuda.get_device_name(0)}")
rgb = synth.stream_feed_frames(K, SW, SH, 0)
i420 = [yc.from_rgb(rgb[f], yc.I420, MATRIX) for f in range(K)]
nv12 = np.stack([yc.pack(yc.join(*p, yc.NV12)) for p in i420])
packed = {fmt: np.stack([y4.from_i420(p, fmt).reshape(-1) for p in i420]) for fmt in (y4.YUYV, y4.UYVY)}
rgba = np.stack([yc.to_rgba(p, SW, SH, yc.I420, MATRIX) for p in i420])  # the same content as every layout above holds
FSZ, FSZ422 = yc.frame_bytes(SW, SH), y4.frame_bytes(SW, SH)
d_rgba, d_nv12 = torch.from_numpy(rgba).cuda(), torch.from_numpy(nv12).cuda()
d_422 = {fmt: torch.from_numpy(packed[fmt]).cuda() for fmt in packed}

say(f"## device time, median [min .. max] of {CALLS} calls after {WARM} warm-up calls (HIP events around each launch)")
for dw, dh in ((320, 240), (1920, 1080)):
    dst = torch.empty((K, dh, dw, 4), dtype=torch.uint8, device="cuda")
    dst2 = torch.empty_like(dst)
    c = Context(options="graph_max_frames=0")
    c.set_geometry(dw, dh, K)
    c.draw_frames_device(d_rgba.data_ptr(), K, SW, SH, dst=dst.data_ptr())
    t_rgba = medians(c, lambda: c.draw_frames_device(d_rgba.data_ptr(), K, SW, SH, dst=dst.data_ptr()), "draw_frames")
    say(f"{K} x {SW}x{SH} -> {dw}x{dh}: k_draw_frames on RGBA            {t_rgba[0]:9.2f} us [{t_rgba[1]:.2f} .. {t_rgba[2]:.2f}]")
    base = d_nv12.data_ptr()
    t = medians(c, lambda: c.draw_frames_yuv_device(base, base + SW * SH, None, K, SW, SH, yc.NV12, MATRIX, stride=FSZ, dst=dst2.data_ptr()), "draw_yuv")
    c.synchronize()
    say(f"{K} x {SW}x{SH} -> {dw}x{dh}: k_draw_yuv<NV12>                 {t[0]:9.2f} us [{t[1]:.2f} .. {t[2]:.2f}]   = {t[0] / t_rgba[0]:.2f} x k_draw_frames; "
        f"same bytes as the RGBA draw: {bool(torch.equal(dst, dst2))}")
    for fmt in (y4.YUYV, y4.UYVY):
        dst2.zero_()
        p = d_422[fmt].data_ptr()

        def draw(p=p, fmt=fmt):
            c.draw_frames_yuv_device(p, None, None, K, SW, SH, fmt, MATRIX, stride=FSZ422, dst=dst2.data_ptr())

        t = medians(c, draw, "draw_list_mean")
        c.synchronize()
        say(f"{K} x {SW}x{SH} -> {dw}x{dh}: {y4.FORMAT_NAMES[fmt].upper()} (k_draw_list_mean_tile<4>)  {t[0]:9.2f} us [{t[1]:.2f} .. {t[2]:.2f}]   = {t[0] / t_rgba[0]:.2f} x k_draw_frames; "
            f"same bytes as the RGBA draw: {bool(torch.equal(dst, dst2))}")
    c.close()
    del dst, dst2

say()
say(f"## wall clock, host upload + draw -> 320x240, {K} feeds from pinned host memory; blocks of {PER_BLOCK} calls, {BLOCKS} blocks per route, alternated")
L = native.lib()


def pinned(arr):
    p = C.c_void_p()
    assert L.ht_host_alloc(arr.nbytes, C.byref(p)) == 0
    C.memmove(p.value, arr.ctypes.data, arr.nbytes)
    return p.value


c = Context()
c.set_geometry(320, 240, K)
hosts = {"rgba": (pinned(rgba), rgba.nbytes), "nv12": (pinned(nv12), nv12.nbytes), "yuyv": (pinned(packed[y4.YUYV]), packed[y4.YUYV].nbytes)}


def route(name):
    ptr = hosts[name][0]
    if name == "rgba":
        assert L.ht_draw_frames(c._h, ptr, K, SW, SH, 0, None) == 0
    else:
        assert L.ht_draw_frames_yuv(c._h, ptr, K, SW, SH, yc.NV12 if name == "nv12" else y4.YUYV, MATRIX, 0, None) == 0
    c.synchronize()


order = ["rgba", "nv12", "yuyv"]
for name in order:
    for _ in range(WARM):
        route(name)
blocks = {name: [] for name in order}
for b in range(BLOCKS):
    for name in order[b % 3:] + order[:b % 3]:  # every route leads a block twice
        ts = []
        for _ in range(PER_BLOCK):
            t0 = time.perf_counter()
            route(name)
            ts.append((time.perf_counter() - t0) * 1e3)
        blocks[name].append(float(np.median(ts)))
med = {}
for name in order:
    m = med[name] = float(np.median(blocks[name]))
    nbytes = hosts[name][1]
    say(f"{name.upper():4s}: {nbytes / 1e6:6.1f} MB per call; wall ms per call, median of each block {[round(v, 3) for v in blocks[name]]}; median {m:.3f} ms, "
        f"spread between blocks {max(blocks[name]) - min(blocks[name]):.3f} ms; {nbytes / m / 1e6:.1f} GB/s of source bytes; {K / m * 1e3:.0f} frames/s")
say(f"YUYV / RGBA: {med['yuyv'] / med['rgba']:.3f} x the wall time for {hosts['yuyv'][1] / hosts['rgba'][1]:.3f} x the bytes; "
    f"YUYV / NV12: {med['yuyv'] / med['nv12']:.3f} x the wall time for {hosts['yuyv'][1] / hosts['nv12'][1]:.3f} x the bytes")
for name in order:
    L.ht_host_free(hosts[name][0])
c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
