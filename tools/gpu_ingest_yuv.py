#!/usr/bin/env python3
"""tools/gpu_ingest_yuv.py [out] — what taking YUV 4:2:0 frames directly costs and buys, on the shape the path exists for (8 resident
1920x1080 feeds).  Sets no pass mark; writes what it measured to `out` (default: stdout only).  The committed output is
profiles/ingest_yuv.txt.  Reads nothing outside the tree.

Part 1, device time (HIP events on the context's stream: ht_profile / ht_kernel_times), one process, median of CALLS single calls after
a warm-up: k_draw_yuv<NV12> and k_draw_yuv<I420> (timer `draw_yuv`) next to k_draw_frames (timer `draw_frames`) on the SAME content — the
RGBA frames are the declared conversion of the planes — at 8 x 1920x1080 -> 320x240 and 8 x 1920x1080 -> 1920x1080.  The two results are
compared byte for byte first.

Part 2, wall clock of host upload + draw (a call that ends in a wait) for the same eight feeds, as NV12 through ht_draw_frames_yuv
(3.1 MB per frame over the link) against RGBA through ht_draw_frames (8.3 MB per frame), from pinned host memory, in alternating blocks
in one process: per-block medians, then the median over blocks and the spread between blocks of one route."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv_cases as yc  # noqa: E402  (the numpy restatement of the declared conversion and the forward packer)
from headtrackr_amd import native, synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
CALLS, WARM, BLOCKS, PER_BLOCK = 60, 10, 6, 20
K, SW, SH = 8, 1920, 1080
MATRIX = 1  # BT.709 limited: what a 1080p decoder delivers
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


def rows_touched(sh, dh):
    j = np.arange(dh, dtype=np.float64)
    f = np.clip((j + 0.5) * (sh / dh) - 0.5, 0.0, sh - 1.0)
    a = np.floor(f).astype(np.int64)
    return len(set(a.tolist()) | set(np.minimum(a + 1, sh - 1).tolist()))


say(f"# tools/gpu_ingest_yuv.py: {K} x {SW}x{SH} feeds, matrix {yc.MATRIX_NAMES[MATRIX]}; GPU: {torch.cuda.get_device_name(0)}")
rgb = synth.stream_feed_frames(K, SW, SH, 0)
planes = {fmt: [yc.from_rgb(rgb[f], fmt, MATRIX) for f in range(K)] for fmt in (yc.NV12, yc.I420)}
rgba = np.stack([yc.to_rgba(planes[yc.NV12][f], SW, SH, yc.NV12, MATRIX) for f in range(K)])  # the same content as the planes hold
packed = {fmt: np.stack([yc.pack(p) for p in planes[fmt]]) for fmt in planes}
FSZ = yc.frame_bytes(SW, SH)
d_rgba = torch.from_numpy(rgba).cuda()
d_yuv = {fmt: torch.from_numpy(packed[fmt]).cuda() for fmt in packed}

say(f"## device time, median [min .. max] of {CALLS} calls after {WARM} warm-up calls (HIP events around each launch)")
for dw, dh in ((320, 240), (1920, 1080)):
    dst = torch.empty((K, dh, dw, 4), dtype=torch.uint8, device="cuda")
    dst2 = torch.empty_like(dst)
    c = Context(options="graph_max_frames=0")
    c.set_geometry(dw, dh, K)
    c.draw_frames_device(d_rgba.data_ptr(), K, SW, SH, dst=dst.data_ptr())
    t_rgba = medians(c, lambda: c.draw_frames_device(d_rgba.data_ptr(), K, SW, SH, dst=dst.data_ptr()), "draw_frames")
    touched = rows_touched(SH, dh)
    say(f"{K} x {SW}x{SH} -> {dw}x{dh}: k_draw_frames on RGBA      {t_rgba[0]:9.2f} us [{t_rgba[1]:.2f} .. {t_rgba[2]:.2f}]   ({touched} of {SH} source rows named; "
        f"{K * touched * SW * 4 / 1e6:.1f} MB of source rows + {K * dw * dh * 4 / 1e6:.1f} MB written)")
    for fmt, name in ((yc.NV12, "NV12"), (yc.I420, "I420")):
        base = d_yuv[fmt].data_ptr()
        y, u = base, base + SW * SH
        v = u + (SW // 2) * (SH // 2) if fmt == yc.I420 else None

        def draw(out=dst2):
            c.draw_frames_yuv_device(y, u, v, K, SW, SH, fmt, MATRIX, stride=FSZ, dst=out.data_ptr())

        draw()
        c.synchronize()
        equal = bool(torch.equal(dst, dst2))
        t = medians(c, draw, "draw_yuv")
        say(f"{K} x {SW}x{SH} -> {dw}x{dh}: k_draw_yuv<{name}>           {t[0]:9.2f} us [{t[1]:.2f} .. {t[2]:.2f}]   = {t[0] / t_rgba[0]:.2f} x k_draw_frames; "
            f"{K * touched * SW * 1.5 / 1e6:.1f} MB of source rows; same bytes as the RGBA draw: {equal}")
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
h_rgba, h_nv12 = pinned(rgba), pinned(packed[yc.NV12])


def route_rgba():
    assert L.ht_draw_frames(c._h, h_rgba, K, SW, SH, 0, None) == 0
    c.synchronize()


def route_nv12():
    assert L.ht_draw_frames_yuv(c._h, h_nv12, K, SW, SH, yc.NV12, MATRIX, 0, None) == 0
    c.synchronize()


for call in (route_rgba, route_nv12):
    for _ in range(WARM):
        call()
blocks = {"rgba": [], "nv12": []}
for b in range(BLOCKS):
    for name, call in (("rgba", route_rgba), ("nv12", route_nv12)) if b % 2 == 0 else (("nv12", route_nv12), ("rgba", route_rgba)):
        ts = []
        for _ in range(PER_BLOCK):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        blocks[name].append(float(np.median(ts)))
for name, nbytes, what in (("rgba", rgba.nbytes, "RGBA through ht_draw_frames    "), ("nv12", packed[yc.NV12].nbytes, "NV12 through ht_draw_frames_yuv")):
    m = float(np.median(blocks[name]))
    say(f"{what}: {nbytes / 1e6:6.1f} MB per call; wall ms per call, median of each block {[round(v, 3) for v in blocks[name]]}; median {m:.3f} ms, "
        f"spread between blocks {max(blocks[name]) - min(blocks[name]):.3f} ms; {nbytes / m / 1e6:.1f} GB/s of source bytes; {K / m * 1e3:.0f} frames/s")
mr, mn = float(np.median(blocks["rgba"])), float(np.median(blocks["nv12"]))
say(f"NV12 / RGBA: {mn / mr:.3f} x the wall time for {packed[yc.NV12].nbytes / rgba.nbytes:.3f} x the bytes")
L.ht_host_free(h_rgba)
L.ht_host_free(h_nv12)
c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
