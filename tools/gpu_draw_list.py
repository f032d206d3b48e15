#!/usr/bin/env python3
"""tools/gpu_draw_list.py [out] — eight feeds, each in an allocation of its own, drawn onto 320x240: 4 x 1080p NV12, 2 x 720p I420 and
2 x 1080p RGBA under a centre-crop rect (the 4 : 3 window of a 16 : 9 frame), once through ONE ht_draw_list_device and once through the
single-source entry points, one call per feed (ht_draw_frames_yuv_device / ht_draw_frames_device: unchanged, the baseline).  Sets no pass
mark; writes what it measured to `out` (default: stdout only).  The committed output is profiles/draw_list.txt.  Reads nothing outside the
tree.

The two routes alternate in blocks in one process.  Reported: device time per kernel (HIP events around each launch: ht_profile /
ht_kernel_times), summed per step, and the wall clock of a step (enqueue of all eight feeds + one ht_synchronize): per-block medians,
the median over blocks and the spread between the blocks of one route.  The two results are compared byte for byte first."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv_cases as yc  # noqa: E402  (the forward packer)
from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
WARM, BLOCKS, PER_BLOCK = 20, 6, 40
DW, DH = 320, 240
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def centre_crop(w, h):
    cw = h * 4 // 3
    return ((w - cw) // 2, 0, cw, h)


FEEDS = [("nv12", 1920, 1080, "bt709", None)] * 4 + [("i420", 1280, 720, "bt601", None)] * 2 + [("rgba", 1920, 1080, None, centre_crop(1920, 1080))] * 2
say(f"# tools/gpu_draw_list.py: {len(FEEDS)} feeds in separate allocations -> {DW}x{DH}; GPU: {torch.cuda.get_device_name(0)}")
say("# feeds: " + ", ".join(f"{f} {w}x{h}" + (f" rect {r}" if r else "") for f, w, h, _, r in FEEDS))
entries, keep = [], []
for k, (fmt, w, h, matrix, rect) in enumerate(FEEDS):
    rgb = synth.stream_feed_frames(1, w, h, k)[0]
    if fmt == "rgba":
        t = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
        entries.append(dict(format="rgba", width=w, height=h, p0=t.data_ptr(), rect=rect))
    else:
        code = yc.FORMATS[fmt]
        t = torch.from_numpy(yc.pack(yc.from_rgb(rgb, code, yc.MATRIX_NAMES.index(matrix)))).cuda()
        cw, ch = yc.chroma_dims(w, h)
        base = t.data_ptr()
        entries.append(dict(format=fmt, width=w, height=h, matrix=matrix, p0=base, p1=base + w * h, p2=base + w * h + cw * ch if fmt == "i420" else None, rect=rect))
    keep.append(t)
fb = DW * DH * 4
dst_list = torch.zeros((len(FEEDS), DH, DW, 4), dtype=torch.uint8, device="cuda")
dst_each = torch.zeros_like(dst_list)
c = Context(options="graph_max_frames=0")
c.set_geometry(DW, DH, len(FEEDS))


def route_list():
    c.draw_list(entries, dst=dst_list.data_ptr())


def route_each():
    for k, e in enumerate(entries):
        d = dst_each.data_ptr() + k * fb
        if e["format"] == "rgba":
            c.draw_frames_device(e["p0"], 1, e["width"], e["height"], rect=e["rect"], dst=d)
        else:
            c.draw_frames_yuv_device(e["p0"], e["p1"], e["p2"], 1, e["width"], e["height"], e["format"], e["matrix"], rect=e["rect"], dst=d)


for call in (route_list, route_each):
    for _ in range(WARM):
        call()
c.synchronize()
say(f"same bytes from both routes: {bool(torch.equal(dst_list, dst_each))}")
c.profile(True)
wall = {"list": [], "each": []}
dev = {"list": [], "each": []}
for b in range(BLOCKS):
    for name, call in (("list", route_list), ("each", route_each)) if b % 2 == 0 else (("each", route_each), ("list", route_list)):
        ts, ds = [], []
        for _ in range(PER_BLOCK):
            c.kernel_times(reset=True)
            t0 = time.perf_counter()
            call()
            c.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            kt = c.kernel_times(reset=True)
            ds.append({k: (v["ms"] * 1e3, v["launches"]) for k, v in kt.items() if k.startswith("draw_")})
        wall[name].append(float(np.median(ts)))
        dev[name].append(ds)
c.profile(False)
say(f"## per step (all {len(FEEDS)} feeds), blocks of {PER_BLOCK} steps, {BLOCKS} blocks per route, alternated; profiling on (its events are inside the wall clock of both routes)")
for name, what in (("list", "ONE ht_draw_list_device          "), ("each", "one single-source call per feed ")):
    steps = [s for blk in dev[name] for s in blk]
    timers = sorted({k for s in steps for k in s})
    per = ", ".join(f"{k}: {np.median([s[k][0] for s in steps if k in s]):.2f} us in {int(np.median([s[k][1] for s in steps if k in s]))} launches" for k in timers)
    total = float(np.median([sum(v[0] for v in s.values()) for s in steps]))
    m = float(np.median(wall[name]))
    say(f"{what}: device {total:8.2f} us per step ({per}); wall ms per step, median of each block {[round(v, 4) for v in wall[name]]}; median {m:.4f} ms, "
        f"spread between blocks {max(wall[name]) - min(wall[name]):.4f} ms")
ml, me = float(np.median(wall["list"])), float(np.median(wall["each"]))
spread = max(max(wall[k]) - min(wall[k]) for k in wall)
say(f"list / each: {ml / me:.3f} x the wall time per step; difference {me - ml:+.4f} ms against a largest spread between blocks of {spread:.4f} ms")
c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
