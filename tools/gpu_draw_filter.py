#!/usr/bin/env python3
"""tools/gpu_draw_filter.py [out] — the workload of tools/gpu_draw_list.py (eight feeds, each in an allocation of its own, drawn onto
320x240: 4 x 1080p NV12, 2 x 720p I420 and 2 x 1080p RGBA under a centre-crop rect) through the prefiltered draw, max_factor 8:

  ONE ht_draw_list_filtered_device, in both tile forms (context option draw_filter_rows = 4 | 16: k_draw_list_mean_tile<1> / <4>);
  ONE ht_draw_list_device of the same list (the yardstick kernel, k_draw_list: profiles/draw_list.txt records 8.5 us);
  the route a user had before: per group of entries with equal factors, ht_draw_list_device on a second context whose geometry is
  (Nx W, Ny H) into a scratch buffer, then torch's block mean with the rule's rounding on the SAME stream.

Sets no pass mark; writes what it measured to `out` (default: stdout only).  The committed output is profiles/draw_filter.txt.  Reads
nothing outside the tree.

The routes alternate in blocks in one process.  Reported per route: device time per library kernel (HIP events around each launch:
ht_profile / ht_kernel_times), the stream span of the whole route (torch events on the stream in front of and behind it) and the wall clock
of route + synchronize: per-block medians, the median over blocks and the spread between blocks.  Next to the device times: the source
bytes a call has to read at least once over the kernel time, as a fraction of 8 TB/s.  Before timing, the run prints the factors the
library's own function gives per entry and asserts that every route that filters gives the same bytes."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv_cases as yc  # noqa: E402  (the forward packer)
from headtrackr_amd import api, synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
WARM, BLOCKS, PER_BLOCK = 20, 6, 40
DW, DH, MAX_FACTOR = 320, 240, 8
PEAK = 8e12  # bytes per second
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def centre_crop(w, h):
    cw = h * 4 // 3
    return ((w - cw) // 2, 0, cw, h)


FEEDS = [("nv12", 1920, 1080, "bt709", None)] * 4 + [("i420", 1280, 720, "bt601", None)] * 2 + [("rgba", 1920, 1080, None, centre_crop(1920, 1080))] * 2
K = len(FEEDS)
say(f"# tools/gpu_draw_filter.py: {K} feeds in separate allocations -> {DW}x{DH}, max_factor {MAX_FACTOR}; GPU: {torch.cuda.get_device_name(0)}")
say("# feeds: " + ", ".join(f"{f} {w}x{h}" + (f" rect {r}" if r else "") for f, w, h, _, r in FEEDS))
stream = torch.cuda.Stream()
entries, keep, must_read = [], [], 0
for k, (fmt, w, h, matrix, rect) in enumerate(FEEDS):
    rgb = synth.stream_feed_frames(1, w, h, k)[0]
    rw, rh = (rect[2], rect[3]) if rect else (w, h)
    if fmt == "rgba":
        t = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
        entries.append(dict(format="rgba", width=w, height=h, p0=t.data_ptr(), rect=rect))
        must_read += rw * rh * 4
    else:
        code = yc.FORMATS[fmt]
        t = torch.from_numpy(yc.pack(yc.from_rgb(rgb, code, yc.MATRIX_NAMES.index(matrix)))).cuda()
        cw, ch = yc.chroma_dims(w, h)
        base = t.data_ptr()
        entries.append(dict(format=fmt, width=w, height=h, matrix=matrix, p0=base, p1=base + w * h, p2=base + w * h + cw * ch if fmt == "i420" else None, rect=rect))
        must_read += rw * rh + 2 * ((rw + 1) // 2) * ((rh + 1) // 2)
    keep.append(t)
factors = [tuple(int(v) for v in f) for f in api.draw_filter_factors(entries, DW, DH, MAX_FACTOR)]
say(f"factors (Nx, Ny) per entry: {factors}")
say(f"source bytes under the rects, read at least once by a call that filters: {must_read} ({must_read / 1e6:.2f} MB; {must_read / PEAK * 1e6:.2f} us at 8 TB/s); "
    f"destination bytes: {K * DW * DH * 4}")
fb = DW * DH * 4
dst = {name: torch.zeros((K, DH, DW, 4), dtype=torch.uint8, device="cuda") for name in ("rows4", "rows16", "plain", "two")}
torch.cuda.synchronize()
ctxs = {name: Context(stream=stream.cuda_stream, options="graph_max_frames=0" + opt) for name, opt in (("rows4", ",draw_filter_rows=4"), ("rows16", ",draw_filter_rows=16"), ("plain", ""))}
for c in ctxs.values():
    c.set_geometry(DW, DH, K)
# the route a user had before: one second context per distinct factor pair
groups = {}
for i, f in enumerate(factors):
    groups.setdefault(f, []).append(i)
fine = {}
for (nx, ny), idx in groups.items():
    c = Context(stream=stream.cuda_stream, options="graph_max_frames=0")
    c.set_geometry(nx * DW, ny * DH, 1)
    fine[(nx, ny)] = (c, idx, torch.zeros((len(idx), ny * DH, nx * DW, 4), dtype=torch.uint8, device="cuda"))
say(f"the route a user had before: {len(groups)} groups of equal factors {[(f, len(i)) for f, i in groups.items()]}, each ONE ht_draw_list_device on a context of "
    f"geometry (Nx W, Ny H) + torch's block mean on the same stream")


def route_rows4():
    ctxs["rows4"].draw_list(entries, dst=dst["rows4"].data_ptr(), prefilter=MAX_FACTOR)


def route_rows16():
    ctxs["rows16"].draw_list(entries, dst=dst["rows16"].data_ptr(), prefilter=MAX_FACTOR)


def route_plain():
    ctxs["plain"].draw_list(entries, dst=dst["plain"].data_ptr())


def route_two():
    for (nx, ny), (c, idx, scratch) in fine.items():
        c.draw_list([entries[i] for i in idx], dst=scratch.data_ptr())
        with torch.cuda.stream(stream):
            n = nx * ny
            s = scratch.view(len(idx), DH, ny, DW, nx, 4).to(torch.int32).sum(dim=(2, 4))
            dst["two"][idx] = ((s + (n >> 1)) // n).to(torch.uint8)


ROUTES = {
    "ONE filtered call, tile 64 x 4       ": (route_rows4, [ctxs["rows4"]]),
    "ONE filtered call, tile 64 x 16      ": (route_rows16, [ctxs["rows16"]]),
    "ONE unfiltered call (the yardstick)  ": (route_plain, [ctxs["plain"]]),
    "unfiltered at N x + torch block mean ": (route_two, [c for c, _i, _s in fine.values()]),
}
everyone = [c for _call, cs in ROUTES.values() for c in cs]


def sync():
    for c in everyone:
        c.synchronize()
    torch.cuda.synchronize()


for call, _cs in ROUTES.values():
    for _ in range(WARM):
        call()
sync()
same = bool(torch.equal(dst["rows4"], dst["rows16"])) and bool(torch.equal(dst["rows4"], dst["two"]))
say(f"same bytes from both tile forms and from the route a user had before: {same}; they differ from the unfiltered draw in "
    f"{int((dst['rows4'] != dst['plain']).sum())} of {dst['plain'].numel()} bytes")
assert same
for c in everyone:
    c.profile(True)
wall, span, dev = {k: [] for k in ROUTES}, {k: [] for k in ROUTES}, {k: [] for k in ROUTES}
order = list(ROUTES.items())
for b in range(BLOCKS):
    for name, (call, cs) in order if b % 2 == 0 else order[::-1]:
        ts, sp = [], []
        for _ in range(PER_BLOCK):
            for c in cs:
                c.kernel_times(reset=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            call()
            e1.record(stream)
            for c in cs:
                c.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            sp.append(e0.elapsed_time(e1) * 1e3)
            step = {}
            for c in cs:
                for k, v in c.kernel_times(reset=True).items():
                    if v["launches"]:
                        step[k] = step.get(k, 0.0) + v["ms"] * 1e3
            dev[name].append(step)
        wall[name].append(float(np.median(ts)))
        span[name].append(float(np.median(sp)))
for c in everyone:
    c.profile(False)
say(f"## per call (all {K} feeds): blocks of {PER_BLOCK} calls, {BLOCKS} blocks per route, alternated; profiling on (its events are inside the wall clock and the span of every route)")
for name in ROUTES:
    timers = sorted({k for s in dev[name] for k in s})
    per = ", ".join(f"{k}: {np.median([s[k] for s in dev[name] if k in s]):.2f} us (min {min(s[k] for s in dev[name] if k in s):.2f}, max {max(s[k] for s in dev[name] if k in s):.2f})"
                    for k in timers)
    say(f"{name}: device {per}; stream span {float(np.median(span[name])):.1f} us; wall ms per route + sync, median of each block {[round(v, 4) for v in wall[name]]}; "
        f"median {float(np.median(wall[name])):.4f} ms, spread between blocks {max(wall[name]) - min(wall[name]):.4f} ms")
    if "filtered call" in name and "un" not in name:
        t = float(np.median([s["draw_list_mean"] for s in dev[name] if "draw_list_mean" in s]))
        say(f"    {must_read} source bytes in {t:.2f} us: {must_read / (t * 1e-6) / 1e12:.2f} TB/s, {must_read / (t * 1e-6) / PEAK * 100:.1f} % of 8 TB/s")
names = list(ROUTES)
spread = max(max(v) - min(v) for v in wall.values())
for a, b in ((names[0], names[1]), (names[0], names[3]), (names[1], names[3]), (names[0], names[2])):
    ma, mb = float(np.median(wall[a])), float(np.median(wall[b]))
    sa, sb = float(np.median(span[a])), float(np.median(span[b]))
    say(f"{a.strip()} / {b.strip()}: {ma / mb:.3f} x the wall time, {sa / sb:.3f} x the stream span; wall difference {ma - mb:+.4f} ms against a largest spread between blocks of {spread:.4f} ms")
# the two tile forms below max_factor 8: does one tile serve every factor?  Device time of the kernel alone, the forms alternating in blocks
say("## the tile forms at smaller max_factor: device time of draw_list_mean per call, median over 3 blocks of 40 calls per form, alternated (min .. max)")
for c in (ctxs["rows4"], ctxs["rows16"]):
    c.profile(True)
for mf in (4, 3, 2, 1):
    got = {"rows4": [], "rows16": []}
    fs = sorted({tuple(int(v) for v in f) for f in api.draw_filter_factors(entries, DW, DH, mf)})
    for name in got:
        for _ in range(WARM):
            ctxs[name].draw_list(entries, dst=dst[name].data_ptr(), prefilter=mf)
        ctxs[name].synchronize()
    for b in range(6):
        name = ("rows4", "rows16")[b % 2]
        for _ in range(PER_BLOCK):
            ctxs[name].kernel_times(reset=True)
            ctxs[name].draw_list(entries, dst=dst[name].data_ptr(), prefilter=mf)
            ctxs[name].synchronize()
            got[name].append(ctxs[name].kernel_times(reset=True)["draw_list_mean"]["ms"] * 1e3)
    assert bool(torch.equal(dst["rows4"], dst["rows16"]))
    say(f"max_factor {mf} (factors {fs}): tile 64 x 4 {np.median(got['rows4']):.2f} us ({min(got['rows4']):.2f} .. {max(got['rows4']):.2f}); "
        f"tile 64 x 16 {np.median(got['rows16']):.2f} us ({min(got['rows16']):.2f} .. {max(got['rows16']):.2f})")
for c in (ctxs["rows4"], ctxs["rows16"]):
    c.profile(False)
for c in everyone:
    c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
