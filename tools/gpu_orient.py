#!/usr/bin/env python3
"""tools/gpu_orient.py [out] — the oriented draw measured: eight resident 1080p NV12 feeds, each in an allocation of its own, declared
rot 1 (a phone in portrait) and drawn onto a 240x320 canvas.  Sets no pass mark; writes what it measured to `out` (default: stdout only).
The committed output is profiles/orient.txt.  Reads nothing outside the tree.

Per row the routes alternate in blocks in one process:
  (a)  ONE oriented ht_draw_list_device — for odd rot in both lane mappings that are built (context option orient_lanes = 1: lanes along
       O's x, k_draw_list_oriented; = 2: lanes along the stored row, the tile turned through LDS, k_draw_list_oriented_turn);
  (b)  the same list with the orientation bits cleared, onto the canvas with its sides swapped: the unoriented floor (k_draw_list);
  (c)  the two-pass route: every feed oriented 1 : 1 into an RGBA frame of its own size (the oriented draw onto a canvas of O's size: what
       the calls that orient first pay), then ht_draw_list_device on those RGBA frames.
Rows: rot 1 -> 240x320; rot 2 and flip -> 320x240 (no transpose); 1 : 1, rot 1 -> 1080x1920 (the transposing tile matters most).
Reported: device time per kernel (HIP events around each launch: ht_profile / ht_kernel_times), summed per step, and the wall clock of a
step (enqueue + one ht_synchronize): the median over the per-block medians and the spread between the blocks of one route.  (a) and (c)
are compared byte for byte first."""
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
WARM, BLOCKS, PER_BLOCK = 20, 6, 200
N, SW, SH = 8, 1920, 1080
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/gpu_orient.py: {N} feeds of {SW}x{SH} NV12 in separate allocations; GPU: {torch.cuda.get_device_name(0)}")
stream = torch.cuda.current_stream()
keep, feeds = [], []
cw, ch = yc.chroma_dims(SW, SH)
for k in range(N):
    rgb = synth.stream_feed_frames(1, SW, SH, k)[0]
    t = torch.from_numpy(yc.pack(yc.from_rgb(rgb, yc.NV12, 1))).cuda()
    keep.append(t)
    feeds.append(dict(format="nv12", width=SW, height=SH, matrix="bt709", p0=t.data_ptr(), p1=t.data_ptr() + SW * SH))
contexts = {}


def ctx(w, h, lanes=0):
    """one context per geometry and lane mapping, all on one stream"""
    key = (w, h, lanes)
    if key not in contexts:
        c = Context(stream=stream.cuda_stream, options="graph_max_frames=0" + (f",orient_lanes={lanes}" if lanes else ""))
        c.set_geometry(w, h, N)
        contexts[key] = c
    return contexts[key]


def oriented(k):
    return [dict(e, orientation=k) for e in feeds]


def measure(title, routes):
    """routes: [(label, callable, [contexts whose timers count])]"""
    for _label, call, _cs in routes:
        for _ in range(WARM):
            call()
    torch.cuda.synchronize()
    used = {id(c): c for _l, _c, cs in routes for c in cs}.values()
    for c in used:
        c.profile(True)
    wall = {label: [] for label, _c, _cs in routes}
    dev = {label: [] for label, _c, _cs in routes}
    for b in range(BLOCKS):
        for label, call, cs in (routes if b % 2 == 0 else routes[::-1]):
            ts = []
            for _ in range(PER_BLOCK):
                for c in cs:
                    c.kernel_times(reset=True)
                t0 = time.perf_counter()
                call()
                cs[-1].synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                step = {}
                for c in cs:
                    for name, v in c.kernel_times(reset=True).items():
                        if name.startswith("draw_"):
                            us, n = step.get(name, (0.0, 0))
                            step[name] = (us + v["ms"] * 1e3, n + v["launches"])
                dev[label].append(step)
            wall[label].append(float(np.median(ts)))
    for c in used:
        c.profile(False)
    say(f"## {title}: blocks of {PER_BLOCK} steps, {BLOCKS} blocks per route, alternated; profiling on (its events are inside the wall clock of every route)")
    for label, _call, _cs in routes:
        steps = dev[label]
        timers = sorted({k for s in steps for k in s})
        per = ", ".join(f"{k}: {np.median([s[k][0] for s in steps if k in s]):.2f} us in {int(np.median([s[k][1] for s in steps if k in s]))} timed scopes" for k in timers)
        total = float(np.median([sum(v[0] for v in s.values()) for s in steps]))
        say(f"{label:44s}: device {total:9.2f} us per step ({per}); wall median {np.median(wall[label]):.4f} ms, spread between blocks {max(wall[label]) - min(wall[label]):.4f} ms")
    return {label: float(np.median([sum(v[0] for v in s.values()) for s in dev[label]])) for label, _c, _cs in routes}


def row(title, k, canvas, both_lanes):
    W, H = canvas
    ow, oh = (SH, SW) if k & 1 else (SW, SH)
    fw, fh = (H, W) if k & 1 else (W, H)  # the floor's canvas: the stored frame's way round
    dst = {name: torch.zeros((N, H, W, 4), dtype=torch.uint8, device="cuda") for name in ("x", "turn", "two")}
    floor_dst = torch.zeros((N, fh, fw, 4), dtype=torch.uint8, device="cuda")
    upright = torch.zeros((N, oh, ow, 4), dtype=torch.uint8, device="cuda")  # the RGBA frames of O the two-pass route draws from
    rgba = [dict(format="rgba", width=ow, height=oh, p0=upright.data_ptr() + j * ow * oh * 4) for j in range(N)]
    entries = oriented(k)
    c1, c2, cf, cu = ctx(W, H, 1), ctx(W, H, 2), ctx(fw, fh), ctx(ow, oh, 2 if k & 1 else 1)

    def two_pass():
        cu.draw_list(entries, dst=upright.data_ptr())
        c1.draw_list(rgba, dst=dst["two"].data_ptr())

    routes = [("(a) ONE oriented draw list, lanes along O's x", lambda: c1.draw_list(entries, dst=dst["x"].data_ptr()), [c1])]
    if both_lanes:
        routes.append(("(a) ONE oriented draw list, tile turned in LDS", lambda: c2.draw_list(entries, dst=dst["turn"].data_ptr()), [c2]))
    routes.append((f"(b) bits cleared onto {fw}x{fh}: the floor", lambda: cf.draw_list(feeds, dst=floor_dst.data_ptr()), [cf]))
    routes.append(("(c) two passes: orient 1 : 1, then draw", two_pass, [cu, c1]))
    res = measure(title, routes)
    torch.cuda.synchronize()
    say(f"same bytes: lanes-x against the two-pass route {bool(torch.equal(dst['x'], dst['two']))}" + (f", against the turned tile {bool(torch.equal(dst['x'], dst['turn']))}" if both_lanes else ""))
    a = min(v for label, v in res.items() if label.startswith("(a)"))
    c = [v for label, v in res.items() if label.startswith("(c)")][0]
    say(f"(a) / (c) device time: {a / c:.3f}")
    del dst, floor_dst
    return res


row("rot 1 -> 240x320", 1, (240, 320), True)
row("rot 2 -> 320x240", 2, (320, 240), False)
row("flip -> 320x240", 4, (320, 240), False)
# 1 : 1: the orient pass itself, in both lane mappings, against the unoriented 1 : 1 conversion of the same frames
big = torch.zeros((N, SW, SH, 4), dtype=torch.uint8, device="cuda")
bigf = torch.zeros((N, SH, SW, 4), dtype=torch.uint8, device="cuda")
b1, b2, bf = ctx(SH, SW, 1), ctx(SH, SW, 2), ctx(SW, SH)
e1 = oriented(1)
measure("1 : 1, rot 1 -> 1080x1920", [("(a) oriented 1 : 1, lanes along O's x", lambda: b1.draw_list(e1, dst=big.data_ptr()), [b1]),
                                       ("(a) oriented 1 : 1, tile turned in LDS", lambda: b2.draw_list(e1, dst=big.data_ptr()), [b2]),
                                       ("(b) bits cleared onto 1920x1080: the floor", lambda: bf.draw_list(feeds, dst=bigf.data_ptr()), [bf])])
for c in contexts.values():
    c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
