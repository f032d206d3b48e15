#!/usr/bin/env python3
"""tools/gpu_align.py [out] — the workload of tools/gpu_crop.py (8 trackers on 8 resident 1080p NV12 feeds, each in an allocation of its
own, drawn onto a 320x240 canvas and tracked there, 112x112 patches): ONE ht_camshift_align_sources_device against ONE
ht_camshift_crop_sources_device on the same entries.  The crop call is the existing kernel and the yardstick: k_crop_list reads rows of an
axis-aligned rect, k_align_list gathers along tilted lines.  Sets no pass mark; writes what it measured to `out` (default: stdout only).
The committed output is profiles/align.txt.  Reads nothing outside the tree.

Twice: with the trackers stepped at calc_angles = 0 (every angle exactly pi / 2: the aligned patch is an axis-aligned block, the gather runs
along rows) and at calc_angles = 1 (the angles the blobs have).  The two calls alternate in blocks in one process.  Reported: device time
per kernel (HIP events around each launch: ht_profile / ht_kernel_times) and the wall clock of call + synchronize: per-block medians, the
median over blocks and the spread between blocks; then the same for a list of ONE entry, the most tilted tracker's.  The run first asserts
that every tracker has a face and that the most tilted entry's aligned patch is the Python restatement's, byte for byte."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import align_cases as al  # noqa: E402  (the rule, restated in Python)
import yuv_cases as yc  # noqa: E402  (the forward packer and the declared conversion)
from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
WARM, BLOCKS, PER_BLOCK = 20, 6, 40
CW, CH, SW, SH, P, Q, K = 320, 240, 1920, 1080, 112, 112, 8
MARGIN_Q8, FLAGS = 384, al.SQUARE
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


TURN = [0, 5, 10, 20, 30, 45, 60, 80]  # degrees: feed k's picture is turned by TURN[k] about its face's centre, so that the tracked blobs tilt
STRETCH = 1.6  # ... and stretched along its turned vertical, so that the (round) face becomes a blob with a long axis to find


def turned(rgb, cx, cy, degrees):
    """the picture stretched by STRETCH along y and then turned about (cx, cy): nearest neighbour, edges repeated"""
    t = np.deg2rad(degrees)
    y, x = np.mgrid[0:rgb.shape[0], 0:rgb.shape[1]].astype(np.float32)
    u, v = (x - cx) * np.cos(t) + (y - cy) * np.sin(t), -(x - cx) * np.sin(t) + (y - cy) * np.cos(t)  # the pixel in the turned frame
    sx = np.rint(cx + u).astype(np.int64).clip(0, rgb.shape[1] - 1)
    sy = np.rint(cy + v / STRETCH).astype(np.int64).clip(0, rgb.shape[0] - 1)
    return np.ascontiguousarray(rgb[sy, sx])


say(f"# tools/gpu_align.py: pictures stretched {STRETCH} x along y and turned by {TURN} degrees; {K} trackers on {K} resident {SW}x{SH} NV12 feeds (canvas {CW}x{CH}) -> {P}x{Q}, margin {MARGIN_Q8}/256, square; "
    f"GPU: {torch.cuda.get_device_name(0)}")
entries, keep, rects, planes_of = [], [], [], []
for k in range(K):
    rgb = turned(synth.stream_feed_frames(1, SW, SH, k)[0], 700 + 40 * k + 180, 300 + 180, TURN[k])
    planes = yc.from_rgb(rgb, yc.NV12, 1)
    planes_of.append(planes)
    t = torch.from_numpy(yc.pack(planes)).cuda()
    entries.append(dict(format="nv12", width=SW, height=SH, matrix="bt709", p0=t.data_ptr(), p1=t.data_ptr() + SW * SH, rect=None))
    keep.append(t)
    rects.append(((700 + 40 * k) * CW // SW, 300 * CH // SH, 360 * CW // SW, 360 * CH // SH))  # the face of synth.stream_feed_frames on the canvas
out_align = torch.zeros((K, Q, P, 4), dtype=torch.uint8, device="cuda")
out_crop = torch.zeros_like(out_align)
c = Context(options="graph_max_frames=0")
c.set_geometry(CW, CH, K)
c.draw_list(entries)  # bound: frame k = feed k's canvas
c.camshift_reserve(K)
pairs = [(k, k) for k in range(K)]
c.camshift_init_pairs(pairs, rects)


def measure(calls):
    """calls: {name: callable}; alternated in blocks -> ({name: [block medians of the wall ms]}, {name: [per call {timer: (us, launches)}]})"""
    wall, dev = {k: [] for k in calls}, {k: [] for k in calls}
    order = list(calls.items())
    for b in range(BLOCKS):
        for name, call in order if b % 2 == 0 else order[::-1]:
            ts = []
            for _ in range(PER_BLOCK):
                c.kernel_times(reset=True)
                t0 = time.perf_counter()
                call()
                c.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                kt = c.kernel_times(reset=True)
                dev[name].append({k: (v["ms"] * 1e3, v["launches"]) for k, v in kt.items() if v["launches"]})
            wall[name].append(float(np.median(ts)))
    return wall, dev


def report(title, wall, dev):
    say(f"## {title}: blocks of {PER_BLOCK} calls, {BLOCKS} blocks per call, alternated; profiling on (its events are inside the wall clock of both)")
    for name in wall:
        timers = sorted({k for s in dev[name] for k in s})
        per = ", ".join(f"{k}: {np.median([s[k][0] for s in dev[name] if k in s]):.2f} us" for k in timers)
        m = float(np.median(wall[name]))
        say(f"{name}: device {per}; wall ms per call + sync, median of each block {[round(v, 4) for v in wall[name]]}; median {m:.4f} ms, "
            f"spread between blocks {max(wall[name]) - min(wall[name]):.4f} ms")
    ma, mc = (float(np.median(wall[k])) for k in wall)
    spread = max(max(wall[k]) - min(wall[k]) for k in wall)
    say(f"align / crop: {ma / mc:.3f} x the wall time per call; difference {ma - mc:+.4f} ms against a largest spread between blocks of {spread:.4f} ms")


for calc_angles in (False, True):
    objs = c.camshift_track_pairs(pairs, calc_angles=calc_angles)
    assert all(float(o["width"]) > 0 and float(o["height"]) > 0 for o in objs), "every tracker follows a face"
    a12 = [al.a12_of(float(o["angle"])) for o in objs]
    tilt = [min((a - 1024) % 4096, (1024 - a) % 4096) for a in a12]  # steps away from upright
    say()
    say(f"# trackers stepped with calc_angles = {int(calc_angles)}: a12 {a12} (1024 is upright; 4096 steps per turn), boxes {[(int(o['width']), int(o['height'])) for o in objs]}")

    def align_list(n=K, first=0):
        c.camshift_align_sources_device(out_align.data_ptr(), list(range(first, first + n)), entries[first:first + n], P, Q, margin=MARGIN_Q8 / 256, square=bool(FLAGS))

    def crop_list(n=K, first=0):
        c.camshift_crop_sources_device(out_crop.data_ptr(), list(range(first, first + n)), entries[first:first + n], P, Q, margin=MARGIN_Q8 / 256, square=bool(FLAGS))

    align_list()
    crop_list()
    rec = c.camshift_align_result(K)
    c.synchronize()
    assert all(int(r["code"]) == al.FACE for r in rec) and [int(r["a12"]) for r in rec] == a12
    k = int(np.argmax(tilt))  # the most tilted tracker: its patch is checked and timed alone below
    view = yc.to_rgba(planes_of[k], SW, SH, yc.NV12, 1)
    want = al.sample(view, al.plan(tuple(float(objs[k][f]) for f in ("x", "y", "width", "height", "angle")), CW, CH, SW, SH, None, MARGIN_Q8, FLAGS), P, Q)
    same = bool((out_align[k].cpu().numpy() == want).all())
    say(f"entry {k}'s aligned patch equals the restatement's: {same}; the patch's vectors in source pixels (ux, uy), (vx, vy): "
        f"{[(round(int(r['ux']) / 65536, 1), round(int(r['uy']) / 65536, 1), round(int(r['vx']) / 65536, 1), round(int(r['vy']) / 65536, 1)) for r in rec]}")
    assert same
    for call in (align_list, crop_list):
        for _ in range(WARM):
            call()
    c.synchronize()
    c.profile(True)
    wall, dev = measure({"ONE ht_camshift_align_sources_device": align_list, "ONE ht_camshift_crop_sources_device ": crop_list})
    report(f"{K} entries", wall, dev)
    wall, dev = measure({"ONE ht_camshift_align_sources_device": lambda: align_list(1, k), "ONE ht_camshift_crop_sources_device ": lambda: crop_list(1, k)})
    report(f"1 entry, tracker {k} ({tilt[k]} steps = {tilt[k] * 360 / 4096:.1f} degrees from upright)", wall, dev)
    c.profile(False)
c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
