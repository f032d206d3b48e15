#!/usr/bin/env python3
"""tools/gpu_crop.py [out] — 8 trackers on 8 resident 1080p NV12 feeds (each in an allocation of its own, drawn onto a 320x240 canvas and
tracked there), every tracker's face cut from ITS FEED'S OWN frame into a 112x112 patch: once through ONE ht_camshift_crop_sources_device
behind an enqueue-only track step, and once by today's route — collect the track objects (which synchronises), run the rule on the host,
ht_draw_list_device with those rects on a second context whose geometry is 112x112.  Sets no pass mark; writes what it measured to `out`
(default: stdout only).  The committed output is profiles/crop.txt.  Reads nothing outside the tree.

The two routes alternate in blocks in one process.  Reported: device time per kernel (HIP events around each launch: ht_profile /
ht_kernel_times) and the wall clock of a step — track step + crops + the synchronisation(s) the route needs —, and of the crop part alone
on objects that are already known: per-block medians, the median over blocks and the spread between the blocks of one route.  The run
first asserts that both routes give identical bytes and that every tracker has a face."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import crop_cases as cr  # noqa: E402  (the rule, restated in Python: the host route's)
import yuv_cases as yc  # noqa: E402  (the forward packer)
from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
WARM, BLOCKS, PER_BLOCK = 20, 6, 40
CW, CH, SW, SH, P, Q, K = 320, 240, 1920, 1080, 112, 112, 8
MARGIN_Q8, FLAGS = 384, cr.SQUARE
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/gpu_crop.py: {K} trackers on {K} resident {SW}x{SH} NV12 feeds (canvas {CW}x{CH}) -> {P}x{Q}, margin {MARGIN_Q8}/256, square; GPU: {torch.cuda.get_device_name(0)}")
entries, keep, rects = [], [], []
for k in range(K):
    rgb = synth.stream_feed_frames(1, SW, SH, k)[0]
    t = torch.from_numpy(yc.pack(yc.from_rgb(rgb, yc.NV12, 1))).cuda()
    entries.append(dict(format="nv12", width=SW, height=SH, matrix="bt709", p0=t.data_ptr(), p1=t.data_ptr() + SW * SH, rect=None))
    keep.append(t)
    rects.append(((700 + 40 * k) * CW // SW, 300 * CH // SH, 360 * CW // SW, 360 * CH // SH))  # the face of synth.stream_feed_frames on the canvas
pb = P * Q * 4
out_dev = torch.zeros((K, Q, P, 4), dtype=torch.uint8, device="cuda")
out_host = torch.zeros_like(out_dev)
c = Context(options="graph_max_frames=0")
c.set_geometry(CW, CH, K)
c.draw_list(entries)  # bound: frame k = feed k's canvas
c.camshift_reserve(K)
pairs = [(k, k) for k in range(K)]
streams = list(range(K))
c.camshift_init_pairs(pairs, rects)
c2 = Context(options="graph_max_frames=0")  # today's route: a second context whose geometry is the patch size
c2.set_geometry(P, Q, K)


def crop_device():
    c.camshift_crop_sources_device(out_dev.data_ptr(), streams, entries, P, Q, margin=MARGIN_Q8 / 256, square=bool(FLAGS))


def crop_host(objs):
    cut = []
    for e, o in zip(entries, objs):
        code, rect = cr.rule((float(o["x"]), float(o["y"]), float(o["width"]), float(o["height"])), CW, CH, SW, SH, None, MARGIN_Q8, FLAGS)
        assert code == cr.FACE
        cut.append(dict(e, rect=rect))
    c2.draw_list(cut, dst=out_host.data_ptr())


def step_device():
    c.camshift_track_pairs(pairs, fetch=False)
    crop_device()
    c.synchronize()
    c.camshift_track_collect(K)  # complete by now: takes the step out of the ring


def step_host():
    objs = c.camshift_track_pairs(pairs)  # collects: the host needs the objects
    crop_host(objs)
    c2.synchronize()


objs = c.camshift_track_pairs(pairs)
assert all(float(o["width"]) > 0 and float(o["height"]) > 0 for o in objs), "every tracker follows a face"
crop_device()
crop_host(objs)
c.synchronize()
c2.synchronize()
rec = c.camshift_crop_result(K)
same = bool(torch.equal(out_dev, out_host))
say(f"same bytes from both routes: {same}; rects (source pixels) {[(int(r['x']), int(r['y']), int(r['width']), int(r['height'])) for r in rec]}")
assert same and all(int(r["code"]) == cr.FACE for r in rec)
for call in (step_device, step_host):
    for _ in range(WARM):
        call()
c.profile(True)
c2.profile(True)


def measure(dev_call, host_call):
    wall, dev = {"device": [], "host": []}, {"device": [], "host": []}
    for b in range(BLOCKS):
        order = (("device", dev_call), ("host", host_call))
        for name, call in order if b % 2 == 0 else order[::-1]:
            ts, ds = [], []
            for _ in range(PER_BLOCK):
                c.kernel_times(reset=True)
                c2.kernel_times(reset=True)
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e3)
                kt = {**c.kernel_times(reset=True), **c2.kernel_times(reset=True)}
                ds.append({k: (v["ms"] * 1e3, v["launches"]) for k, v in kt.items() if v["launches"]})
            wall[name].append(float(np.median(ts)))
            dev[name].append(ds)
    return wall, dev


def report(title, wall, dev, names):
    say(f"## {title}: blocks of {PER_BLOCK} calls, {BLOCKS} blocks per route, alternated; profiling on (its events are inside the wall clock of both routes)")
    for name in ("device", "host"):
        steps = [s for blk in dev[name] for s in blk]
        timers = sorted({k for s in steps for k in s})
        per = ", ".join(f"{k}: {np.median([s[k][0] for s in steps if k in s]):.2f} us in {int(np.median([s[k][1] for s in steps if k in s]))} launches" for k in timers)
        total = float(np.median([sum(v[0] for v in s.values()) for s in steps]))
        m = float(np.median(wall[name]))
        say(f"{names[name]}: device {total:8.2f} us per call ({per}); wall ms per call, median of each block {[round(v, 4) for v in wall[name]]}; median {m:.4f} ms, "
            f"spread between blocks {max(wall[name]) - min(wall[name]):.4f} ms")
    md, mh = float(np.median(wall["device"])), float(np.median(wall["host"]))
    spread = max(max(wall[k]) - min(wall[k]) for k in wall)
    say(f"device / host route: {md / mh:.3f} x the wall time per call; difference {mh - md:+.4f} ms against a largest spread between blocks of {spread:.4f} ms")


wall, dev = measure(step_device, step_host)
report("a track step and its crops", wall, dev, {"device": "enqueue-only track + ONE ht_camshift_crop_sources_device + sync ",
                                                  "host": "track + collect, rule on the host, ht_draw_list_device on ctx 2 + sync"})
objs = c.camshift_track_pairs(pairs)


def only_device():
    crop_device()
    c.synchronize()


def only_host():
    crop_host(objs)
    c2.synchronize()


wall, dev = measure(only_device, only_host)
report("the crops alone, objects already known to the host", wall, dev, {"device": "ONE ht_camshift_crop_sources_device + sync            ",
                                                                         "host": "rule on the host, ht_draw_list_device on ctx 2 + sync"})
c.close()
c2.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
