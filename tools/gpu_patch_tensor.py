#!/usr/bin/env python3
"""tools/gpu_patch_tensor.py [out] — the workload of tools/gpu_align.py (8 trackers on 8 resident 1080p NV12 feeds, each in an allocation of
its own, drawn onto a 320x240 canvas and tracked there with the angles the blobs have, 112x112 patches): ONE tensor call (f16 CHW RGB,
ImageNet mean / std) against the route a user had before it — the RGBA call followed by torch's elementwise chain
    x[..., :3].permute(0, 3, 1, 2).float().mul(scale).add(bias).half()
on the SAME stream (the Context is created on a torch stream and the chain runs under it) — for the crop calls and for the align calls.
Sets no pass mark; writes what it measured to `out` (default: stdout only).  The committed output is profiles/patch_tensor.txt.  Reads
nothing outside the tree.

The routes alternate in blocks in one process.  Reported per route: device time per library kernel (HIP events around each launch:
ht_profile / ht_kernel_times), the stream span of the whole route (torch events on the stream in front of and behind it, which for the
chain includes the gaps between its launches) and the wall clock of route + synchronize: per-block medians, the median over blocks and the
spread between blocks.  Before timing, the run compares the two routes' results: f32 must be equal (torch's mul and add are two binary32
roundings, as the rule's); for f16 it prints the number of elements that differ, if any."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv_cases as yc  # noqa: E402  (the forward packer)
from headtrackr_amd import native, synth, torch_patches  # noqa: E402
from headtrackr_amd.api import Context, PatchFormat  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
WARM, BLOCKS, PER_BLOCK = 20, 6, 40
CW, CH, SW, SH, P, Q, K = 320, 240, 1920, 1080, 112, 112, 8
MARGIN, SQUARE = 1.5, True
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TURN, STRETCH = [0, 5, 10, 20, 30, 45, 60, 80], 1.6  # tools/gpu_align.py's pictures
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def turned(rgb, cx, cy, degrees):
    t = np.deg2rad(degrees)
    y, x = np.mgrid[0:rgb.shape[0], 0:rgb.shape[1]].astype(np.float32)
    u, v = (x - cx) * np.cos(t) + (y - cy) * np.sin(t), -(x - cx) * np.sin(t) + (y - cy) * np.cos(t)
    sx = np.rint(cx + u).astype(np.int64).clip(0, rgb.shape[1] - 1)
    sy = np.rint(cy + v / STRETCH).astype(np.int64).clip(0, rgb.shape[0] - 1)
    return np.ascontiguousarray(rgb[sy, sx])


say(f"# tools/gpu_patch_tensor.py: {K} trackers on {K} resident {SW}x{SH} NV12 feeds (canvas {CW}x{CH}, pictures turned by {TURN} degrees) -> {P}x{Q}, margin {MARGIN}, square; "
    f"f16 CHW RGB, ImageNet mean / std; GPU: {torch.cuda.get_device_name(0)}; library: {os.path.relpath(native.LIB_PATH, ROOT)}")
stream = torch.cuda.Stream()
entries, keep, rects = [], [], []
for k in range(K):
    rgb = turned(synth.stream_feed_frames(1, SW, SH, k)[0], 700 + 40 * k + 180, 300 + 180, TURN[k])
    t = torch.from_numpy(yc.pack(yc.from_rgb(rgb, yc.NV12, 1))).cuda()
    entries.append(dict(format="nv12", width=SW, height=SH, matrix="bt709", p0=t.data_ptr(), p1=t.data_ptr() + SW * SH, rect=None))
    keep.append(t)
    rects.append(((700 + 40 * k) * CW // SW, 300 * CH // SH, 360 * CW // SW, 360 * CH // SH))
fmt16 = PatchFormat.mean_std(MEAN, STD, dtype="f16", layout="chw", channels="rgb")
fmt32 = PatchFormat.mean_std(MEAN, STD, dtype="f32", layout="chw", channels="rgb")
scale = torch.tensor(fmt16.scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
bias = torch.tensor(fmt16.bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
rgba = torch.zeros((K, Q, P, 4), dtype=torch.uint8, device="cuda")
x16 = torch_patches.empty_patches(K, P, Q, fmt16, "cuda")
x32 = torch_patches.empty_patches(K, P, Q, fmt32, "cuda")
torch.cuda.synchronize()
c = Context(stream=stream.cuda_stream, options="graph_max_frames=0")
c.set_geometry(CW, CH, K)
c.draw_list(entries)
c.camshift_reserve(K)
pairs = [(k, k) for k in range(K)]
streams = list(range(K))
c.camshift_init_pairs(pairs, rects)
objs = c.camshift_track_pairs(pairs)
assert all(float(o["width"]) > 0 and float(o["height"]) > 0 for o in objs), "every tracker follows a face"


def chain32():
    with torch.cuda.stream(stream):
        return rgba[..., :3].permute(0, 3, 1, 2).float().mul(scale).add(bias)


def chain16():
    with torch.cuda.stream(stream):
        return rgba[..., :3].permute(0, 3, 1, 2).float().mul(scale).add(bias).half()


ROUTES = {
    "crop": (lambda f, x: torch_patches.crop_sources_into(c, x, streams, entries, f, margin=MARGIN, square=SQUARE),
             lambda: c.camshift_crop_sources_device(rgba.data_ptr(), streams, entries, P, Q, margin=MARGIN, square=SQUARE), "cut_tensor", "crop_list"),
    "align": (lambda f, x: torch_patches.align_sources_into(c, x, streams, entries, f, margin=MARGIN, square=SQUARE),
              lambda: c.camshift_align_sources_device(rgba.data_ptr(), streams, entries, P, Q, margin=MARGIN, square=SQUARE), "upright_tensor", "align_list"),
}


def measure(calls):
    wall, span, dev = {k: [] for k in calls}, {k: [] for k in calls}, {k: [] for k in calls}
    order = list(calls.items())
    for b in range(BLOCKS):
        for name, call in order if b % 2 == 0 else order[::-1]:
            ts, sp = [], []
            for _ in range(PER_BLOCK):
                c.kernel_times(reset=True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                call()
                e1.record(stream)
                c.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                sp.append(e0.elapsed_time(e1) * 1e3)
                kt = c.kernel_times(reset=True)
                dev[name].append({k: v["ms"] * 1e3 for k, v in kt.items() if v["launches"]})
            wall[name].append(float(np.median(ts)))
            span[name].append(float(np.median(sp)))
    return wall, span, dev


for kind, (tensor_call, rgba_call, t_tensor, t_rgba) in ROUTES.items():
    say()
    say(f"# {kind}")
    tensor_call(fmt32, x32)
    tensor_call(fmt16, x16)
    rgba_call()
    want32, want16 = chain32(), chain16()
    c.synchronize()
    eq32 = bool(torch.equal(want32.contiguous().view(torch.int32), x32.view(torch.int32)))
    diff16 = int((want16.contiguous().view(torch.int16) != x16.view(torch.int16)).sum())
    say(f"the torch chain's result against the tensor call's: f32 equal: {eq32}; f16: {diff16} of {x16.numel()} elements differ")
    assert eq32

    def fused():
        tensor_call(fmt16, x16)

    def unfused():
        rgba_call()
        chain16()

    for call in (fused, unfused):
        for _ in range(WARM):
            call()
    c.synchronize()
    c.profile(True)
    wall, span, dev = measure({"ONE tensor call            ": fused, "RGBA call + the torch chain": unfused})
    c.profile(False)
    say(f"## {K} entries: blocks of {PER_BLOCK} calls, {BLOCKS} blocks per route, alternated; profiling on (its events are inside the wall clock and the span of both)")
    for name in wall:
        timers = sorted({k for s in dev[name] for k in s})
        per = ", ".join(f"{k}: {np.median([s[k] for s in dev[name] if k in s]):.2f} us" for k in timers)
        say(f"{name}: device {per}; stream span {float(np.median(span[name])):.1f} us; wall ms per route + sync, median of each block {[round(v, 4) for v in wall[name]]}; "
            f"median {float(np.median(wall[name])):.4f} ms, spread between blocks {max(wall[name]) - min(wall[name]):.4f} ms")
    (na, wa), (nb, wb) = wall.items()
    ma, mb = float(np.median(wa)), float(np.median(wb))
    spread = max(max(v) - min(v) for v in wall.values())
    say(f"tensor call / (RGBA call + chain): {ma / mb:.3f} x the wall time; difference {ma - mb:+.4f} ms against a largest spread between blocks of {spread:.4f} ms; "
        f"stream span {float(np.median(span[na])):.1f} us against {float(np.median(span[nb])):.1f} us")
c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
