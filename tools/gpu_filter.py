#!/usr/bin/env python3
"""tools/gpu_filter.py [out] — the workload of tools/gpu_crop.py (8 trackers on 8 resident 1080p NV12 feeds, each in an allocation of its
own, drawn onto a 320x240 canvas and tracked there, 112x112 patches, margin 384/256, square) through the prefiltered calls, max_factor 8:
ONE filtered call against ONE unfiltered call of the same list (the yardstick kernel: k_crop_list / k_align_list, whose times
profiles/crop.txt and profiles/align.txt record) and against the two-launch route a user had before — the unfiltered call at N * 112 into
a scratch buffer plus torch's block mean (and, for the tensor, torch's elementwise chain) on the SAME stream —, which exists only where the
factors are uniform and N * 112 <= 1024.  For the crop calls and the align calls, RGBA8 and f16 CHW RGB (ImageNet mean / std).  Sets no
pass mark; writes what it measured to `out` (default: stdout only).  The committed output is profiles/filter.txt.  Reads nothing outside
the tree.

The routes alternate in blocks in one process.  Reported per route: device time per library kernel (HIP events around each launch:
ht_profile / ht_kernel_times), the stream span of the whole route (torch events on the stream in front of and behind it) and the wall clock
of route + synchronize: per-block medians, the median over blocks and the spread between blocks.  Before timing, the run prints the factors
the library's own functions give for the call's records and asserts that the two-launch route's RGBA bytes equal the filtered call's."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import yuv_cases as yc  # noqa: E402  (the forward packer)
from headtrackr_amd import api, native, synth, torch_patches  # noqa: E402
from headtrackr_amd.api import Context, PatchFormat  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
WARM, BLOCKS, PER_BLOCK = 20, 6, 40
CW, CH, SW, SH, P, Q, K = 320, 240, 1920, 1080, 112, 112, 8
MARGIN, SQUARE, MAX_FACTOR = 384 / 256, True, 8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/gpu_filter.py: {K} trackers on {K} resident {SW}x{SH} NV12 feeds (canvas {CW}x{CH}) -> {P}x{Q}, margin 384/256, square, max_factor {MAX_FACTOR}; "
    f"GPU: {torch.cuda.get_device_name(0)}; library: {os.path.relpath(native.LIB_PATH, ROOT)}")
stream = torch.cuda.Stream()
entries, keep, rects = [], [], []
for k in range(K):
    rgb = synth.stream_feed_frames(1, SW, SH, k)[0]
    t = torch.from_numpy(yc.pack(yc.from_rgb(rgb, yc.NV12, 1))).cuda()
    entries.append(dict(format="nv12", width=SW, height=SH, matrix="bt709", p0=t.data_ptr(), p1=t.data_ptr() + SW * SH, rect=None))
    keep.append(t)
    rects.append(((700 + 40 * k) * CW // SW, 300 * CH // SH, 360 * CW // SW, 360 * CH // SH))  # the face of synth.stream_feed_frames on the canvas
fmt16 = PatchFormat.mean_std(MEAN, STD, dtype="f16", layout="chw", channels="rgb")
scale = torch.tensor(fmt16.scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
bias = torch.tensor(fmt16.bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
rgba = torch.zeros((K, Q, P, 4), dtype=torch.uint8, device="cuda")
rgba_plain = torch.zeros_like(rgba)
x16 = torch_patches.empty_patches(K, P, Q, fmt16, "cuda")
x16_plain = torch_patches.empty_patches(K, P, Q, fmt16, "cuda")
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

KINDS = {
    "crop": dict(filtered=c.camshift_crop_sources_filtered_device, plain=c.camshift_crop_sources_device, tensor=c.camshift_crop_sources_tensor_device,
                 result=c.camshift_crop_result, factors=api.crop_filter_factors),
    "align": dict(filtered=c.camshift_align_sources_filtered_device, plain=c.camshift_align_sources_device, tensor=c.camshift_align_sources_tensor_device,
                  result=c.camshift_align_result, factors=api.align_filter_factors),
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


def report(title, calls):
    for call in calls.values():
        for _ in range(WARM):
            call()
    c.synchronize()
    c.profile(True)
    wall, span, dev = measure(calls)
    c.profile(False)
    say(f"## {title}: blocks of {PER_BLOCK} calls, {BLOCKS} blocks per route, alternated; profiling on (its events are inside the wall clock and the span of every route)")
    for name in wall:
        timers = sorted({k for s in dev[name] for k in s})
        per = ", ".join(f"{k}: {np.median([s[k] for s in dev[name] if k in s]):.2f} us (min {min(s[k] for s in dev[name] if k in s):.2f}, max {max(s[k] for s in dev[name] if k in s):.2f})"
                        for k in timers)
        say(f"{name}: device {per}; stream span {float(np.median(span[name])):.1f} us; wall ms per route + sync, median of each block {[round(v, 4) for v in wall[name]]}; "
            f"median {float(np.median(wall[name])):.4f} ms, spread between blocks {max(wall[name]) - min(wall[name]):.4f} ms")
    names = list(wall)
    base = float(np.median(wall[names[1]]))
    spread = max(max(v) - min(v) for v in wall.values())
    for name in names[:1] + names[2:]:
        m = float(np.median(wall[name]))
        say(f"{name.strip()} / {names[1].strip()}: {m / base:.3f} x the wall time; difference {m - base:+.4f} ms against a largest spread between blocks of {spread:.4f} ms")


for kind, k in KINDS.items():
    say()
    say(f"# {kind}")
    k["filtered"](rgba.data_ptr(), streams, entries, P, Q, MAX_FACTOR, None, margin=MARGIN, square=SQUARE)
    rec = k["result"](K)
    factors = [tuple(int(v) for v in f) for f in k["factors"](rec, P, Q, MAX_FACTOR)]
    c.synchronize()
    say(f"factors (Nx, Ny) per entry: {factors}")
    if kind == "align":
        say(f"a12 per entry: {[int(r['a12']) for r in rec]}; vectors in source pixels (ux, uy), (vx, vy): "
            f"{[tuple(round(int(r[f]) / 65536, 1) for f in ('ux', 'uy', 'vx', 'vy')) for r in rec]}")
    else:
        say(f"rects (source pixels): {[(int(r['x']), int(r['y']), int(r['width']), int(r['height'])) for r in rec]}")
    uniform = len(set(factors)) == 1 and factors[0][0] * P <= 1024 and factors[0][1] * Q <= 1024
    nx, ny = factors[0]
    scratch = torch.zeros((K, ny * Q, nx * P, 4), dtype=torch.uint8, device="cuda") if uniform else None

    def mean_rgba():
        """the two-launch route: the unfiltered call at the fine size, torch's block mean on the same stream"""
        k["plain"](scratch.data_ptr(), streams, entries, nx * P, ny * Q, margin=MARGIN, square=SQUARE)
        with torch.cuda.stream(stream):
            n = nx * ny
            s = scratch.view(K, Q, ny, P, nx, 4).to(torch.int32).sum(dim=(2, 4))
            return ((s + (n >> 1)) // n).to(torch.uint8)

    def chain16(patches):
        with torch.cuda.stream(stream):
            return patches[..., :3].permute(0, 3, 1, 2).float().mul(scale).add(bias).half()

    routes_rgba = {
        "ONE filtered call                    ": lambda: k["filtered"](rgba.data_ptr(), streams, entries, P, Q, MAX_FACTOR, None, margin=MARGIN, square=SQUARE),
        "ONE unfiltered call (the yardstick)  ": lambda: k["plain"](rgba_plain.data_ptr(), streams, entries, P, Q, margin=MARGIN, square=SQUARE),
    }
    routes_f16 = {
        "ONE filtered call                    ": lambda: k["filtered"](x16.data_ptr(), streams, entries, P, Q, MAX_FACTOR, fmt16, margin=MARGIN, square=SQUARE),
        "ONE unfiltered tensor call           ": lambda: k["tensor"](x16_plain.data_ptr(), streams, entries, P, Q, fmt16, margin=MARGIN, square=SQUARE),
    }
    if uniform:
        two = mean_rgba()
        c.synchronize()
        torch.cuda.synchronize()
        same = bool(torch.equal(two, rgba))
        say(f"the two-launch route (unfiltered call at {nx * P}x{ny * Q} + torch's block mean) gives the filtered call's bytes: {same}")
        assert same
        k["filtered"](x16.data_ptr(), streams, entries, P, Q, MAX_FACTOR, fmt16, margin=MARGIN, square=SQUARE)
        want16 = chain16(two)
        c.synchronize()
        torch.cuda.synchronize()
        say(f"... and its f16 chain against the filtered tensor call: {int((want16.contiguous().view(torch.int16) != x16.view(torch.int16)).sum())} of {x16.numel()} elements differ")
        routes_rgba["unfiltered at N x + torch block mean "] = mean_rgba
        routes_f16["unfiltered at N x + mean + f16 chain "] = lambda: chain16(mean_rgba())
    else:
        say("the factors are not uniform (or N * 112 > 1024): there is no two-launch route to compare with")
    report(f"{kind}, RGBA8, {K} entries", routes_rgba)
    report(f"{kind}, f16 CHW RGB, {K} entries", routes_f16)
c.close()
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
