#!/usr/bin/env python3
"""tools/gpu_ingest.py [calls] — device time of k_draw_frames (ht_draw_frames_device; timer `draw_frames`: HIP events on the context's
stream, ht_profile / ht_kernel_times) for the shapes the scaled ingest exists for, and in the SAME process k_gray_linear (timer `gray` of a
detect step) on the same DESTINATION frames as the yardstick.  Median over `calls` (default 60) single calls after a warm-up.

Bytes of a draw = source rows actually touched x 4 sw bytes (every row that some destination row's taps a / b name, whole rect width: at
these ratios every 64-byte line of a touched row is touched) + 4 W H destination bytes written, per frame.  Bytes of gray = 4 + 1 B/px.

Second part: what the scaling step buys a large-feed user — wall time (host clock around calls that end in a wait) of a C5-style detect
step and track step on 8 x 1920x1080 originals, next to draw + the same step on the drawn 8 x 320x240 frames, same process.  The committed
output is profiles/ingest.txt."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 60
WARM = 10
SHAPES = [("8 x 1920x1080 -> 320x240", 1920, 1080, 320, 240, 8), ("256 x 1920x1080 -> 320x240", 1920, 1080, 320, 240, 256),
          ("128 x 1280x720 -> 320x240", 1280, 720, 320, 240, 128), ("8 x 1920x1080 -> 1920x1080 (copy)", 1920, 1080, 1920, 1080, 8),
          ("256 x 160x120 -> 320x240 (upscale)", 160, 120, 320, 240, 256)]


def rows_touched(sh, dh):
    """source rows named by the row taps of the declared resampler (oracle/canvas_shim.js), binary64 like the kernel"""
    j = np.arange(dh, dtype=np.float64)
    f = np.clip((j + 0.5) * (sh / dh) - 0.5, 0.0, sh - 1.0)
    a = np.floor(f).astype(np.int64)
    return len(set(a.tolist()) | set(np.minimum(a + 1, sh - 1).tolist()))


def medians(c, call, names):
    for _ in range(WARM):
        call()
    c.synchronize()
    c.profile(True)
    c.kernel_times(reset=True)
    rows = {k: [] for k in names}
    for _ in range(CALLS):
        call()
        c.synchronize()
        kt = c.kernel_times(reset=True)
        for k in names:
            rows[k].append(kt[k]["ms"] * 1e3)
    c.profile(False)
    return {k: float(np.median(v)) for k, v in rows.items()}


def rate(nbytes, us):
    return f"{us:9.2f} us  {nbytes / us / 1e6:7.3f} TB/s"


def source_frames(w, h, n):
    """n device frames from 8 distinct host frames (a 256 x 1080p batch is 2.1 GB)"""
    uniq = synth.stream_feed_frames(8, w, h, 0) if (w, h) == (1920, 1080) else np.stack(
        [synth.face_frame(w, h, [(w // 4 + 3 * k, h // 5 + 2 * k, min(w, h) // 2)]) for k in range(8)])
    d = torch.from_numpy(uniq).cuda()
    return d.repeat((n + 7) // 8, 1, 1, 1)[:n].contiguous()


print(f"# median of {CALLS} calls after {WARM} warm-up calls, one process; device time from HIP events around each launch")
for name, sw, sh, dw, dh, n in SHAPES:
    src = source_frames(sw, sh, n)
    dst = torch.empty((n, dh, dw, 4), dtype=torch.uint8, device="cuda")
    c = Context(options="graph_max_frames=0")  # plain launches, so that the detect step's `gray` timer brackets k_gray_linear itself
    c.set_geometry(dw, dh, n)
    t = medians(c, lambda: c.draw_frames_device(src.data_ptr(), n, sw, sh, dst=dst.data_ptr()), ["draw_frames"])["draw_frames"]
    c.bind_device(dst.data_ptr(), n)

    def gray():
        c.detect_enqueue(0)
        c.detect_collect_best(1)

    g = medians(c, gray, ["gray"])["gray"]
    nbytes = n * (rows_touched(sh, dh) * sw * 4 + dw * dh * 4)
    print(f"{name}: k_draw_frames ({rows_touched(sh, dh)} of {sh} source rows + 4 B/px written)  {rate(nbytes, t)}")
    print(f"{name}: k_gray_linear on the {n} destination frames (4 + 1 B/px)  {rate(5 * n * dw * dh, g)}"
          f"   draw = {nbytes / t / (5 * n * dw * dh / g):.2f} x its bytes/s, {t / g:.2f} x its time")
    c.close()
    del src, dst


# ---- the scaling step in a C5-style loop: 8 feeds of 1920x1080 ---------------------------------------------------------------------------
def wall(call, sync):
    for _ in range(WARM):
        call()
    sync()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


K, SW, SH, W, H = 8, 1920, 1080, 320, 240
src = source_frames(SW, SH, K)
big = Context()
big.set_geometry(SW, SH, K)
big.camshift_reserve(K)
big.bind_device(src.data_ptr(), K)
small = Context()
small.set_geometry(W, H, K)
small.camshift_reserve(K)


def detect_step(c):
    c.detect_enqueue(0)
    return c.detect_collect_best(1)[0]


def rects_of(best, w, h):
    fl = np.floor(np.stack([best["x"], best["y"], best["width"], best["height"]], axis=1)).astype(np.int64)
    return [tuple(int(v) for v in fl[f]) if best["neighbors"][f] > 0 and best["confidence"][f] > -10 else (w // 4, h // 4, w // 2, h // 2) for f in range(len(best))]


print(f"# C5-style steps, {K} feeds, wall ms per step (median of {CALLS}; every step ends in a wait for its results)")
d_big = wall(lambda: detect_step(big), big.synchronize)
big.camshift_init(rects_of(detect_step(big), SW, SH))
t_big = wall(lambda: big.camshift_track(K, calc_angles=True), big.synchronize)


def draw():
    small.draw_frames_device(src.data_ptr(), K, SW, SH)


def draw_wait():
    draw()
    small.synchronize()


dr = wall(draw_wait, small.synchronize)
d_small = wall(lambda: (draw(), detect_step(small)), small.synchronize)
draw()
small.camshift_init(rects_of(detect_step(small), W, H))
t_small = wall(lambda: (draw(), small.camshift_track(K, calc_angles=True)), small.synchronize)
print(f"detect step on the 1080p originals            {d_big:8.3f} ms")
print(f"draw -> 320x240 + detect step on the result   {d_small:8.3f} ms   (draw alone, waited for: {dr:.3f} ms = {100 * dr / d_small:.0f} % of the step)")
print(f"track step on the 1080p originals             {t_big:8.3f} ms")
print(f"draw -> 320x240 + track step on the result    {t_small:8.3f} ms   (draw alone: {100 * dr / t_small:.0f} % of the step)")
big.close()
small.close()
