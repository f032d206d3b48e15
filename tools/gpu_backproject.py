#!/usr/bin/env python3
"""tools/gpu_backproject.py [calls] — device time of the three launches of ht_camshift_backproject_device (timers cs_bp_hist, cs_bp_lut,
cs_backproject: HIP events on the context's stream, ht_profile / ht_kernel_times) for 8 x 1920x1080, 256 x 320x240 and 1 x 320x240, both
output kinds, and in the SAME process k_gray_linear (timer `gray` of a detect step) on the same frames as the yardstick: the same shape
of kernel (16-byte loads, 16-byte stores, 5 B/px) with a known share of the HBM rate.  Median over `calls` (default 60)
single calls after a warm-up, each read back on its own.  Bytes: histogram pass 4 B/px read; back-project kernel 4 B/px read + 4 (RGBA8) or
8 (F64) B/px written; gray 4 B/px read + 1 B/px written.  The committed output is profiles/backproject.txt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 60
WARM = 10
SHAPES = [("8 x 1920x1080", 1920, 1080, 8), ("256 x 320x240", 320, 240, 256), ("1 x 320x240", 320, 240, 1)]


def frames_of(w, h, n):
    if (w, h) == (1920, 1080):
        return synth.stream_feed_frames(n, w, h, 0)  # the C5 feeds of bench.py
    return synth.mixed_batch(n, w, h, seed0=1234)    # the C2 / C3 batch of bench.py


def medians(c, call, names):
    """median device us of every timer in `names` over CALLS single calls"""
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
    return f"{us:9.2f} us  {nbytes / us / 1e6:7.3f} TB/s" if us > 0 else "not measured"


print(f"# median of {CALLS} calls after {WARM} warm-up calls, one process; device time from HIP events around each launch")
for name, w, h, n in SHAPES:
    px = n * w * h
    host = frames_of(w, h, n)
    dev = torch.from_numpy(host).cuda()
    out = torch.empty(px * 8, dtype=torch.uint8, device="cuda")
    c = Context(options="graph_max_frames=0")  # plain launches, so that the detect step's `gray` timer brackets k_gray_linear itself
    c.set_geometry(w, h, n)
    c.camshift_reserve(n)
    c.bind_device(dev.data_ptr(), n)
    c.camshift_init([(w // 4, h // 4, w // 2, h // 2)] * n)

    def gray():
        c.detect_enqueue(0)
        c.detect_collect_best(1)

    g = medians(c, gray, ["gray"])["gray"]
    print(f"{name}: k_gray_linear (4 + 1 B/px)                 {rate(5 * px, g)}")
    for kind, wb in (("rgba8", 4), ("f64", 8)):
        t = medians(c, lambda: c.camshift_backproject_device(out.data_ptr(), n, kind=kind), ["cs_bp_hist", "cs_bp_lut", "cs_backproject"])
        print(f"{name}: {kind:5s} cs_bp_hist     (4 B/px)            {rate(4 * px, t['cs_bp_hist'])}")
        print(f"{name}: {kind:5s} cs_bp_lut                          {t['cs_bp_lut']:9.2f} us")
        print(f"{name}: {kind:5s} cs_backproject (4 + {wb} B/px)        {rate((4 + wb) * px, t['cs_backproject'])}"
              f"   = {(4 + wb) * px / t['cs_backproject'] / (5 * px / g):.2f} x k_gray_linear's bytes/s")
    c.close()
    del dev, out
