#!/usr/bin/env python3
"""tools/gpu_bp_pairs.py [output file] — M trackers on ONE frame: the pair call (ht_camshift_backproject_pairs_device: one histogram pass
per distinct frame, one pass over the pixels per group of 4 RGBA8 / 2 binary64 outputs) against the workaround the contiguous API offers
(the frame replicated M times in the bound set, one ht_camshift_backproject_device over M streams), in the same process and library, the
two forms taking turns.  Per case: device us per kernel (ht_profile / ht_kernel_times, HIP events) and the median wall us of a call that
ends in a synchronise.  Both forms write into device memory: no copy to the host in either.

    one frame of 1920x1080 and one of 320x240, M = 1, 2, 4, 8, both output kinds

Bytes per pixel: pair call 4 + 4 ceil(M / G) + out M, replicated M (8 + out) — out = 4 (RGBA8, G = 4) or 8 (binary64, G = 2).  What to read
off: whether the summed device time of the pair call stays at or below the replicated call's from M = 2 on (at M = 4 on 1080p above
all), and which kernel decides it."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

STEPS, WARM, NU, ROUNDS = 30, 8, 3, 3  # calls per timed window / warm-up calls / distinct frames the calls cycle through / windows per form
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bytes_per_pixel(M, kind):
    out, G = (8, 2) if kind == "f64" else (4, 4)
    return 4 + 4 * -(-M // G) + out * M, M * (8 + out)


def device_times(c, step):
    c.synchronize()
    c.profile(True)
    c.kernel_times(reset=True)
    for i in range(STEPS):
        step(i)
    kt = c.kernel_times(reset=True)
    c.profile(False)
    c.synchronize()
    return {k: round(v["ms"] / STEPS * 1e3, 2) for k, v in kt.items() if v["launches"] and v["ms"] > 0}


def wall_times(c, step):
    ts = []
    for i in range(STEPS):
        t0 = time.perf_counter()
        step(i)
        c.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def case(w, h, a, b, M, kind, results):
    host = np.stack([synth.blob_frame(w, h, w // 2 + 2 * k, h // 2 + k, a, b, (4, 3, 5), (200, 60, 40), seed=6100 + k) for k in range(NU)])
    rects = [(w // 2 - a + j, h // 2 - b, 2 * a, 2 * b) for j in range(M)]
    fb, ob = w * h * 4, w * h * (8 if kind == "f64" else 4)
    out = torch.empty(M * ob, dtype=torch.uint8, device="cuda")
    # the pair call: one bound frame, streams 0 .. M - 1 on frame 0
    dev = torch.from_numpy(host).cuda()
    cp = Context(options="cs_pairs_force=1")
    cp.set_geometry(w, h, 1)
    cp.camshift_reserve(M)
    pairs = np.zeros(M, dtype=[("stream", "<i4"), ("frame", "<i4")])
    pairs["stream"] = np.arange(M)
    cp.bind_device(dev.data_ptr(), 1)
    cp.camshift_init_pairs(pairs, rects)

    def step_pairs(i):
        cp.bind_device(dev.data_ptr() + (i % NU) * fb, 1)
        cp.camshift_backproject_pairs_device(out.data_ptr(), pairs, kind=kind)

    # the workaround: the frame M times in the bound set, one contiguous call over M streams
    rep = torch.from_numpy(np.repeat(host, M, axis=0)).cuda()
    cb = Context()
    cb.set_geometry(w, h, M)
    cb.camshift_reserve(M)
    cb.bind_device(rep.data_ptr(), M)
    cb.camshift_init(rects)

    def step_batch(i):
        cb.bind_device(rep.data_ptr() + (i % NU) * M * fb, M)
        cb.camshift_backproject_device(out.data_ptr(), M, kind=kind)

    for i in range(WARM):
        step_pairs(i)
        step_batch(i)
    dp, db = device_times(cp, step_pairs), device_times(cb, step_batch)
    wp, wb = [], []
    for _ in range(ROUNDS):  # the two forms take turns
        wp += wall_times(cp, step_pairs)
        wb += wall_times(cb, step_batch)
    bp, bb = bytes_per_pixel(M, kind)
    say(f"{w}x{h} {kind} M={M}: bytes/px pairs {bp} replicated {bb}")
    say(f"  pairs       device us/call {dp} sum {sum(dp.values()):.1f}; wall us/call median {np.median(wp):.1f}")
    say(f"  replicated  device us/call {db} sum {sum(db.values()):.1f}; wall us/call median {np.median(wb):.1f}")
    results[(w, kind, M)] = (sum(dp.values()), sum(db.values()))
    cp.close()
    cb.close()
    del dev, rep, out
    torch.cuda.empty_cache()


def main():
    results = {}
    for w, h, a, b in ((1920, 1080, 180, 120), (320, 240, 30, 18)):
        for kind in ("rgba8", "f64"):
            for M in (1, 2, 4, 8):
                case(w, h, a, b, M, kind, results)
    say("summed device us/call, pairs / replicated: " + ", ".join(f"{w}px {kind} M={M}: {p:.1f} / {r:.1f}" for (w, kind, M), (p, r) in results.items()))
    p, r = results[(1920, "rgba8", 4)]
    say(f"expectation (pair call <= replicated call at M = 4 on 1080p, rgba8): {'holds' if p <= r else 'REFUTED'} ({p:.1f} vs {r:.1f} us)")
    p, r = results[(1920, "f64", 4)]
    say(f"expectation (pair call <= replicated call at M = 4 on 1080p, f64): {'holds' if p <= r else 'REFUTED'} ({p:.1f} vs {r:.1f} us)")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
