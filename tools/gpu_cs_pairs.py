#!/usr/bin/env python3
"""tools/gpu_cs_pairs.py [output file] — M trackers per frame, three ways in the same run and library: the pair call on its one-workgroup
schedule (ht_camshift_track_pairs: one chunk-histogram pass per DISTINCT frame, one mean-shift workgroup per pair), the pair call on the
cluster schedule (option cs_pairs_cluster=1: k_csp_lut + G workgroups per pair where ht_cs_plan_track_pairs takes it), and the workaround
the contiguous API offers (the frames replicated M times in the bound set, one ht_camshift_track_batch over F x M streams).  Per case:
device us per kernel (ht_profile / ht_kernel_times, HIP events, calls strictly in turn) and wall us per synchronous call; for the pair
forms also initTracker (csp_init against csp_init_rows, which times the model zeroing with the row kernel, under the option).

    64 frames of 320x240 x M = 1, 2, 4        8 frames of 1920x1080 x M = 1, 4        1 frame of 1920x1080 x M = 1, 2, 4, 8 (360 x 360 windows)

Three things to read off: whether csp_hist follows the number of distinct frames and not the number of pairs, where the pair path loses
(the single-launch kernel from 192 replicated streams on), and what decides the default of cs_pairs_cluster: csp_lut +
csp_meanshift_cluster against csp_meanshift, and csp_init_rows against csp_init, on the 1080p rows."""
import functools
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

STEPS, WARM, NU = 40, 10, 4  # calls measured / warm-up calls / distinct frame sets the calls cycle through
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


@functools.lru_cache(maxsize=2)
def frames_of(F, w, h, a, b):
    """NU sets of F frames: one blob per frame, drifting 2 px per set"""
    out = np.empty((NU, F, h, w, 4), dtype=np.uint8)
    for k in range(NU):
        for f in range(F):
            out[k, f] = synth.blob_frame(w, h, w // 2 + 2 * k + (f % 5), h // 2 + k - (f % 3), a, b, (4, 3, 5), (200, 60, 40), seed=6000 + 7 * f + k)
    return out


def measure(c, step, label, wall=True):
    for i in range(WARM):
        step(i)
    c.synchronize()
    c.profile(True)
    c.kernel_times(reset=True)
    for i in range(STEPS):
        step(i)
    kt = c.kernel_times(reset=True)
    c.profile(False)
    per = {k: round(v["ms"] / STEPS * 1e3, 2) for k, v in kt.items() if v["launches"] and v["ms"] > 0}
    c.synchronize()
    if not wall:
        say(f"  {label:<34} device us/call {per} sum {sum(per.values()):.1f}")
        return per
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(STEPS):
            step(i)
        c.synchronize()
        ts.append((time.perf_counter() - t0) / STEPS * 1e6)
    say(f"  {label:<34} device us/call {per} sum {sum(per.values()):.1f}; wall us/call median {np.median(ts):.1f}")
    return per


def case(F, w, h, a, b, M):
    host = frames_of(F, w, h, a, b)
    rect = (w // 2 - a, h // 2 - b, 2 * a, 2 * b)
    fb = w * h * 4
    say(f"{F} frames of {w}x{h} x {M} trackers per frame ({F * M} trackers):")
    # the pair call: F bound frames, stream f * M + j on frame f — one workgroup per pair, then the cluster schedule
    dev = torch.from_numpy(host).cuda()
    pairs = np.zeros(F * M, dtype=[("stream", "<i4"), ("frame", "<i4")])
    pairs["stream"], pairs["frame"] = np.arange(F * M), np.arange(F * M) // M
    rects = [(rect[0] + (j % M), rect[1], rect[2], rect[3]) for j in range(F * M)]
    pp = pc = None
    for options, label in (("cs_pairs_force=1", "track_pairs"), ("cs_pairs_force=1,cs_pairs_cluster=1", "track_pairs, cs_pairs_cluster=1")):
        cp = Context(options=options)
        cp.set_geometry(w, h, F)
        cp.camshift_reserve(F * M)
        cp.bind_device(dev.data_ptr(), F)

        def step_init(i):
            cp.camshift_init_pairs(pairs, rects)

        measure(cp, step_init, "init_pairs" + label[len("track_pairs"):], wall=False)

        def step_pairs(i):
            cp.bind_device(dev.data_ptr() + (i % NU) * F * fb, F)
            cp.camshift_track_pairs(pairs)

        got = measure(cp, step_pairs, label)
        pp, pc = (got, pc) if pp is None else (pp, got)
        cp.close()
    del dev
    # the workaround: every frame M times in the bound set, one contiguous call over F * M streams
    rep = torch.from_numpy(np.repeat(host, M, axis=1)).cuda()
    cb = Context()
    cb.set_geometry(w, h, F * M)
    cb.camshift_reserve(F * M)
    cb.bind_device(rep.data_ptr(), F * M)
    cb.camshift_init(rects)

    def step_batch(i):
        cb.bind_device(rep.data_ptr() + (i % NU) * F * M * fb, F * M)
        cb.camshift_track(F * M)

    pb = measure(cb, step_batch, f"track_batch on {F * M} replicated")
    cb.close()
    del rep
    torch.cuda.empty_cache()
    return pp, pc, pb


def main():
    hist, forms = {}, []
    for F, w, h, a, b, Ms in ((64, 320, 240, 30, 18, (1, 2, 4)), (8, 1920, 1080, 180, 120, (1, 4)), (1, 1920, 1080, 180, 180, (1, 2, 4, 8))):
        for M in Ms:
            pp, pc, _pb = case(F, w, h, a, b, M)
            hist[(F, w, M)] = pp.get("csp_hist")
            if "csp_meanshift_cluster" in pc:
                forms.append(f"{F} x {w}px-wide x M={M}: {pp.get('csp_meanshift')} -> {round(pc.get('csp_lut', 0) + pc['csp_meanshift_cluster'], 2)}")
    say("csp_hist us/call by trackers per frame: " + ", ".join(f"{F} x {w}px-wide x M={M}: {v}" for (F, w, M), v in hist.items()))
    say("csp_meanshift -> csp_lut + csp_meanshift_cluster us/call where the option takes the cluster form: " + ", ".join(forms))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
