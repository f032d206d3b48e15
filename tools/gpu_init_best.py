#!/usr/bin/env python3
"""tools/gpu_init_best.py [output file] — the detect -> track hand-off of the resident C5-shaped loop, on the host and on the device, in ONE
process and alternating blocks: 8 frame-synchronous feeds, detect every 30th step, camshift.track in between, two track steps outstanding.

  host    the hand-off exactly as benchlib/c5.py issues it: the detect is enqueued behind the track steps in flight, the queue is drained,
          detect_collect_best brings the best faces to the host, which floors them (init_rects) and calls camshift_init; only then is the
          next track step enqueued.
  device  detect_enqueue, detect_best_enqueue, camshift_init_best (threshold -10, centre-half fallback) and the following track steps are
          enqueued without draining; the best faces are collected behind the first of those track steps.

Per shape (8 x 1920x1080, 8 x 320x240) and arm: frames/s of the loop (median over the blocks), the wall time from a detect step's enqueue
to the first following track result on the host, and — from a profiled pass of its own (ht_profile: HIP events, not part of the timed
blocks) — the device time of k_csb_resolve and of the init launches.  Whether both arms end their last block with the same track objects is reported.
The baseline is the host arm of the same run."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

K, NUNIQ, STEPS, BLOCKS = 8, 30, 300, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def init_rects(best, w, h):
    """benchlib/c5.py's: initTracker on the floored best face, the centre half where nothing was found"""
    fl = np.floor(np.stack([best["x"], best["y"], best["width"], best["height"]], axis=1)).astype(np.int64)
    return [tuple(fl[f]) if best["neighbors"][f] > 0 and best["confidence"][f] > -10 else (w // 4, h // 4, w // 2, h // 2) for f in range(K)]


class Loop:
    def __init__(self, w, h, dev, device_arm):
        self.w, self.h, self.dev, self.device_arm = w, h, dev, device_arm
        self.sbytes = K * w * h * 4
        self.ctx = c = Context()
        c.set_geometry(w, h, K)
        c.camshift_reserve(K)
        self.pairs = [(f, f) for f in range(K)]
        self.fallback = [(w // 4, h // 4, w // 2, h // 2)] * K
        self.handoff_us = []
        self.last = None

    def run(self, steps):
        """one block; returns seconds"""
        c, pend, t_detect, uncollected = self.ctx, [], None, False
        t0 = time.perf_counter()
        for i in range(steps):
            c.bind_device(self.dev.data_ptr() + (i % NUNIQ) * self.sbytes, K)
            if i % 30 == 0:
                t_detect = time.perf_counter()
                c.detect_enqueue(0)
                if self.device_arm:
                    c.detect_best_enqueue(1)
                    c.camshift_init_best(self.pairs, -10.0, self.fallback)
                    uncollected = True
                else:
                    while pend:
                        pend.pop(0)
                        self.last = c.camshift_track_collect(K)
                    c.camshift_init(init_rects(c.detect_collect_best(1)[0], self.w, self.h))
                continue
            c.camshift_track(K, calc_angles=True, fetch=False)
            pend.append(i)
            if uncollected:  # the best faces, whenever the host wants them: behind the first track step that follows
                c.detect_best_collect()
                uncollected = False
            if len(pend) > 1:
                j = pend.pop(0)
                self.last = c.camshift_track_collect(K)
                if t_detect is not None and j % 30 == 1:
                    self.handoff_us.append((time.perf_counter() - t_detect) * 1e6)
                    t_detect = None
        while pend:
            pend.pop(0)
            self.last = c.camshift_track_collect(K)
        if uncollected:
            c.detect_best_collect()
        return time.perf_counter() - t0

    def profiled(self):
        c = self.ctx
        c.synchronize()
        c.profile(True)
        c.kernel_times(reset=True)
        self.run(61)
        c.synchronize()
        kt = c.kernel_times(reset=True)
        c.profile(False)
        names = ("csb_resolve", "csp_init", "csp_init_rows", "cs_init")
        return {k: round(v["ms"] / v["launches"] * 1e3, 2) for k, v in kt.items() if k in names and v["launches"]}


def shape(w, h):
    uniq = synth.stream_feed_frames(NUNIQ, w, h, 0)
    host = np.empty((NUNIQ, K, h, w, 4), dtype=np.uint8)
    for k in range(NUNIQ):
        for f in range(K):
            host[k, f] = uniq[synth.stream_frame_index(k, f, NUNIQ)]
    dev = torch.from_numpy(host).cuda()
    arms = {"host": Loop(w, h, dev, False), "device": Loop(w, h, dev, True)}
    for a in arms.values():
        a.run(61)
        a.handoff_us.clear()
    fps = {k: [] for k in arms}
    for _ in range(BLOCKS):  # alternating blocks
        for name, a in arms.items():
            fps[name].append(K * STEPS / a.run(STEPS))
    agree = arms["host"].last.tobytes() == arms["device"].last.tobytes()
    say(f"{K} x {w}x{h}, {STEPS} steps per block, {BLOCKS} alternating blocks; last track objects of the two arms: {'the same bytes' if agree else 'DIFFERENT'}:")
    for name, a in arms.items():
        v, hu = np.array(fps[name]), np.array(a.handoff_us)
        say(f"  {name:<7} frames/s median {np.median(v):.0f} (min {v.min():.0f}, max {v.max():.0f}); detect enqueue -> first following track result on the host: "
            f"median {np.median(hu):.1f} us (min {hu.min():.1f}, n = {len(hu)}); device us per launch {a.profiled()}")
    say(f"  device / host frames/s: {np.median(fps['device']) / np.median(fps['host']):.4f}")
    for a in arms.values():
        a.ctx.close()
    del dev
    torch.cuda.empty_cache()


def main():
    for w, h in ((1920, 1080), (320, 240)):
        shape(w, h)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
