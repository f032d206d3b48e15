#!/usr/bin/env python3
"""tools/gpu_init_faces.py [output file] — the detect -> track hand-off for SEVERAL faces per feed, on the host and on the device, in ONE
process and alternating blocks: 8 frame-synchronous feeds with 4 faces each, 4 tracker slots per feed (32 trackers), detect every 30th
step, camshift.track on all 32 (stream, frame) pairs in between, two track steps outstanding.

  host    the hand-off as a host has to issue it today: the detect and its device grouping are enqueued behind the track steps in flight,
          the queue is drained, detect_best_collect, ht_detect_grouped per frame, the rule of ht_camshift_init_faces in Python (with the
          search windows of the last track result), camshift_init_pairs; only then is the next track step enqueued.
  device  detect_enqueue, detect_best_enqueue, camshift_init_faces(associate) and the following track steps are enqueued without
          draining; the batch is collected behind the first of those track steps.

Per shape and arm: frames/s of the loop (median over the blocks), the wall time from a detect step's enqueue to the first following track
result on the host, and — from a profiled pass of its own (ht_profile: HIP events, not part of the timed blocks) — the device time of
k_csf_resolve next to k_csb_resolve (one ht_camshift_init_best of the 8 feeds on the same batch) and of the init launches.  Whether both
arms end their last block with the same track objects is reported.  The baseline is the host arm of the same run."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from headtrackr_amd import synth  # noqa: E402
from headtrackr_amd.api import Context  # noqa: E402

K, SLOTS, NUNIQ, STEPS, BLOCKS = 8, 4, 30, 300, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def overlap(a, b):
    if a[2] <= 0 or a[3] <= 0 or b[2] <= 0 or b[3] <= 0:
        return 0
    w = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    h = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    return w * h if w > 0 and h > 0 else 0


def host_rule(faces, windows):
    """the rule with HT_CSF_ASSOCIATE and threshold -10 for one frame: -> {slot: rect}"""
    el = sorted((i for i in range(len(faces)) if faces["neighbors"][i] > 0 and faces["confidence"][i] > -10.0), key=lambda i: (-faces["confidence"][i], i))[:len(windows)]
    rects = [tuple(int(math.floor(faces[k][i])) for k in ("x", "y", "width", "height")) for i in el]
    live = [w[2] > 0 and w[3] > 0 for w in windows]
    out, free = {}, list(range(len(rects)))
    for _o, j, r in sorted((-overlap(windows[j], rects[r]), j, r) for j in range(len(windows)) if live[j] for r in free):
        if _o < 0 and j not in out and r in free:
            out[j] = r
            free.remove(r)
    rest = [j for j in range(len(windows)) if not live[j]] + [j for j in range(len(windows)) if live[j] and j not in out]
    for j, r in zip(rest, free):
        out[j] = r
    return {j: rects[r] for j, r in out.items()}


class Loop:
    def __init__(self, w, h, dev, device_arm):
        self.w, self.h, self.dev, self.device_arm = w, h, dev, device_arm
        self.sbytes = K * w * h * 4
        self.ctx = c = Context()
        c.set_geometry(w, h, K)
        c.camshift_reserve(K * SLOTS)
        self.pairs = [(f * SLOTS + j, f) for j in range(SLOTS) for f in range(K)]  # slot j of feed f; the feeds' slots interleaved
        self.n = len(self.pairs)
        self.handoff_us = []
        self.last = None
        self.inited = False

    def host_handoff(self):
        c = self.ctx
        c.detect_best_collect()
        pairs, rects = [], []
        for f in range(K):
            slots = [i for i, (_s, pf) in enumerate(self.pairs) if pf == f]
            wins = [(self.w // 4, self.h // 4, self.w // 2, self.h // 2)] * SLOTS if self.last is None else [tuple(int(self.last[i][k]) for k in ("sw_x", "sw_y", "sw_width", "sw_height")) for i in slots]
            for j, r in host_rule(c.detect_grouped(f), wins).items():
                pairs.append(self.pairs[slots[j]])
                rects.append(r)
        if pairs:
            c.camshift_init_pairs(pairs, rects)

    def run(self, steps):
        """one block; returns seconds"""
        c, pend, t_detect, uncollected = self.ctx, [], None, False
        if not self.inited:  # every slot starts as a tracker on the centre half: no track step ever meets a stream without a model
            c.bind_device(self.dev.data_ptr(), K)
            c.camshift_init_pairs(self.pairs, [(self.w // 4, self.h // 4, self.w // 2, self.h // 2)] * self.n)
            self.inited = True
        t0 = time.perf_counter()
        for i in range(steps):
            c.bind_device(self.dev.data_ptr() + (i % NUNIQ) * self.sbytes, K)
            if i % 30 == 0:
                t_detect = time.perf_counter()
                c.detect_enqueue(0)
                c.detect_best_enqueue(1)
                if self.device_arm:
                    c.camshift_init_faces(self.pairs, -10.0, associate=True)
                    uncollected = True
                else:
                    while pend:
                        pend.pop(0)
                        self.last = c.camshift_track_collect(self.n)
                    self.host_handoff()
                continue
            c.camshift_track_pairs(self.pairs, calc_angles=True, fetch=False)
            pend.append(i)
            if uncollected:  # the batch, whenever the host wants it: behind the first track step that follows
                c.detect_best_collect()
                uncollected = False
            if len(pend) > 1:
                j = pend.pop(0)
                self.last = c.camshift_track_collect(self.n)
                if t_detect is not None and j % 30 == 1:
                    self.handoff_us.append((time.perf_counter() - t_detect) * 1e6)
                    t_detect = None
        while pend:
            pend.pop(0)
            self.last = c.camshift_track_collect(self.n)
        if uncollected:
            c.detect_best_collect()
        return time.perf_counter() - t0

    def profiled(self):
        c = self.ctx
        c.synchronize()
        c.profile(True)
        c.kernel_times(reset=True)
        self.run(61)
        if self.device_arm:  # k_csb_resolve next to it: one best-face hand-off of the 8 feeds on the batch collected last, then the slots again
            c.camshift_init_best([(f * SLOTS, f) for f in range(K)], -10.0, None)
            c.camshift_init_faces(self.pairs, -10.0, associate=True)
        c.synchronize()
        kt = c.kernel_times(reset=True)
        c.profile(False)
        names = ("csf_resolve", "csb_resolve", "csp_init", "csp_init_rows")
        return {k: round(v["ms"] / v["launches"] * 1e3, 2) for k, v in kt.items() if k in names and v["launches"]}


def feed_frames(w, h):
    """NUNIQ frames of one camera: four faces drifting 2 px right / 1 px down per frame"""
    s = h // 5
    base = [(w // 16, h // 10), (w // 16 + w // 4, h // 2), (w // 2, h // 12), (w // 2 + w // 5, h // 2 + h // 12)]
    return np.stack([synth.face_frame(w, h, [(x + 2 * k % 24, y + k % 12, s) for x, y in base]) for k in range(NUNIQ)])


def shape(w, h):
    uniq = feed_frames(w, h)
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
    say(f"{K} feeds x {SLOTS} slots, {w}x{h}, {STEPS} steps per block, {BLOCKS} alternating blocks; last track objects of the two arms: {'the same bytes' if agree else 'DIFFERENT'}:")
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
    for w, h in ((1280, 720), (320, 240)):
        shape(w, h)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
