"""Inputs of the (stream, frame) pair tests (tests/test_gpu_camshift_pairs.py, tests/js/pairs_*.js) and their expectations from the CPU
oracle.  A plain module like tests/cs_cases.py; tests/test_pairs_cpu.py proves, from the oracle alone, that every sequence here keeps its
objects and that the reference does not depend on the summation order on any of its calls — which is what entitles the GPU tests to demand
the oracle's integers on every call.

Frames with several blobs are built from headtrackr_amd/synth.py only: the noise frame of a seed, and for every blob the blob_frame of the
same seed, whose pixels that differ from the noise frame are copied in (blob_frame draws its ellipse over exactly that noise)."""
import functools
import math

import numpy as np

import cs_cases as cc
from headtrackr_amd import synth
from oracle import ht_oracle as ho


def multi_blob_frame(w, h, blobs, seed):
    """blobs: [(cx, cy, a, b, rot, color)], later ones on top"""
    base = synth.noise_frame(w, h, seed)
    out = base.copy()
    for (cx, cy, a, b, rot, color) in blobs:
        bf = synth.blob_frame(w, h, cx, cy, a, b, rot, color, seed)
        m = (bf != base).any(axis=2)
        out[m] = bf[m]
    return out


class MultiSeq:
    """M trackers on ONE sequence of frames: frames[0] initialises tracker j on rects[j], every later frame is one track() of each"""

    def __init__(self, name, w, h, blobs_per_frame, seeds, tags=()):
        self.name, self.w, self.h, self.blobs, self.seeds, self.tags = name, w, h, blobs_per_frame, list(seeds), tuple(tags)
        self.rects = [(cx - a, cy - b, 2 * a, 2 * b) for (cx, cy, a, b, _r, _c) in blobs_per_frame[0]]

    @property
    def ntrackers(self):
        return len(self.rects)

    @property
    def ncalls(self):
        return len(self.seeds) - 1

    @functools.cached_property
    def frames(self):
        return [multi_blob_frame(self.w, self.h, bl, sd) for bl, sd in zip(self.blobs, self.seeds)]

    def specs(self):
        """generator specs of the frames (JSON-able): what tests/golden/multitrack.json stores instead of pixels"""
        return [dict(seed=int(sd), blobs=[dict(cx=int(cx), cy=int(cy), a=int(a), b=int(b), rot=list(rot), color=list(col)) for (cx, cy, a, b, rot, col) in bl])
                for bl, sd in zip(self.blobs, self.seeds)]

    def oracle_calls(self, j=None):
        """tracker j: [(search window before, search window after, track object)] per call; j None: the list of all trackers' lists"""
        if j is None:
            return [self.oracle_calls(i) for i in range(self.ntrackers)]
        o = ho.Camshift(True)
        o.init_tracker(self.frames[0], self.rects[j])
        out = []
        for f in self.frames[1:]:
            before = o.search_window()
            sw, to = o.track(f)
            out.append((before, sw, to))
        return out

    def expected(self):
        """[tracker][call] -> (search window, track object), computed once"""
        if not hasattr(self, "_expected"):
            self._expected = [[(sw, to) for (_b, sw, to) in calls] for calls in self.oracle_calls()]
        return self._expected


def seq_from_specs(name, w, h, specs):
    blobs = [[(b["cx"], b["cy"], b["a"], b["b"], tuple(b["rot"]), tuple(b["color"])) for b in s["blobs"]] for s in specs]
    return MultiSeq(name, w, h, blobs, [s["seed"] for s in specs])


# ---- three trackers per frame ---------------------------------------------------------------------------------------------------------

FEED_CALLS = 4


@functools.lru_cache(maxsize=None)
def feed_scene(f, w=320, h=240, calls=FEED_CALLS):
    """feed f: three blobs side by side (thirds of the frame), each with its own size, rotation, colour and walk of <= 3 px per call"""
    tracks = []
    for j in range(3):
        r = synth.lcg_stream(9000 + 131 * (8 * f + j), 16).astype(np.int64) >> 12
        cx, cy = w * (2 * j + 1) // 6 + int(r[0] % 21) - 10, h // 2 + int(r[1] % 61) - 30
        a, b = 14 + int(r[2] % 14), 10 + int(r[3] % 10)
        walk = [int(v % 7) - 3 for v in r[6:14]]
        pos = [(cx, cy)]
        for k in range(calls):
            pos.append((pos[-1][0] + walk[(2 * k) % 8], pos[-1][1] + walk[(2 * k + 1) % 8]))
        tracks.append((pos, a, b, cc.ROTS[int(r[4] % 5)], cc.COLORS[(j + f) % 4]))
    blobs = [[(pos[k][0], pos[k][1], a, b, rot, col) for (pos, a, b, rot, col) in tracks] for k in range(calls + 1)]
    return MultiSeq(f"feed{f}-{w}x{h}", w, h, blobs, [9500 + 17 * f + k for k in range(calls + 1)])


def three_per_frame(nfeeds=6):
    return [feed_scene(f) for f in range(nfeeds)]


# ---- two blobs of the same colour: both models match both blobs, only the search windows tell them apart ------------------------------------

@functools.lru_cache(maxsize=None)
def same_colour(w, h, calls=4):
    blobs = [[(w // 4 + 2 * k, h // 2 + k, 26, 16, (4, 3, 5), cc.COLORS[0]), (3 * w // 4 - 3 * k, h // 2 - 2 * k, 20, 24, (1, 0, 1), cc.COLORS[0])]
             for k in range(calls + 1)]
    return MultiSeq(f"same-colour-{w}x{h}", w, h, blobs, [9900 + k for k in range(calls + 1)])


SAME_COLOUR_SIZES = [(320, 240), (641, 363)]


# ---- many pairs: 50 small frames x 4 trackers ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_scene(f, w=160, h=120, calls=2):
    """four blobs in the quadrants of a 160 x 120 frame, one colour each"""
    r = synth.lcg_stream(9300 + 53 * f, 16).astype(np.int64) >> 12
    blobs = []
    for k in range(calls + 1):
        bl = []
        for j in range(4):
            cx, cy = w * (2 * (j % 2) + 1) // 4 + int(r[j] % 9) - 4, h * (2 * (j // 2) + 1) // 4 + int(r[4 + j] % 7) - 3
            bl.append((cx + k * (int(r[8 + j] % 5) - 2), cy + k * (int(r[12 + j] % 3) - 1), 12 + int(r[j] % 5), 8 + int(r[4 + j] % 4), cc.ROTS[(f + j) % 5],
                       cc.COLORS[(j + f) % 4]))
        blobs.append(bl)
    return MultiSeq(f"small{f}", w, h, blobs, [9700 + 7 * f + k for k in range(calls + 1)])


def many_pairs(nframes=50):
    return [small_scene(f) for f in range(nframes)]


# ---- two trackers on 1080p windows too large for the LDS region (the uncached path) --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def large_1080p(calls=2):
    w, h = 1920, 1080
    blobs = [[(520 + 3 * k, 500 + k, 180, 120, (4, 3, 5), cc.COLORS[0]), (1350 - 2 * k, 560 + 2 * k, 150, 130, (1, 0, 1), cc.COLORS[2])] for k in range(calls + 1)]
    return MultiSeq("large-1080p", w, h, blobs, [9950 + k for k in range(calls + 1)], tags=("uncached",))


def error_scene():
    """eight calls of one three-blob scene: a valid call behind every refused one (the error-path test)"""
    return feed_scene(7, 320, 240, 8)


def all_multi_sequences():
    """every multi-tracker sequence a GPU test compares with the oracle; the CPU guard runs both of its checks over all of them"""
    return three_per_frame() + [same_colour(w, h) for w, h in SAME_COLOUR_SIZES] + many_pairs() + [large_1080p(), error_scene()]


# ---- the per-feed-state loop (main.js:229-244, facetrackr.js:97-108) ---------------------------------------------------------------------------

LOOP_W, LOOP_H, LOOP_FEEDS, LOOP_STEPS = 320, 240, 4, 12
# feed -> first step without its face; the face is back two steps later.  The face-less frame is face_frame with no face (the flat
# background), NOT a noise frame: on noise the reference does not lose its object — every model bin occurs somewhere in a noise window, so
# m00 > 0 and track() returns a large window (the oracle gives 116 x 120 and 140 x 160 on the two noise frames of feed 1) — while on the
# flat background no pixel of the window carries weight, m00 = 0, and width = height = 0 (camshift.js:230-241), which is what main.js:229
# tests for.
LOOP_LOST = {1: 4, 3: 7}
LOOP_FACE = [(60, 50, 96), (150, 70, 88), (90, 90, 104), (170, 40, 92)]  # (x, y, size) of feed f's face at step 0


def loop_frame(f, k):
    if f in LOOP_LOST and LOOP_LOST[f] <= k < LOOP_LOST[f] + 2:
        return synth.face_frame(LOOP_W, LOOP_H, [])
    x, y, s = LOOP_FACE[f]
    return synth.face_frame(LOOP_W, LOOP_H, [(x + (2 - f % 3) * k, y + (f % 2) * k, s)])


@functools.lru_cache(maxsize=None)
def loop_frames():
    """[step][feed] -> frame"""
    return [[loop_frame(f, k) for f in range(LOOP_FEEDS)] for k in range(LOOP_STEPS)]


def floored_rect(best):
    return [math.floor(best["x"]), math.floor(best["y"]), math.floor(best["width"]), math.floor(best["height"])]  # facetrackr.js:185-190


def loop_feed_oracle(f, cascade_blob):
    """feed f's own loop on the oracle: VJ until confidence > -10, initTracker on the floored rect, CS until width or height is 0, VJ
    again.  One record per step: dict(mode="VJ", best=rect record, found=bool) or dict(mode="CS", before, sw, to, lost=bool)."""
    out, tracker = [], None
    for k in range(LOOP_STEPS):
        frame = loop_frames()[k][f]
        if tracker is None:
            best = ho.best_faces([frame], cascade_blob, 1)[0]
            found = bool(best["confidence"] > -10)  # facetrackr.js:97
            out.append(dict(mode="VJ", best=best.copy(), found=found))
            if found:
                tracker = ho.Camshift(True)
                tracker.init_tracker(frame, floored_rect(best))
        else:
            before = tracker.search_window()
            sw, to = tracker.track(frame)
            lost = to["width"] == 0 or to["height"] == 0  # main.js:229-238
            out.append(dict(mode="CS", before=before, sw=sw, to=to, lost=lost))
            if lost:
                tracker = None
    return out


_LOOP = {}


def loop_oracle(cascade_blob):
    """[feed][step] records, computed once per process (the real oracle)"""
    if "v" not in _LOOP:
        _LOOP["v"] = [loop_feed_oracle(f, cascade_blob) for f in range(LOOP_FEEDS)]
    return _LOOP["v"]


# ---- scattered streams, shuffled pair order ---------------------------------------------------------------------------------------------------

def scattered_streams(npairs, reserved, seed):
    """npairs distinct stream slots spread with gaps through a reservation (never 0 .. npairs-1 in order)"""
    r = synth.lcg_stream(seed, 4 * reserved).astype(np.int64) >> 8
    order = sorted(range(reserved), key=lambda s: (int(r[s]), s))
    return order[:npairs]


def shuffled(n, seed):
    r = synth.lcg_stream(seed, n).astype(np.int64) >> 8
    return sorted(range(n), key=lambda i: (int(r[i]), i))


# ---- the job of tests/js/pairs_common.js ------------------------------------------------------------------------------------------------------

def _call(to, sw, lost=False):
    a = to["angle"]
    return dict(to=[to["x"], to["y"], to["width"], to["height"], None if math.isnan(a) else a], sw=[int(v) for v in sw], lost=bool(lost))


def js_job(tmp, cascade_blob, golden):
    """writes the raw frame files into directory `tmp` and returns the job dict: two feeds x three trackers on scattered streams of a
    reservation of 10 with shuffled pair order, the per-feed-state loop, and the recorded multi-tracker cases"""
    import os

    feeds = [feed_scene(0), feed_scene(1)]
    ncalls = FEED_CALLS
    sets = []
    for k in range(ncalls + 1):
        p = os.path.join(str(tmp), f"batch_{k}.raw")
        np.stack([s.frames[k] for s in feeds]).tofile(p)
        sets.append(p)
    trackers = [(f, j) for f in range(len(feeds)) for j in range(3)]
    streams = scattered_streams(len(trackers), 10, 9111)
    init_pairs, rects = [], []
    for (f, j), s in zip(trackers, streams):
        init_pairs += [s, f]
        rects += list(feeds[f].rects[j])
    calls = []
    for k in range(1, ncalls + 1):
        order = shuffled(len(trackers), 9200 + k)
        pairs, expect = [], []
        for i in order:
            f, j = trackers[i]
            pairs += [streams[i], f]
            sw, to = feeds[f].expected()[j][k - 1]
            expect.append(_call(to, sw))
        calls.append(dict(set=k, pairs=pairs, expect=expect))
    batch = dict(w=feeds[0].w, h=feeds[0].h, n=len(feeds), trackers=10, sets=sets, init_pairs=init_pairs, rects=[int(v) for v in rects], calls=calls)

    lsets = []
    for k in range(LOOP_STEPS):
        p = os.path.join(str(tmp), f"loop_{k}.raw")
        np.stack(loop_frames()[k]).tofile(p)
        lsets.append(p)
    lexp = []
    for recs in loop_oracle(cascade_blob):
        row = []
        for r in recs:
            if r["mode"] == "VJ":
                b = r["best"]
                row.append(dict(mode="VJ", best=[float(b[q]) for q in ("x", "y", "width", "height", "confidence")], found=r["found"]))
            else:
                row.append(dict(mode="CS", **_call(r["to"], r["sw"], r["lost"])))
        lexp.append(row)
    loop = dict(w=LOOP_W, h=LOOP_H, n=LOOP_FEEDS, sets=lsets, expect=lexp)

    multi = []
    for c in golden["cases"]:
        s = seq_from_specs(c["name"], c["w"], c["h"], c["gen"])
        files = []
        for k, f in enumerate(s.frames):
            files.append(os.path.join(str(tmp), f"{c['name']}_{k}.raw"))
            f.tofile(files[-1])
        multi.append(dict(name=c["name"], w=c["w"], h=c["h"], rects=c["rects"], frames=files, trackers=c["trackers"]))
    return dict(angle_tol=cc.ANGLE_TOL, batch=batch, loop=loop, multi=multi)
