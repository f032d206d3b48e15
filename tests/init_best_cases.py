"""Inputs of the record-driven initTracker (ht_camshift_init_best): tests/test_init_best_cpu.py, tests/test_gpu_init_best.py.  A plain
module, imported like tests/group_cases.py.

One 320 x 240 batch of six frames: five recorded frames of tests/golden/detect.json and a frame tiled with 15 faces, whose 129 raw hits
are above the lowest grouping cap (group_cap=64) and below the default one.  What every call must decide always comes from the CPU
oracle (best_faces) and from Math.floor as Python's math.floor gives it; tests/test_init_best_cpu.py proves from the oracle alone that
every frame reaches the state it is named after."""
import functools
import math
import zlib

import numpy as np

from conftest import load_golden
from headtrackr_amd import native, synth
from oracle import ht_oracle as ho

W, H = 320, 240
GOLDEN_FRAMES = ("two_faces_320x240", "noise_320x240", "mixed2_320x240", "c1_face_320x240", "mixed5_320x240")
TILED_GEN = {"family": "face", "faces": [[x, y, 48] for y in range(2, 192, 64) for x in range(2, 272, 64)]}
TILED = len(GOLDEN_FRAMES)  # its frame index
NOISE = GOLDEN_FRAMES.index("noise_320x240")
NFRAMES = TILED + 1
THRESHOLDS = (-10.0, 5.0)  # the reference's (facetrackr.js:97) and one that splits the frames differently

UNTOUCHED, FACE, FALLBACK, DEFERRED = native.HT_CSB_UNTOUCHED, native.HT_CSB_FACE, native.HT_CSB_FALLBACK, native.HT_CSB_DEFERRED


@functools.lru_cache(maxsize=None)
def frames():
    by_name = {c["name"]: c for c in load_golden("detect.json")["cases"]}
    out = []
    for name in GOLDEN_FRAMES:
        c = by_name[name]
        assert (c["w"], c["h"]) == (W, H)
        f = synth.make(c["gen"], W, H)
        assert zlib.crc32(f.tobytes()) == c["input_crc"]
        out.append(f)
    out.append(synth.make(TILED_GEN, W, H))
    out = np.ascontiguousarray(np.stack(out))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def raw_counts(cascade_blob):
    return tuple(len(ho.detect_raw(f, cascade_blob)) for f in frames())


@functools.lru_cache(maxsize=None)
def best(cascade_blob, min_neighbors=1):
    """the oracle's best face per frame (facetrackr.js:147-175); computed once"""
    b = ho.best_faces(frames(), cascade_blob, min_neighbors)
    b.setflags(write=False)
    return b


def js_floor_i32(v):
    """Math.floor(v) as the library stores it: int32, saturated, NaN -> 0"""
    if v != v:
        return 0
    if v >= 2147483647.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(math.floor(v))


def floor_rect(r):
    return tuple(js_floor_i32(float(r[k])) for k in ("x", "y", "width", "height"))


def decide(rec, min_confidence, fallback=None, deferred=False):
    """(code, rect) of one pair: rec = a best-face rect (fields x .. neighbors), facetrackr.js:97-107"""
    if deferred:
        return DEFERRED, (0, 0, 0, 0)
    if rec["neighbors"] > 0 and float(rec["confidence"]) > min_confidence:
        return FACE, floor_rect(rec)
    if fallback is not None:
        return FALLBACK, tuple(int(v) for v in fallback)
    return UNTOUCHED, (0, 0, 0, 0)


def expected(cascade_blob, pairs, min_confidence, fallback=None, deferred_frames=()):
    """codes [n] and rects [n] (tuples) for a pair list on this batch"""
    b = best(cascade_blob)
    out = [decide(b[f], min_confidence, None if fallback is None else fallback[i], f in deferred_frames) for i, (_s, f) in enumerate(pairs)]
    return [c for c, _r in out], [r for _c, r in out]


def centre_half():
    """detectStepFinish's fallback rect: the centre half of the canvas"""
    return (W >> 2, H >> 2, W >> 1, H >> 1)


# the pair list of the GPU tests: streams in shuffled order meet frames 0 .. 5, two further streams meet frame 0 as well
STREAMS = 8
PAIRS = [(5, 0), (0, 1), (3, 2), (1, 3), (4, 4), (2, 5), (6, 0), (7, 0)]
