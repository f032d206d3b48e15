"""Inputs and expectations of the device drawImage (ht_draw_frames / ht_draw_frames_device; main.js:170), shared by
tests/test_ingest_cpu.py (which pins `expected` to oracle/canvas_shim.js, headtrackr_amd/js/canvas.js and the reference's recorded
canvases) and tests/test_gpu_ingest.py (which compares the GPU with it).  Everything is seeded; nothing is read from outside the tree."""
import ctypes as C
import json
import os
import zlib

import numpy as np

from conftest import GOLDEN
from headtrackr_amd import synth
from oracle import ht_oracle as ho


def expected(src, rect, dw, dh):
    """drawImage(src, sx, sy, sw, sh, 0, 0, dw, dh) by the oracle: src uint8 [SH, SW, 4], rect = (sx, sy, sw, sh) or None (the whole
    frame) -> uint8 [dh, dw, 4].  The channels are de-interleaved, ho_resample (oracle/ht_oracle.c: the declared resampler on one byte
    plane) runs once per channel with the rect, and the result is interleaved again."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    SH, SW, _ = src.shape
    sx, sy, sw, sh = (0, 0, SW, SH) if rect is None else [int(v) for v in rect]
    assert 0 <= sx and 0 <= sy and sw > 0 and sh > 0 and sx + sw <= SW and sy + sh <= SH
    out = np.empty((dh, dw, 4), dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    for ch in range(4):
        plane = np.ascontiguousarray(src[..., ch])
        dst = np.zeros((dh, dw), dtype=np.uint8)
        ho.lib().ho_resample(plane.ctypes.data_as(u8p), SW, sx, sy, sw, sh, dst.ctypes.data_as(u8p), dw, dw, dh)
        out[..., ch] = dst
    return out


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ---- content ----------------------------------------------------------------------------------------------------------------------------

def noise(w, h, seed):
    """all four channels random (alpha too: the resampler treats it like any other channel)"""
    s = synth.lcg_stream(seed, 4 * w * h)
    return (s >> np.uint32(24)).astype(np.uint8).reshape(h, w, 4)


def smooth(w, h, seed):
    f = synth.smooth_frame(w, h, seed)
    f[..., 3] = (f[..., 0].astype(np.int64) * 3 // 4 + 17).astype(np.uint8)
    return f


def flat(w, h, v):
    return np.full((h, w, 4), v, dtype=np.uint8)


def ties(w, h, seed):
    """exact .5 ties of an exact 2:1 draw: every 2 x 2 block's four values sum to 4 q + 2, so the box mean is q + 0.5, with q even in
    half of the blocks (rounds down to q) and odd in the others (rounds up to q + 1) — per channel, parities mixed.  w, h even."""
    assert w % 2 == 0 and h % 2 == 0
    r = (synth.lcg_stream(seed, w * h) >> np.uint32(20)).astype(np.int64).reshape(h // 2, w // 2, 4)
    q = 1 + r % 253                                 # 1 .. 253: q - 1 .. q + 2 stay inside a byte
    out = np.empty((h, w, 4), dtype=np.uint8)
    kind = (r >> 9) & 1
    # block values (q, q / q + 1, q + 1) or (q - 1, q + 2 / q, q + 1): sums 4 q + 2 either way
    out[0::2, 0::2] = np.where(kind == 0, q, q - 1)
    out[0::2, 1::2] = np.where(kind == 0, q, q + 2)
    out[1::2, 0::2] = np.where(kind == 0, q + 1, q)
    out[1::2, 1::2] = q + 1
    return out


def frames_of(family, w, h, n, seed=1):
    if family == "noise":
        return np.stack([noise(w, h, seed + 10 * k) for k in range(n)])
    if family == "smooth":
        return np.stack([smooth(w, h, seed + 10 * k) for k in range(n)])
    if family == "zeros":
        return np.stack([flat(w, h, 0)] * n)
    if family == "ones":
        return np.stack([flat(w, h, 255)] * n)
    if family == "ties":
        return np.stack([ties(w, h, seed + 10 * k) for k in range(n)])
    raise ValueError(family)


# ---- ratio families: (source w, h) -> (canvas w, h) -------------------------------------------------------------------------------------

RATIOS = [
    ((97, 81), (97, 81)),          # 1 : 1 (the declared exact copy)
    ((320, 240), (320, 240)),
    ((194, 162), (97, 81)),        # exact 2 : 1
    ((291, 243), (97, 81)),        # exact 3 : 1
    ((388, 324), (97, 81)),        # exact 4 : 1
    ((1920, 1080), (320, 240)),    # the sizes the path exists for
    ((1280, 720), (320, 240)),
    ((640, 480), (320, 240)),
    ((333, 217), (97, 81)),
    ((333, 217), (160, 120)),
    ((511, 97), (131, 99)),        # anisotropic: down in x, up in y
    ((160, 120), (320, 240)),      # upscales
    ((23, 23), (40, 30)),
    ((1, 57), (40, 30)),           # degenerate sources: one column, one row, one pixel
    ((61, 1), (40, 30)),
    ((1, 1), (40, 30)),
    ((333, 217), (1, 120)),        # 1-pixel-wide / 1-pixel-high canvases
    ((333, 217), (160, 1)),
]

# small ones for the CPU cross-checks through node (every family of the list above, at sizes a scalar JS loop does in milliseconds)
CPU_RATIOS = [r for r in RATIOS if r[0][0] * r[0][1] <= 400 * 400]


def rects_for(sw, sh):
    """odd origins and rects touching every edge and corner of a sw x sh source frame (clipped to sizes that exist)"""
    w2, h2 = max(sw // 2, 1), max(sh // 2, 1)
    cand = [(0, 0, w2, h2), (sw - w2, 0, w2, h2), (0, sh - h2, w2, h2), (sw - w2, sh - h2, w2, h2),       # corners
            (1, 1, sw - 2, sh - 2), (3, 5, sw - 7, sh - 9), (sw - 1, sh - 1, 1, 1), (0, sh // 3, sw, 1), (sw // 3, 0, 1, sh),
            (7, 0, sw - 7, sh), (0, 9, sw, sh - 9), (5, 3, 2, 2)]
    return [r for r in cand if r[0] >= 0 and r[1] >= 0 and r[2] > 0 and r[3] > 0 and r[0] + r[2] <= sw and r[1] + r[3] <= sh]


def outside_filled(frame, rect, seed):
    """the frame with everything OUTSIDE rect replaced by another pattern: a draw of `rect` that clamps to the rect gives the same
    bytes from both; one that clamps to the frame does not"""
    x, y, w, h = rect
    out = 255 - noise(frame.shape[1], frame.shape[0], seed)
    out[y:y + h, x:x + w] = frame[y:y + h, x:x + w]
    return out


# ---- the reference's recorded canvases (tests/golden/ingest.json, written by tests/golden/make_ingest_golden.py) ---------------------------

def golden():
    with open(os.path.join(GOLDEN, "ingest.json")) as f:
        return json.load(f)


def golden_video(case, k):
    """video frame k of a golden case, rebuilt from its generator spec"""
    return synth.make(case["gen"][k], case["vw"], case["vh"])
