"""Inputs and expectations of the face crops (ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device), shared by
tests/test_crop_cpu.py and tests/test_gpu_crop.py.  `rule` restates the crop rule in Python integers (written from the rule's description,
not from headtrackr_amd/csrc/ht_crop_plan.h); the sources are draw_list_cases.Source, so the expected patch of a rect is
Source.expected(rect, P, Q) — the oracle's resampler; the track objects of the scenes come from the oracle's camshift.  Nothing here
comes from the code under test, and everything is seeded."""
import functools
import math
import struct

import numpy as np

import draw_list_cases as dl
import pair_cases as pc
import yuv_cases as yc
from oracle import ht_oracle as ho

EMPTY, FACE = 0, 1
SQUARE = 1
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def floor_i32(v):
    """floor as int32, saturated; NaN -> 0"""
    if v != v:
        return 0
    if v >= 2147483647.0:
        return I32_MAX
    if v <= -2147483648.0:
        return I32_MIN
    return math.floor(v)


def ceildiv(a, b):
    return -((-a) // b)


def rule(obj, W, H, SW, SH, mapping, margin_q8, flags):
    """obj = (x, y, width, height) of the track object (x, y: the centre), canvas W x H, source SW x SH, mapping = (mx, my, mw, mh) or None
    -> (code, (l, t, w, h)).  Python's // rounds towards -inf and its integers do not overflow."""
    mx, my, mw, mh = mapping if mapping is not None and (mapping[2] or mapping[3]) else (0, 0, SW, SH)
    cx, cy, w, h = (floor_i32(v) for v in obj)
    if w <= 0 or h <= 0 or w > 65536 or h > 65536 or abs(cx) > 2 ** 20 or abs(cy) > 2 ** 20:
        return EMPTY, (0, 0, 0, 0)
    L, R = 512 * cx - w * margin_q8, 512 * cx + w * margin_q8
    T, B = 512 * cy - h * margin_q8, 512 * cy + h * margin_q8
    l, r = mx + (L * mw) // (512 * W), mx + ceildiv(R * mw, 512 * W)
    t, b = my + (T * mh) // (512 * H), my + ceildiv(B * mh, 512 * H)
    if flags & SQUARE:
        dw, dh = r - l, b - t
        if dw < dh:
            l -= (dh - dw) // 2
            r = l + dh
        elif dh < dw:
            t -= (dw - dh) // 2
            b = t + dw
    l, t, r, b = max(l, 0), max(t, 0), min(r, SW), min(b, SH)
    if r <= l or b <= t:
        return EMPTY, (0, 0, 0, 0)
    return FACE, (l, t, r - l, b - t)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def record(stream, obj, W, H, SW, SH, mapping, margin_q8, flags, P, Q):
    """the 40-byte record of an entry as a tuple (code, stream, x, y, width, height, rx bits, ry bits): Python's / is one binary64 division"""
    code, (l, t, w, h) = rule(obj, W, H, SW, SH, mapping, margin_q8, flags)
    rx, ry = (w / P, h / Q) if code == FACE else (0.0, 0.0)
    return (code, stream, l, t, w, h, f64_bits(rx), f64_bits(ry))


def patch(source, obj, W, H, mapping, margin_q8, flags, P, Q):
    """the expected patch uint8 [Q, P, 4] of a dl.Source under the rule: zeros when empty"""
    code, rect = rule(obj, W, H, source.w, source.h, mapping, margin_q8, flags)
    return source.expected(rect, P, Q) if code == FACE else np.zeros((Q, P, 4), dtype=np.uint8)


def obj_of(to):
    return (to["x"], to["y"], to["width"], to["height"])


# ---- the harness cases of the CPU test: (x, y, width, height, W, H, SW, SH, mx, my, mw, mh, margin_q8, flags) ------------------------------------

CASE = struct.Struct("<4d9iI2i")  # 80 bytes: tests/host/crop_plan_harness.cc
assert CASE.size == 80


def pack_cases(cases):
    return b"".join(CASE.pack(*[float(v) for v in c[:4]], *[int(v) for v in c[4:14]], 0, 0) for c in cases)


def want_of(case):
    code, rect = rule(case[:4], case[4], case[5], case[6], case[7], case[8:12], case[12], case[13])
    return (code, *rect)


def edge_cases():
    """the edge table.  Every geometry x margin x flag combination of the listed objects."""
    nan, inf = float("nan"), float("inf")
    geoms = [
        (97, 81, 97, 81, (0, 0, 97, 81)),            # the pairs form: the canvas is the source
        (97, 81, 333, 217, (0, 0, 0, 0)),            # whole source (width == height == 0)
        (97, 81, 333, 217, (3, 5, 326, 208)),        # odd-origin mapping rect
        (97, 81, 511, 97, (7, 1, 500, 95)),          # anamorphic: down in x, about 1:1 in y
        (97, 81, 23, 23, (1, 1, 21, 21)),            # the canvas upscales the source: boxes of 1-2 source pixels
        (320, 240, 1920, 1080, (0, 0, 1920, 1080)),  # the sizes the path exists for
        (320, 240, 1920, 1080, (241, 135, 1439, 811)),
        (97, 81, 1, 5, (0, 0, 1, 5)),                # a source one pixel wide
        (16384, 16384, 16384, 16384, (0, 0, 16384, 16384)),
        (1, 1, 16384, 16384, (0, 0, 16384, 16384)),  # the largest products the rule forms
        (1 << 21, 1 << 21, 16384, 16384, (0, 0, 16384, 16384)),  # a canvas on which a centre at 2^20 is inside: only the bound refuses 2^20 + 1
        (1 << 21, 1 << 21, 16384, 16384, (16000, 16000, 1, 1)),  # ... and one whose mapping rect has source pixels to its left: -2^20 is a face, -2^20 - 1 is not
    ]
    objs = [
        (nan, 10, 10, 10), (10, nan, 10, 10), (10, 10, nan, 10), (10, 10, 10, nan), (inf, 10, 10, 10), (-inf, 10, 10, 10), (10, inf, 10, 10), (10, 10, inf, 10),
        (10, 10, 10, -inf), (-5, -7, 10, 10), (10, 10, -3, 10), (10, 10, 10, -0.5), (0, 0, 0, 0), (48, 40, 0, 0), (48, 40, 0, 12), (48, 40, 12, 0),
        (48.9, 40.9, 0.99, 12), (48.9, 40.9, 1.0, 1.0),
        (48, 40, 65536, 10), (48, 40, 65537, 10), (48, 40, 10, 65536), (48, 40, 10, 65536.999), (48, 40, 10, 65537),
        (2 ** 20, 40, 10, 10), (2 ** 20 + 1, 40, 10, 10), (2 ** 20 + 0.5, 40, 10, 10), (-2 ** 20, 40, 10, 10), (-2 ** 20 - 0.5, 40, 10, 10), (-2 ** 20 - 1, 40, 10, 10),
        (48, 2 ** 20, 10, 10), (48, 2 ** 20 + 1, 10, 10), (48, -2 ** 20, 10, 10), (48, -2 ** 20 - 1, 10, 10), (2 ** 20, 2 ** 20, 65536, 65536), (-2 ** 20, -2 ** 20, 65536, 65536),
        (1e300, 1e300, 1e300, 1e300), (-1e300, 5, 5, 5), (2147483647.0, 0, 1, 1), (-2147483648.0, 0, 1, 1), (5e-324, 5e-324, 5e-324, 5e-324),
        # touching and crossing every edge of a 97 x 81 canvas
        (5, 40, 10, 10), (4, 40, 10, 10), (0, 40, 10, 10), (-4, 40, 10, 10), (-5, 40, 10, 10), (-6, 40, 10, 10),
        (92, 40, 10, 10), (93, 40, 10, 10), (97, 40, 10, 10), (101, 40, 10, 10), (102, 40, 10, 10), (103, 40, 10, 10),
        (48, 5, 10, 10), (48, 4, 10, 10), (48, 0, 10, 10), (48, -5, 10, 10), (48, -6, 10, 10),
        (48, 76, 10, 10), (48, 77, 10, 10), (48, 81, 10, 10), (48, 86, 10, 10), (48, 87, 10, 10),
        (48, 40, 200, 200), (48, 40, 97, 81), (48.5, 40.5, 97, 81), (0, 0, 1, 1), (96, 80, 1, 1), (97, 81, 1, 1), (96, 80, 2, 2),
        # results one pixel wide or high, tall and wide boxes for the square flag
        (48, 40, 1, 30), (48, 40, 30, 1), (48, 40, 1, 1), (0, 40, 1, 9), (96.999, 40, 1, 9), (48, 40, 3, 41), (48, 40, 41, 3), (47.25, 39.75, 18.7, 25.3), (300, 200, 64, 48),
    ]
    out = []
    for (W, H, SW, SH, m) in geoms:
        for o in objs:
            for margin in (64, 256, 1024, 65, 1023):
                for flags in (0, SQUARE):
                    out.append((*o, W, H, SW, SH, *m, margin, flags))
    return out


def random_cases(n, seed=20261):
    """n seeded objects on seeded geometries: centres around and beyond the canvas, boxes from a fraction of a pixel to several canvases"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        W, H = int(rng.randint(1, 2000)), int(rng.randint(1, 1200))
        SW, SH = int(rng.randint(1, 4000)), int(rng.randint(1, 2400))
        if rng.randint(4) == 0:
            m = (0, 0, 0, 0)
        else:
            mw, mh = int(rng.randint(1, SW + 1)), int(rng.randint(1, SH + 1))
            m = (int(rng.randint(0, SW - mw + 1)), int(rng.randint(0, SH - mh + 1)), mw, mh)
        scale = [0.05, 0.3, 1.0, 3.0][rng.randint(4)]
        o = (float(rng.uniform(-0.5, 1.5) * W), float(rng.uniform(-0.5, 1.5) * H), float(rng.uniform(-0.01, scale) * W), float(rng.uniform(-0.01, scale) * H))
        if rng.randint(8) == 0:
            o = tuple(float(math.floor(v)) for v in o)  # integer-valued objects: the divisions come out exact more often
        out.append((*o, W, H, SW, SH, *m, int(rng.randint(64, 1025)), int(rng.randint(2))))
    return out


# ---- scenes: blobs the oracle's camshift tracks, on canvases and in the feeds' own frames --------------------------------------------------

CANVAS = (97, 81)
COLORS = [(200, 60, 40), (40, 180, 220), (230, 210, 50), (150, 60, 200)]
CONFIGS = [(64, 0), (256, 0), (1024, 0), (64, SQUARE), (256, SQUARE), (1024, SQUARE)]  # (margin_q8, flags)
SIZES = [(70, 19), (1, 1), (112, 112)]                                                     # (P, Q): partial tiles both ways, one pixel, the embedder's size


@functools.lru_cache(maxsize=None)
def pairs_scene(calls=2):
    """two bound 97 x 81 canvases: frame 0 carries two blobs (near the top-left and the bottom-right corner, so that a wide margin
    clamps on all four sides), frame 1 one tall blob in the middle.  frames[0] initialise, frames[k] are the k-th step (the blobs move)."""
    W, H = CANVAS
    a = pc.MultiSeq("crop-a", W, H, [[(14 + k, 12 + k, 9, 7, (4, 3, 5), COLORS[0]), (80 - k, 66 - 2 * k, 8, 10, (1, 0, 1), COLORS[1])] for k in range(calls + 1)],
                    [7100 + k for k in range(calls + 1)])
    b = pc.MultiSeq("crop-b", W, H, [[(50 + 2 * k, 40 - k, 6, 15, (0, 1, 1), COLORS[2])] for k in range(calls + 1)], [7200 + k for k in range(calls + 1)])
    return a, b


def pairs_trackers():
    """(stream, bound frame, sequence index, tracker of that sequence): streams scattered through a reservation of 6; stream 4 is
    initialised on frame 1 and never tracked, stream 3 stays untouched"""
    return [(5, 0, 0, 0), (0, 0, 0, 1), (2, 1, 1, 0)]


NEVER_TRACKED, RESERVED = 4, 6


class BlobSource(dl.Source):
    """a dl.Source whose picture is a synth blob frame: RGBA as it is, YUV forward-converted (only to make content: the expectation is
    the declared conversion of the planes, as for every Source).  `share`: a BlobSource whose planes this one re-reads under another matrix"""

    def __init__(self, fmt, w, h, blobs, seed, matrix=0, pad0=0, pad1=0, share=None, pic=None):
        self.fmt, self.w, self.h, self.matrix, self.pad0, self.pad1 = fmt, w, h, matrix, pad0, pad1
        self.share = share
        if share is not None:
            assert (share.fmt, share.w, share.h, share.pad0, share.pad1) == (fmt, w, h, pad0, pad1) and fmt != dl.RGBA
            self.planes = share.planes
            self.rgba = yc.to_rgba(self.planes, w, h, fmt, matrix)
            return
        if pic is None:
            pic = pc.multi_blob_frame(w, h, blobs, seed)
        assert pic.shape == (h, w, 4)
        if fmt == dl.RGBA:
            self.rgba, self.planes = pic, None
        else:
            self.planes = yc.from_rgb(pic, fmt, matrix, margin=40 if blobs else 0)
            self.rgba = yc.to_rgba(self.planes, w, h, fmt, matrix)


def strip_picture():
    """1 x 5: five rows of one pixel each.  On the canvas they are horizontal bands; a tracker on the middle band gives rects one pixel wide"""
    pic = np.zeros((5, 1, 4), dtype=np.uint8)
    pic[:, 0, :3] = [(90, 100, 110), (120, 90, 70), (200, 60, 40), (60, 130, 90), (100, 100, 140)]
    pic[..., 3] = 255
    return pic


STRIP_RECT = (20, 26, 50, 28)  # initTracker on the canvas of a strip feed: the middle band


@functools.lru_cache(maxsize=None)
def feeds():
    """[(source, mapping rect or None)]: a padded RGBA 333 x 217; an NV12 333 x 217 under an odd-origin mapping rect; an I420 23 x 23, which
    the canvas upscales (boxes of 2-3 source pixels); the NV12 allocation again under another rect and matrix; the I420 allocation again
    under the fourth matrix; an RGBA and an NV12 source ONE pixel wide (no tap pair, a single chroma column).  The blob of entry 1 lies
    near the edge of its mapping rect: a wide margin reaches beyond the rect, into source pixels that were never drawn."""
    big, small = (333, 217), (23, 23)
    rgba = BlobSource(dl.RGBA, *big, [(60, 170, 34, 26, (4, 3, 5), COLORS[0])], 7301, pad0=12)
    nv12 = BlobSource(yc.NV12, *big, [(290, 50, 30, 36, (1, 0, 1), COLORS[1]), (70, 150, 28, 22, (0, 1, 1), COLORS[3])], 7302, matrix=1, pad0=13, pad1=6)
    i420 = BlobSource(yc.I420, *small, [(15, 9, 2, 3, (4, 3, 5), COLORS[0])], 7303, matrix=2, pad0=7, pad1=9)
    nv12b = BlobSource(yc.NV12, *big, None, 0, matrix=3, pad0=13, pad1=6, share=nv12)
    i420b = BlobSource(yc.I420, *small, None, 0, matrix=0, pad0=7, pad1=9, share=i420)
    strip = BlobSource(dl.RGBA, 1, 5, None, 0, pad0=8, pic=strip_picture())
    strip_nv = BlobSource(yc.NV12, 1, 5, None, 0, matrix=2, pad0=3, pad1=2, pic=strip_picture())
    return [(rgba, None), (nv12, (3, 5, 326, 208)), (i420, None), (nv12b, (11, 61, 200, 150)), (i420b, (1, 1, 21, 21)), (strip, None), (strip_nv, None)]


# (cx, cy, a, b) in SOURCE pixels of the blob each entry tracks; None: a strip feed
FEED_BLOB = [(60, 170, 34, 26), (290, 50, 30, 36), (15, 9, 2, 3), (70, 150, 28, 22), (15, 9, 2, 3), None, None]


def canvas_of(k):
    src, m = feeds()[k]
    return src.expected(m, *CANVAS)


def canvas_rect_of(k):
    """the tracked blob's bounding rect on the canvas (floats floored / ceiled outwards, clipped): what initTracker gets"""
    src, m = feeds()[k]
    if FEED_BLOB[k] is None:
        return STRIP_RECT
    mx, my, mw, mh = m if m else (0, 0, src.w, src.h)
    cx, cy, a, b = FEED_BLOB[k]
    W, H = CANVAS
    x0, x1 = math.floor((cx - a - mx) * W / mw), math.ceil((cx + a - mx) * W / mw)
    y0, y1 = math.floor((cy - b - my) * H / mh), math.ceil((cy + b - my) * H / mh)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    return (x0, y0, x1 - x0, y1 - y0)


@functools.lru_cache(maxsize=None)
def feed_objects():
    """per feed: the oracle's track object after initTracker on the feed's canvas and one track() on the same canvas"""
    out = []
    for k in range(len(feeds())):
        o = ho.Camshift(True)
        c = canvas_of(k)
        o.init_tracker(c, canvas_rect_of(k))
        _sw, to = o.track(c)
        out.append(to)
    return out


def classify(rects_and_sources, P, Q):
    """what a list of (code, rect, SW, SH) covers: the sides a crop touches, one-pixel-wide rects, up- and downscales"""
    seen = set()
    for code, (l, t, w, h), SW, SH in rects_and_sources:
        if code != FACE:
            seen.add("empty")
            continue
        seen |= {name for name, hit in (("left", l == 0), ("top", t == 0), ("right", l + w == SW), ("bottom", t + h == SH), ("one-wide", w == 1), ("one-high", h == 1),
                                        ("up", w < P or h < Q), ("down", w > P or h > Q)) if hit}
    return seen
