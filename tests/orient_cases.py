"""Inputs and expectations of the oriented ingest (rotated and mirrored feeds: an orientation 0..7 in bits 8..10 of a source's format),
shared by tests/test_orient_cpu.py and tests/test_gpu_orient.py.  The rule is DECLARED (include/headtrackr_hip.h, csrc/ht_orient_plan.h)
and restated here in numpy, independently of the header: rot = k & 3 quarter turns clockwise bring the stored frame upright, flip = k >> 2
mirrors it horizontally after the turn, i.e. np.rot90(stored, -rot) and then np.fliplr.  The expectation of every call on an oriented
source is the expectation of the same call on the RGBA frame orient(convert(stored), k); it never comes from the code under test.
Everything is seeded; nothing is read from outside the tree."""
import numpy as np

import draw_list_cases as dl
import ingest_cases as ic
import yuv422_cases as y4
import yuv_cases as yc

ORIENTATIONS = tuple(range(8))
FORMATS = (dl.RGBA, yc.NV12, yc.I420, y4.YUYV, y4.UYVY)
FORMAT_NAMES = {dl.RGBA: "rgba", yc.NV12: "nv12", yc.I420: "i420", y4.YUYV: "yuyv", y4.UYVY: "uyvy"}
EXIF = {1: 0, 2: 4, 3: 2, 4: 6, 5: 5, 6: 1, 7: 7, 8: 3}  # what the issue states; tests/test_orient_cpu.py derives it again from numpy
MAPPING_SIZES = [(1, 1), (1, 5), (2, 2), (23, 23), (37, 22), (333, 217)]


def orient(frame, k):
    """the oriented frame O of a stored frame [h, w, ...]"""
    out = np.rot90(frame, -(k & 3))
    if k >> 2:
        out = np.fliplr(out)
    return np.ascontiguousarray(out)


def oriented_size(k, w, h):
    return (h, w) if k & 1 else (w, h)


def mapping(k, w, h, x, y):
    """the formula of the header, restated: O(x, y) = S(u, v) -> (u, v).  x, y may be arrays"""
    ow, _ = oriented_size(k, w, h)
    xp = ow - 1 - x if k >> 2 else x
    return [(xp, y), (y, h - 1 - xp), (w - 1 - xp, h - 1 - y), (w - 1 - y, xp)][k & 3]


def fmt_code(fmt, k):
    return fmt | (k << 8)


class PackedSource:
    """draw_list_cases.Source for the packed 4:2:2 formats: one plane of macropixels"""

    def __init__(self, fmt, w, h, seed, matrix=0, pad0=0, content="noise"):
        assert pad0 % 4 == 0
        self.fmt, self.w, self.h, self.matrix, self.pad0, self.pad1 = fmt, w, h, matrix, pad0, 0
        self.frame = y4.raw_noise(w, h, fmt, seed) if content == "raw" else y4.from_rgb_frames(content, w, h, 1, fmt, matrix, seed=seed)[0]
        self.rgba = y4.to_rgba(self.frame, w, h, fmt, matrix)

    def pitches(self):
        return 4 * y4.macropixels(self.w) + self.pad0, 0

    def plane_buffers(self):
        pitch, row = self.pitches()[0], 4 * y4.macropixels(self.w)
        buf = np.full((self.h - 1) * pitch + row, dl.PAD, dtype=np.uint8)
        for r in range(self.h):
            buf[r * pitch:r * pitch + row] = self.frame[r]
        return [buf]

    def packed(self):
        return self.frame.reshape(-1).copy()

    def entry(self, ptrs, rect=None):
        return dict(format=self.fmt, width=self.w, height=self.h, matrix=self.matrix, pitch0=self.pitches()[0] if self.pad0 else 0, rect=rect, p0=ptrs[0])


def source(fmt, w, h, seed, matrix=0, pad0=0, pad1=0, content="noise"):
    """a stored frame of any of the five formats; .rgba is the declared conversion of it"""
    if fmt in (y4.YUYV, y4.UYVY):
        return PackedSource(fmt, w, h, seed, matrix=matrix, pad0=pad0, content=content)
    return dl.Source(fmt, w, h, seed, matrix=matrix, pad0=pad0, pad1=pad1, content=content)


def entry(src, ptrs, k, rect=None):
    """the api.Context.draw_list entry of a stored source under orientation k; rect is in O's coordinates"""
    e = src.entry(ptrs, rect)
    e["orientation"] = k
    return e


def expected(src, k, rect, dw, dh):
    return ic.expected(orient(src.rgba, k), rect, dw, dh)


def odd_origin_rect(k, w, h):
    """a rect of O with an odd origin that reaches O's far edges: (1, 1, ow - 1, oh - 1), or None where O is too small for one"""
    ow, oh = oriented_size(k, w, h)
    return (1, 1, ow - 1, oh - 1) if ow >= 2 and oh >= 2 else None


def list_of_40():
    """5 formats x 8 orientations of 37 x 23 sources (odd x odd: the last chroma column and row and YUYV's half macropixel), every source
    with a pitch padding and a matrix of its own, every other entry under an odd-origin rect in O's coordinates; then a 2 x 2 I420 and a
    1 x 5 RGBA source under all eight orientations.  -> [(source, k, rect)]"""
    out = []
    for f, fmt in enumerate(FORMATS):
        for k in ORIENTATIONS:
            i = 8 * f + k
            pad0 = 4 * (i % 4) if fmt in (dl.RGBA, y4.YUYV, y4.UYVY) else i % 5
            s = source(fmt, 37, 23, seed=100 + i, matrix=i % 4, pad0=pad0, pad1=2 * (i % 3), content="raw" if i % 3 == 0 and fmt != dl.RGBA else "noise")
            out.append((s, k, odd_origin_rect(k, 37, 23) if (i + f) % 2 else None))
    tiny = source(yc.I420, 2, 2, seed=150, matrix=2, pad0=3, pad1=5, content="raw")
    line = source(dl.RGBA, 1, 5, seed=151, pad0=8)
    out += [(tiny, k, None) for k in ORIENTATIONS] + [(line, k, None) for k in ORIENTATIONS]
    return out
