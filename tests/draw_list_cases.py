"""Inputs and expectations of ht_draw_list_device (one launch draws a list of per-feed sources), shared by tests/test_draw_list_cpu.py and
tests/test_gpu_draw_list.py.  A source is one feed's frame: RGBA, NV12 or I420, with a size, pitches and a matrix of its own.  The
expectation of an entry never comes from the code under test: it is ingest_cases.expected on the RGBA frame (the oracle's resampler) or
yuv_cases.expected on the planes (the declared conversion, then the oracle's resampler).  Everything is seeded."""
import numpy as np

import ingest_cases as ic
import yuv_cases as yc

RGBA = 16  # HT_DRAW_RGBA
FORMAT_NAMES = {RGBA: "rgba", yc.NV12: "nv12", yc.I420: "i420"}
PAD, GUARD = 0x5A, 0xA5


class Source:
    """one feed's frame on the host.  pad0 / pad1: bytes added to the packed pitch of plane 0 / of the chroma plane(s)"""

    def __init__(self, fmt, w, h, seed, matrix=0, pad0=0, pad1=0, content="noise"):
        self.fmt, self.w, self.h, self.matrix, self.pad0, self.pad1 = fmt, w, h, matrix, pad0, pad1
        if fmt == RGBA:
            assert pad0 % 4 == 0
            self.rgba = ic.frames_of(content, w, h, 1, seed=seed)[0]
            self.planes = None
        else:
            assert fmt != yc.NV12 or pad1 % 2 == 0
            self.planes = yc.raw_noise(w, h, fmt, seed) if content == "raw" else yc.from_rgb_frames(content, w, h, 1, fmt, matrix, seed=seed)[0]
            self.rgba = yc.to_rgba(self.planes, w, h, fmt, matrix)

    def pitches(self):
        if self.fmt == RGBA:
            return 4 * self.w + self.pad0, 0
        cw, _ = yc.chroma_dims(self.w, self.h)
        return self.w + self.pad0, (2 * cw if self.fmt == yc.NV12 else cw) + self.pad1

    def plane_rows(self):
        """[(rows, row bytes, pitch, the plane's bytes [rows, row bytes])] in the order p0, p1, p2"""
        p0, p1 = self.pitches()
        if self.fmt == RGBA:
            return [(self.h, 4 * self.w, p0, self.rgba.reshape(self.h, 4 * self.w))]
        cw, ch = yc.chroma_dims(self.w, self.h)
        crow = 2 * cw if self.fmt == yc.NV12 else cw
        return [(self.h, self.w, p0, self.planes[0])] + [(ch, crow, p1, np.ascontiguousarray(p).reshape(ch, crow)) for p in self.planes[1:]]

    def plane_buffers(self):
        """every plane as it lies in its own allocation: rows at the pitch, the padding filled with 0x5A; the buffer ends with the last ROW"""
        out = []
        for rows, rowbytes, pitch, data in self.plane_rows():
            buf = np.full((rows - 1) * pitch + rowbytes, PAD, dtype=np.uint8)
            for r in range(rows):
                buf[r * pitch:r * pitch + rowbytes] = data[r]
            out.append(buf)
        return out

    def packed(self):
        """the frame tightly packed, as the JavaScript layer uploads one feed's frame: RGBA rows, or Y then UV / U, V"""
        return self.rgba.reshape(-1).copy() if self.fmt == RGBA else yc.pack(self.planes)

    def expected(self, rect, dw, dh):
        if self.fmt == RGBA:
            return ic.expected(self.rgba, rect, dw, dh)
        return yc.expected(self.planes, self.w, self.h, self.fmt, self.matrix, rect, dw, dh)

    def entry(self, ptrs, rect=None):
        """the api.Context.draw_list entry for this source with its planes at the device pointers ptrs"""
        p0, p1 = self.pitches()
        e = dict(format=self.fmt, width=self.w, height=self.h, matrix=self.matrix, pitch0=p0 if self.pad0 else 0, pitch1=p1 if self.pad1 else 0, rect=rect)
        for k, p in enumerate(ptrs):
            e[f"p{k}"] = p
        return e


def mixed_sources():
    """the seven sources of the mixed list, ordered so that neighbouring entries take different branches of the kernel, and the rect each is
    drawn under: RGBA, NV12, I420 (2 x 2: one chroma column), NV12 odd x odd, RGBA one pixel wide, I420 under a rect with an odd origin, NV12
    under a rect.  Every one has a size, pitch padding and matrix of its own."""
    big, small = (333, 217), (23, 23)
    return [
        (Source(RGBA, *big, seed=11, pad0=12), None),
        (Source(yc.NV12, *big, seed=12, matrix=1, pad0=13, pad1=6), None),
        (Source(yc.I420, 2, 2, seed=13, matrix=2, pad0=3, pad1=5, content="raw"), None),
        (Source(yc.NV12, *small, seed=14, matrix=3, pad0=1, pad1=2), None),
        (Source(RGBA, 1, 5, seed=15, pad0=8), None),
        (Source(yc.I420, *big, seed=16, matrix=0, pad0=7, pad1=9), ic.rects_for(*big)[5]),   # (3, 5, sw - 7, sh - 9): odd origin
        (Source(yc.NV12, *small, seed=17, matrix=2, pad0=5, pad1=4, content="raw"), ic.rects_for(*small)[4]),  # (1, 1, 21, 21): odd origin
    ]


def cycling_sources():
    """six 23 x 23 sources, two per format, for the lists that cycle the formats"""
    return [Source(fmt, 23, 23, seed=30 + k, matrix=k % 4, pad0=4 * (k % 3), pad1=2 * (k % 2), content="noise" if k % 2 else "smooth")
            for k, fmt in enumerate([RGBA, yc.NV12, yc.I420, yc.NV12, RGBA, yc.I420])]


def cycling_list(n):
    """n (source index, rect) pairs over cycling_sources(): neighbouring entries differ in format, every rect of rects_for appears"""
    rects = [None] + ic.rects_for(23, 23)
    return [(k % 6, rects[(k // 6 + k) % len(rects)]) for k in range(n)]


def extent_of(src):
    """numpy restatement of an entry's plane extents: a plane ends with its last row"""
    return [(rows - 1) * pitch + rowbytes for rows, rowbytes, pitch, _ in src.plane_rows()]
