"""Inputs and expectations of the packed 4:2:2 ingest (HT_YUV_YUYV / HT_YUV_UYVY through the draw calls and the face-patch calls), shared by
tests/test_ingest_422_cpu.py and tests/test_gpu_ingest_422.py.  The rule is DECLARED (include/headtrackr_hip.h, csrc/ht_yuv_plan.h) and
restated here in numpy, independently of the header: a frame is ONE plane, row y holds cw = ceil(w / 2) macropixels of 4 bytes — YUYV
Y(2m) U(m) Y(2m+1) V(m), UYVY U(m) Y(2m) V(m) Y(2m+1) —; pixel (x, y) takes its own Y byte and the U and V of macropixel (x >> 1) of ROW y
of the frame; the triple goes through yuv_cases.convert (the declared integer matrices).  The expectation of a draw is that conversion
followed by the oracle's resampler, exactly as yuv_cases.expected builds it.  Everything is seeded; nothing is read from outside the tree."""
import numpy as np

import ingest_cases as ic
import yuv_cases as yc
from headtrackr_amd import synth

YUYV, UYVY = 4, 5
FORMATS = {"yuyv": YUYV, "uyvy": UYVY}
FORMAT_NAMES = {YUYV: "yuyv", UYVY: "uyvy"}
# byte offsets inside a macropixel: (Y0, U, Y1, V)
OFFSETS = {YUYV: (0, 1, 2, 3), UYVY: (1, 0, 3, 2)}
REFUSED_FORMATS = (-1, 2, 3, 6, 7, 15, 17)


def macropixels(w):
    return (w + 1) // 2


def frame_bytes(w, h):
    return 4 * macropixels(w) * h


def pack(y, u, v, fmt, spare=None):
    """y uint8 [h, w], u, v uint8 [h, cw] -> one frame uint8 [h, 4 cw].  An odd width leaves the last macropixel's second luma byte
    without a pixel: it is in memory and never selected, and holds `spare` [h] here (default: the complement of the row's last luma, so a
    read that selects it shows)."""
    y, u, v = (np.asarray(a, dtype=np.uint8) for a in (y, u, v))
    h, w = y.shape
    cw = macropixels(w)
    assert u.shape == (h, cw) and v.shape == (h, cw), (y.shape, u.shape, v.shape)
    y2 = np.empty((h, 2 * cw), dtype=np.uint8)
    y2[:, :w] = y
    if w & 1:
        y2[:, w] = (255 - y[:, w - 1]) if spare is None else spare
    o = OFFSETS[fmt]
    out = np.empty((h, cw, 4), dtype=np.uint8)
    out[..., o[0]], out[..., o[1]], out[..., o[2]], out[..., o[3]] = y2[:, 0::2], u, y2[:, 1::2], v
    return out.reshape(h, 4 * cw)


def unpack(frame, w, h, fmt):
    """-> (y [h, w], u [h, cw], v [h, cw])"""
    cw = macropixels(w)
    m = np.asarray(frame, dtype=np.uint8).reshape(h, cw, 4)
    o = OFFSETS[fmt]
    y2 = np.empty((h, 2 * cw), dtype=np.uint8)
    y2[:, 0::2], y2[:, 1::2] = m[..., o[0]], m[..., o[2]]
    return np.ascontiguousarray(y2[:, :w]), np.ascontiguousarray(m[..., o[1]]), np.ascontiguousarray(m[..., o[3]])


def to_rgba(frame, w, h, fmt, matrix):
    """the declared conversion of one frame -> uint8 [h, w, 4]; chroma of pixel (x, y) = macropixel (x >> 1) of row y of the frame"""
    y, u, v = unpack(frame, w, h, fmt)
    ix = np.arange(w) >> 1
    return yc.convert(y, u[:, ix], v[:, ix], matrix)


def expected(frame, w, h, fmt, matrix, rect, dw, dh):
    return ic.expected(to_rgba(frame, w, h, fmt, matrix), rect, dw, dh)


def from_i420(planes, fmt):
    """the 4:2:2 frame with each chroma row of the I420 frame written twice (the last one once where the height is odd)"""
    y, u, v = planes
    iy = np.arange(y.shape[0]) >> 1
    return pack(y, u[iy], v[iy], fmt)


def clamped_fraction(frame, w, h, fmt, matrix):
    y, u, v = unpack(frame, w, h, fmt)
    ix = np.arange(w) >> 1
    return yc.clamped_fraction(y, u[:, ix], v[:, ix], matrix)


# ---- content --------------------------------------------------------------------------------------------------------------------------------

def raw_noise(w, h, fmt, seed):
    """every byte of the frame random, the spare luma byte of an odd width included: most pixels are out of gamut and clamp"""
    n = frame_bytes(w, h)
    return (synth.lcg_stream(seed, n) >> np.uint32(24)).astype(np.uint8).reshape(h, 4 * macropixels(w))


def extremes(w, h, fmt):
    """yuv_cases.extremes (Y, U, V over {0, 16, 128, 235, 240, 255}^3) with its chroma rows doubled"""
    return from_i420(yc.extremes(w, h, yc.I420), fmt)


def from_rgb(rgba, fmt, matrix, margin=0):
    """forward RGB -> YUV 4:2:2 of an RGBA frame (only to make IN-GAMUT content whose chroma differs from row to row: nothing is asserted
    about this direction).  yuv_cases.from_rgb's matrix in binary64 with the chroma averaged over each horizontal PAIR only."""
    kr, kb, limited = yc.EXACT[matrix]
    kg = 1.0 - kr - kb
    rgb = rgba[..., :3].astype(np.float64)
    rgb = margin + rgb * ((255.0 - 2 * margin) / 255.0)
    h, w = rgb.shape[:2]
    yy = kr * rgb[..., 0] + kg * rgb[..., 1] + kb * rgb[..., 2]
    cb, cr = (rgb[..., 2] - yy) / (2.0 * (1.0 - kb)), (rgb[..., 0] - yy) / (2.0 * (1.0 - kr))
    cols = np.arange(0, w, 2)
    cnt = np.add.reduceat(np.ones(w), cols)
    cb, cr = np.add.reduceat(cb, cols, axis=1) / cnt, np.add.reduceat(cr, cols, axis=1) / cnt
    if limited:
        yy, cb, cr = 16.0 + yy * (219.0 / 255.0), 128.0 + cb * (224.0 / 255.0), 128.0 + cr * (224.0 / 255.0)
    else:
        cb, cr = 128.0 + cb, 128.0 + cr
    q = [np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8) for p in (yy, cb, cr)]
    return pack(q[0], q[1], q[2], fmt)


def from_rgb_frames(kind, w, h, n, fmt, matrix, seed=1):
    """n frames of ingest_cases' smooth or noise content, forward-converted (noise with a margin of 40, as yuv_cases does)"""
    rgba = ic.frames_of(kind, w, h, n, seed=seed)
    return [from_rgb(rgba[f], fmt, matrix, margin=40 if kind == "noise" else 0) for f in range(n)]


# ---- the GPU case list (tests/test_gpu_ingest_422.py draws it; tests/test_ingest_422_cpu.py proves from this file alone that it reaches
# every path of the pixel body) -------------------------------------------------------------------------------------------------------------

class Case:
    """one row: n source frames of w x h drawn onto a dw x dh canvas under each of `rects` (None = the whole frame).  pitch_pad: bytes
    added to the packed pitch 4 cw; base_off: the plane starts that many bytes into its allocation; gap: bytes between frames"""

    def __init__(self, name, src, canvas, rects=(None,), n=1, pitch_pad=0, base_off=0, gap=0):
        self.name, (self.w, self.h), (self.dw, self.dh), self.rects, self.n = name, src, canvas, list(rects), n
        self.pitch_pad, self.base_off, self.gap = pitch_pad, base_off, gap
        self.cw = macropixels(self.w)
        assert pitch_pad % 4 == 0 and base_off % 4 == 0 and gap % 4 == 0

    @property
    def pitch(self):
        return 4 * self.cw + self.pitch_pad

    @property
    def extent(self):
        return self.pitch * (self.h - 1) + 4 * self.cw

    @property
    def stride(self):
        return self.extent + self.gap


CASES = [
    Case("97x81-rects", (97, 81), (64, 48), rects=[None] + ic.rects_for(97, 81)),
    Case("23x23-upscale", (23, 23), (40, 30)),
    Case("333x217-pitched", (333, 217), (320, 240), pitch_pad=12, base_off=4),
    Case("2x2", (2, 2), (8, 8)),
    Case("1x5", (1, 5), (8, 8)),
    Case("2x1", (2, 1), (8, 8)),
    Case("97x81-n3", (97, 81), (65, 17), n=3, gap=4 * 37),
]
TILE_W, TILE_H = 64, 16  # the draw kernels' tile
TILE_H_DRAWN = 4        # ... and the rows of the filtered draw's other tile (the packed draws take the 64 x 16 form, k_draw_list_mean_tile<4>)


def column_taps(case, rect):
    """(a, b) of every canvas column of `case` drawn under `rect`: absolute source columns"""
    x, _y, w, _h = (0, 0, case.w, case.h) if rect is None else rect
    return yc.taps(case.dw, w, x)


def sufficiency(cases=None):
    """what the case list exercises, counted from the restatement alone"""
    cnt = dict.fromkeys(("a_even", "a_odd", "b_same_macropixel", "b_next_macropixel", "last_column_even", "last_column_odd", "cw_1", "sw_1",
                         "tiles_cut_by_column_edge", "tiles_cut_by_row_edge", "tiles_cut_by_the_4_row_edge", "canvases_of_several_4_row_tiles"), 0)
    for c in CASES if cases is None else cases:
        cnt["cw_1"] += c.cw == 1
        cnt["tiles_cut_by_column_edge"] += (c.dw % TILE_W != 0) * ((c.dh + TILE_H - 1) // TILE_H)
        cnt["tiles_cut_by_row_edge"] += (c.dh % TILE_H != 0) * ((c.dw + TILE_W - 1) // TILE_W)
        cnt["tiles_cut_by_the_4_row_edge"] += (c.dh % TILE_H_DRAWN != 0) * ((c.dw + TILE_W - 1) // TILE_W)
        cnt["canvases_of_several_4_row_tiles"] += c.dh > TILE_H_DRAWN
        for rect in c.rects:
            x, _y, w, _h = (0, 0, c.w, c.h) if rect is None else rect
            a, b = column_taps(c, rect)
            last = x + w - 1
            cnt["sw_1"] += w == 1
            cnt["a_even"] += int((a % 2 == 0).sum())
            cnt["a_odd"] += int((a % 2 == 1).sum())
            cnt["b_same_macropixel"] += int(((b >> 1) == (a >> 1)).sum())
            cnt["b_next_macropixel"] += int(((b >> 1) == (a >> 1) + 1).sum())
            assert (((b >> 1) - (a >> 1)) <= 1).all() and (b >= a).all()
            cnt["last_column_even" if last % 2 == 0 else "last_column_odd"] += int((a == last).sum())
    return cnt
