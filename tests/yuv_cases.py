"""Inputs and expectations of the YUV ingest (ht_draw_frames_yuv / ht_draw_frames_yuv_device), shared by tests/test_ingest_yuv_cpu.py
and tests/test_gpu_ingest_yuv.py.  The reference has no YUV path, so the conversion is DECLARED (headtrackr_amd/csrc/ht_yuv_plan.h); this
file restates it in numpy, independently of the header (vectorised int32, >> 8, np.clip): the CPU tests pin the header to this
restatement over all 2^24 triples.  The expectation of a draw is the declared conversion followed by the oracle's resampler:
ingest_cases.expected(to_rgba(...), rect, dw, dh).  Everything is seeded; nothing is read from outside the tree."""
import numpy as np

import ingest_cases as ic
from headtrackr_amd import synth

NV12, I420 = 0, 1
FORMATS = {"nv12": NV12, "i420": I420}
MATRIX_NAMES = ["bt601", "bt709", "bt601-full", "bt709-full"]
# matrix -> (yoff, cy, crv, cgu, cgv, cbu)
TABLE = {
    0: (16, 298, 409, -100, -208, 516),
    1: (16, 298, 459, -55, -136, 541),
    2: (0, 256, 359, -88, -183, 454),
    3: (0, 256, 403, -48, -120, 475),
}
# the exact matrices the tables approximate: (Kr, Kb, limited range?)
EXACT = {0: (0.299, 0.114, True), 1: (0.2126, 0.0722, True), 2: (0.299, 0.114, False), 3: (0.2126, 0.0722, False)}
EXTREME_VALUES = (0, 16, 128, 235, 240, 255)


def chroma_dims(w, h):
    return (w + 1) // 2, (h + 1) // 2


def frame_bytes(w, h):
    cw, ch = chroma_dims(w, h)
    return w * h + 2 * cw * ch


def convert_unclamped(y, u, v, matrix):
    """the declared integer formula before the clamp: int32 arrays (R, G, B)"""
    yoff, cy, crv, cgu, cgv, cbu = TABLE[matrix]
    c = (np.asarray(y, dtype=np.int32) - yoff) * np.int32(cy)
    d = np.asarray(u, dtype=np.int32) - 128
    e = np.asarray(v, dtype=np.int32) - 128
    return (c + crv * e + 128) >> 8, (c + cgu * d + cgv * e + 128) >> 8, (c + cbu * d + 128) >> 8


def convert(y, u, v, matrix):
    """-> uint8 [..., 4] RGBA, A = 255"""
    r, g, b = convert_unclamped(y, u, v, matrix)
    out = np.empty(r.shape + (4,), dtype=np.uint8)
    for k, ch in enumerate((r, g, b)):
        out[..., k] = np.clip(ch, 0, 255)
    out[..., 3] = 255
    return out


def clamped_fraction(y, u, v, matrix):
    """fraction of pixels that clamp on at least one channel"""
    r, g, b = convert_unclamped(y, u, v, matrix)
    bad = np.zeros(r.shape, dtype=bool)
    for ch in (r, g, b):
        bad |= (ch < 0) | (ch > 255)
    return float(bad.mean())


def exact_rgb(y, u, v, matrix):
    """the exact ITU matrix in binary64, rounded (half away from zero is half up here: the clamp removes the negatives) and clamped"""
    kr, kb, limited = EXACT[matrix]
    kg = 1.0 - kr - kb
    y, u, v = (np.asarray(a, dtype=np.float64) for a in (y, u, v))
    if limited:
        yy, cb, cr = (y - 16.0) * (255.0 / 219.0), (u - 128.0) * (255.0 / 224.0), (v - 128.0) * (255.0 / 224.0)
    else:
        yy, cb, cr = y, u - 128.0, v - 128.0
    r = yy + 2.0 * (1.0 - kr) * cr
    g = yy - 2.0 * kb * (1.0 - kb) / kg * cb - 2.0 * kr * (1.0 - kr) / kg * cr
    b = yy + 2.0 * (1.0 - kb) * cb
    return [np.clip(np.floor(c + 0.5), 0, 255).astype(np.int32) for c in (r, g, b)]


# ---- planes of ONE frame: NV12 (y [h, w], uv [ch, cw, 2]); I420 (y, u [ch, cw], v [ch, cw]) --------------------------------------------------

def split(planes, fmt):
    """-> (y, u, v) with u, v [ch, cw]"""
    if fmt == NV12:
        y, uv = planes
        return y, uv[..., 0], uv[..., 1]
    return planes


def join(y, u, v, fmt):
    y, u, v = (np.ascontiguousarray(a, dtype=np.uint8) for a in (y, u, v))
    return (y, np.ascontiguousarray(np.stack([u, v], axis=-1))) if fmt == NV12 else (y, u, v)


def to_rgba(planes, w, h, fmt, matrix):
    """the declared conversion of one frame -> uint8 [h, w, 4]; chroma sample of pixel (x, y) = sample (x >> 1, y >> 1) of the frame"""
    y, u, v = split(planes, fmt)
    cw, ch = chroma_dims(w, h)
    assert y.shape == (h, w) and u.shape == (ch, cw) and v.shape == (ch, cw), (y.shape, u.shape, v.shape)
    iy, ix = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    return convert(y, u[iy, ix], v[iy, ix], matrix)


def pack(planes):
    """one frame tightly packed as the host form and the JavaScript layer take it: Y, then UV (NV12) or U, then V (I420)"""
    return np.concatenate([np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in planes])


def unpack(buf, w, h, fmt):
    cw, ch = chroma_dims(w, h)
    y = buf[:w * h].reshape(h, w)
    if fmt == NV12:
        return y, buf[w * h:w * h + 2 * cw * ch].reshape(ch, cw, 2)
    return y, buf[w * h:w * h + cw * ch].reshape(ch, cw), buf[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)


def expected(planes, w, h, fmt, matrix, rect, dw, dh):
    return ic.expected(to_rgba(planes, w, h, fmt, matrix), rect, dw, dh)


# ---- content --------------------------------------------------------------------------------------------------------------------------------

def from_rgb(rgba, fmt, matrix, margin=0):
    """forward RGB -> YUV 4:2:0 of an RGBA frame (only to make IN-GAMUT content: nothing is asserted about this direction).  The exact
    matrix in binary64, chroma = the mean over each 2 x 2 block (edge blocks of odd sizes: the pixels that exist), rounded.  margin:
    the RGB values are first compressed into [margin, 255 - margin], which leaves the subsampled chroma of noisy content headroom."""
    kr, kb, limited = EXACT[matrix]
    kg = 1.0 - kr - kb
    rgb = rgba[..., :3].astype(np.float64)
    rgb = margin + rgb * ((255.0 - 2 * margin) / 255.0)
    h, w = rgb.shape[:2]
    yy = kr * rgb[..., 0] + kg * rgb[..., 1] + kb * rgb[..., 2]
    cb, cr = (rgb[..., 2] - yy) / (2.0 * (1.0 - kb)), (rgb[..., 0] - yy) / (2.0 * (1.0 - kr))
    cw, ch = chroma_dims(w, h)

    def sub(p):
        s = np.add.reduceat(np.add.reduceat(p, np.arange(0, h, 2), axis=0), np.arange(0, w, 2), axis=1)
        cnt = np.add.reduceat(np.add.reduceat(np.ones((h, w)), np.arange(0, h, 2), axis=0), np.arange(0, w, 2), axis=1)
        return s / cnt

    cb, cr = sub(cb), sub(cr)
    if limited:
        yy, cb, cr = 16.0 + yy * (219.0 / 255.0), 128.0 + cb * (224.0 / 255.0), 128.0 + cr * (224.0 / 255.0)
    else:
        cb, cr = 128.0 + cb, 128.0 + cr
    q = [np.clip(np.floor(p + 0.5), 0, 255).astype(np.uint8) for p in (yy, cb, cr)]
    assert q[1].shape == (ch, cw)
    return join(q[0], q[1], q[2], fmt)


def from_rgb_frames(kind, w, h, n, fmt, matrix, seed=1):
    """n frames of family from_rgb: ingest_cases' smooth or noise content, forward-converted (noise with a margin of 40)"""
    rgba = ic.frames_of(kind, w, h, n, seed=seed)
    return [from_rgb(rgba[f], fmt, matrix, margin=40 if kind == "noise" else 0) for f in range(n)]


def raw_noise(w, h, fmt, seed):
    """random planes: most pixels are out of gamut and clamp"""
    cw, ch = chroma_dims(w, h)
    s = (synth.lcg_stream(seed, w * h + 2 * cw * ch) >> np.uint32(24)).astype(np.uint8)
    return join(s[:w * h].reshape(h, w), s[w * h:w * h + cw * ch].reshape(ch, cw), s[w * h + cw * ch:].reshape(ch, cw), fmt)


def extremes(w, h, fmt):
    """Y, U, V over {0, 16, 128, 235, 240, 255}^3: chroma sample k takes (U, V) combination k mod 36, and the pixels of its block take Y
    values that shift with k // 36, so that a frame of >= 216 full blocks holds every triple"""
    cw, ch = chroma_dims(w, h)
    vals = np.array(EXTREME_VALUES, dtype=np.uint8)
    k = np.arange(ch)[:, None] * cw + np.arange(cw)[None, :]
    u, v = vals[k % 6], vals[(k // 6) % 6]
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    kb = (yy >> 1) * cw + (xx >> 1)
    y = vals[((xx & 1) + 2 * (yy & 1) + kb // 36) % 6]
    return join(y, u, v, fmt)


def triples_of(planes, w, h, fmt):
    y, u, v = split(planes, fmt)
    iy, ix = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    return set(zip(y.reshape(-1).tolist(), u[iy, ix].reshape(-1).tolist(), v[iy, ix].reshape(-1).tolist()))


# ---- source rects ---------------------------------------------------------------------------------------------------------------------------

def chroma_span(rect):
    """the chroma samples a rect's pixels name: columns cx0 .. cx1 and rows cy0 .. cy1, inclusive.  The samples that straddle the rect's
    edge belong to both sides (siting is by FRAME coordinates), so the outside of a rect starts at the next whole sample."""
    x, y, w, h = rect
    return x >> 1, (x + w - 1) >> 1, y >> 1, (y + h - 1) >> 1


def outside_filled(planes, w, h, fmt, rect, seed):
    """the frame with everything OUTSIDE rect replaced: Y pixels outside the rect, chroma samples outside chroma_span(rect).  A draw of
    `rect` that clamps its taps to the rect (and sites chroma by the frame) gives the same bytes from both."""
    y, u, v = (a.copy() for a in split(planes, fmt))
    oy, ou, ov = (255 - a for a in split(raw_noise(w, h, fmt, seed), fmt))
    x0, y0, rw, rh = rect
    cx0, cx1, cy0, cy1 = chroma_span(rect)
    oy[y0:y0 + rh, x0:x0 + rw] = y[y0:y0 + rh, x0:x0 + rw]
    ou[cy0:cy1 + 1, cx0:cx1 + 1] = u[cy0:cy1 + 1, cx0:cx1 + 1]
    ov[cy0:cy1 + 1, cx0:cx1 + 1] = v[cy0:cy1 + 1, cx0:cx1 + 1]
    return join(oy, ou, ov, fmt)


def taps(d, s, origin):
    """numpy twin of rs_tap (ht_resample_tap.h) for a whole axis: destination size d, source extent s at `origin` -> (a, b), absolute"""
    r = np.float64(s) / np.float64(d)
    f = np.clip((np.arange(d, dtype=np.float64) + 0.5) * r - 0.5, 0.0, float(s - 1))
    a = np.floor(f).astype(np.int64)
    return origin + a, origin + np.minimum(a + 1, s - 1)


RECT_CASES = [((333, 217), (97, 81)), ((23, 23), (40, 30))]  # (source size, canvas size): the rects are ingest_cases.rects_for(source)
