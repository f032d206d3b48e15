"""Geometries at the 16384-pixel limits of ht_set_geometry, their frames and the oracle's answers on them (tests/test_limit_cases_cpu.py,
tests/test_gpu_limits.py).  A plain module, imported like tests/pyramid_cases.py.  Nothing here runs the library.

The geometries are the smallest frames that still reach the limits of the packed layouts:
  wide      16384 x 64     W % 4 == 0 (k_gray_linear), 256 resample tile columns (bx 0 .. 255), scale 0 has qw = 4090 window columns;
                           levels thousands of pixels wide and 1 .. 3 high, variant canvases on which nothing is drawn (dh = D.h - 2 <= 0)
  wide_odd  16383 x 97     k_gray_rows, the stride differs from the width on every level
  tall      65 x 16384     k_gray_rows with 4096 row groups, pass0 up to 1023, scan tile origins Y0 near 8180
  area      4099 x 2051    both dimensions beyond everything else in the suite, level 0 beyond 2^23 bytes, frame 1 of the arena beyond 2^25

Two more strips carry the pyramid tests only (THIN): a plane at most 3 pixels across is at most 912 long on 16384 x 64 (the aspect ratio is
256, so a level 3 rows high is 3 * 256 + 255 columns wide at the most), which keeps the undrawn variant canvases (dh = D.h - 2 <= 0) at 12 tile
columns.  On 16384 x 32 and 33 x 16384 they are up to 1824 long: levels 21 .. 24 are 1448 .. 1024 x 2, their slots 2 and 3 draw nothing.

Every batch has frames of different content, so frame 1 (one arena_stride in) cannot pass on frame 0's bytes.  Everything is seeded and
cached; the arrays handed out are read-only."""
import functools

import numpy as np

import pyramid_cases as pc
from headtrackr_amd import synth
from headtrackr_amd.cascade import load_cascade
from oracle import ht_oracle as ho

LIMIT = 16384
GEOMETRIES = {"wide": (16384, 64), "wide_odd": (16383, 97), "tall": (65, 16384), "area": (4099, 2051)}
STRIPS = ("wide", "wide_odd", "tall")
THIN = {"thin": (16384, 32), "thin_tall": (33, 16384)}  # pyramid only
SIZES = dict(GEOMETRIES, **THIN)

# faces (x, y, size) of frame F0: at the far edges, at the origin and near the middle
_WIDE_FACES = [(16356, 20, 24), (16344, 2, 32), (16240, 4, 56), (8, 4, 56), (8190, 2, 48), (4, 30, 24)]
FACES = {
    "wide": _WIDE_FACES,
    "wide_odd": [(16355, 60, 24), (16343, 2, 32), (16239, 4, 88), (8, 4, 88), (8190, 20, 48), (4, 70, 24)],
    "tall": [(min(y, 65 - s), x, s) for (x, y, s) in _WIDE_FACES],  # the wide faces with x and y exchanged
    "area": [(4071, 2023, 24), (3899, 1871, 160), (8, 4, 200), (2000, 1000, 360), (4, 2020, 24), (4060, 6, 32)],
    "thin": [(16356, 4, 24), (8, 2, 28), (8190, 0, 32)],
    "thin_tall": [(4, 16356, 24), (2, 8, 28), (0, 8190, 32)],
}

HIT_DTYPE = np.dtype([("frame", "<u4"), ("scale", "<i4"), ("q", "<i4"), ("y", "<i4"), ("x", "<i4"), ("sum", "<f8")])


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cascade():
    return load_cascade()


@functools.lru_cache(maxsize=None)
def face_frames(name):
    """the two frames of the hit tests: F0 = the faces on flat gray; F1 = the same faces mirrored along the long axis on a smooth frame, so
    that its deep-stage survivors lie all over the frame and its hits at the other end"""
    w, h = GEOMETRIES[name]
    f0 = synth.face_frame(w, h, FACES[name])
    f1 = synth.smooth_frame(w, h, 4)
    for (x, y, s) in FACES[name]:
        if h > w:
            synth.paste_face(f1, x, h - y - s, s)
        else:
            synth.paste_face(f1, w - x - s, y, s)
    return _frozen(np.stack([f0, f1]))


@functools.lru_cache(maxsize=None)
def pyramid_frames(name):
    """an N, an S and an F frame (F0 of face_frames), as tests/test_gpu_detect.py's _check_pyramid builds them"""
    w, h = SIZES[name]
    f0 = face_frames(name)[0] if name in GEOMETRIES else synth.face_frame(w, h, FACES[name])
    return _frozen(np.stack([synth.noise_frame(w, h, 3), synth.smooth_frame(w, h, 4), f0]))


@functools.lru_cache(maxsize=None)
def oracle_pyramid(name):
    """[(levels, arena)] of pyramid_frames(name)"""
    out = []
    for f in pyramid_frames(name):
        levels, arena = ho.pyramid(f)
        out.append((levels, _frozen(arena)))
    return out


@functools.lru_cache(maxsize=None)
def level_dims(name):
    return ho.pyramid_layout(*SIZES[name])


def windows(name, scale, interval=5):
    """(qw, qh) of a scale: the window counts per quarter phase, ccv.js:155-156"""
    lw, lh = level_dims(name)[scale + 2 * (interval + 1)]
    return lw - 6, lh - 6


@functools.lru_cache(maxsize=None)
def oracle_detect(name):
    """(raw hits of face_frames(name) in the reference's order with their frame index, per-frame counts, the stage_pass counters of the batch)"""
    blob = cascade().blob
    sp = np.zeros(cascade().count + 1, dtype=np.int64)
    parts = []
    for i, f in enumerate(face_frames(name)):
        h = ho.detect_raw(f, blob, stage_pass=sp)
        out = np.zeros(len(h), dtype=HIT_DTYPE)
        out["frame"] = i
        for k in ("scale", "q", "x", "y", "sum"):
            out[k] = h[k]
        parts.append(out)
    return _frozen(np.concatenate(parts)), [len(p) for p in parts], _frozen(sp)


@functools.lru_cache(maxsize=None)
def oracle_grouped(name, min_neighbors=1):
    """per frame of face_frames(name): ccv.detect_objects' grouped list"""
    hits, counts, _ = oracle_detect(name)
    out, k = [], 0
    for n in counts:
        h = np.zeros(n, dtype=ho.HIT_DTYPE)
        for fld in ("scale", "q", "x", "y", "sum"):
            h[fld] = hits[fld][k:k + n]
        out.append(_frozen(ho.group(ho.hits_to_rects(h), min_neighbors)))
        k += n
    return out


def select_best(grouped):
    """facetrackr.js:147-175: the grouped rect of the highest confidence, the first of equals; no detection: zeros, -10000, 0 neighbours"""
    best = np.zeros(1, dtype=ho.RECT_DTYPE)
    best[0]["confidence"] = -10000.0
    for k in range(len(grouped)):
        if k == 0 or grouped[k]["confidence"] > best[0]["confidence"]:
            best[0] = grouped[k]
    return best


def whitebalance(frame):
    """whitebalance.js:5-23 in numpy: the three channel sums (exact in int64), each divided by the pixel count, their mean"""
    px = frame.reshape(-1, 4)
    n = float(px.shape[0])
    r, g, b = (float(px[:, c].sum(dtype=np.int64)) for c in range(3))
    return (r / n + g / n + b / n) / 3


# ---- camshift: a blob within 200 pixels of the far edge -----------------------------------------------------------------------------------
# (cx, cy, a, b): elongated across the strip.  The reference sizes its next search window as 1.1 x (width, height) of the track object
# whatever its angle, so a blob elongated ALONG a 64-pixel strip is lost after one step; this one is tracked.
CS_BLOBS = {"wide": (16250, 30, 12, 22), "tall": (30, 16250, 12, 60)}
CS_STEPS = 4
CS_STREAMS = 2


@functools.lru_cache(maxsize=None)
def cs_case(name):
    """the shape of tests/test_gpu_camshift.py's test_frame_sizes_and_chunking: (seqs[stream][step], rects[stream])"""
    w, h = GEOMETRIES[name]
    cx0, cy0, a, b = CS_BLOBS[name]
    seqs, rects = [], []
    for s in range(CS_STREAMS):
        cx, cy = cx0 + 3 * s, cy0 - 2 * s
        seqs.append([_frozen(synth.blob_frame(w, h, cx + k, cy + k // 2, a, b, (4, 3, 5), (200, 60, 40), seed=77 + 13 * s + k)) for k in range(CS_STEPS)])
        rects.append((cx - a, cy - b, 2 * a, 2 * b))
    return seqs, rects


@functools.lru_cache(maxsize=None)
def cs_oracle(name):
    """(calls[step - 1][stream] = (search window, track object) of the oracle, models[stream] = the histogram initTracker leaves)"""
    seqs, rects = cs_case(name)
    calls = [[None] * CS_STREAMS for _ in range(CS_STEPS - 1)]
    models = []
    for s in range(CS_STREAMS):
        o = ho.Camshift(True)
        o.init_tracker(seqs[s][0], rects[s])
        models.append(_frozen(np.array(o.s.model, dtype=np.int64)))
        for k in range(1, CS_STEPS):
            calls[k - 1][s] = o.track(seqs[s][k])
    return calls, models


# ---- the planner harness's case lines (tests/host/geometry_plan_harness.cc, `plan` mode) ---------------------------------------------------
PLAN_GEOMETRIES = dict(SIZES, full=(16384, 16384), row=(16384, 1))


def plan_line(name, batch=2, dims=None):
    """a context's default plan inputs (interval 5, rs_rpt 4, tail cap 32768, nothing forced) for max_batch frames; ccv's own level sizes, or dims"""
    w, h = PLAN_GEOMETRIES[name] if dims is None else dims[0]
    line = f"{name} {w} {h} {batch} 5 4 0 0 0 32768 0 1 0 0 0 0 {len(dims or [])}"
    return line + "".join(f" {a} {b}" for a, b in dims or [])


# ---- the last tile column: a level as wide as the frame -------------------------------------------------------------------------------------
# ccv's widest resample destination is level 1, floor(16384 / 2^(1/6)) = 14596 pixels: 229 tile columns, bx <= 228.  Through level_dims
# level 2 takes the frame's own size (a ratio-1 copy, as tests/pyramid_cases.py's copy_level_case), so bx reaches 255 and level 8 halves the
# test's own bytes from 16384 columns.
COPIES = ("wide", "tall")  # and pass0 reaches 1023 on the tall one, whose tallest destination at ccv's sizes has 913 passes of 16 rows


@functools.lru_cache(maxsize=None)
def copy_case(name, copy_level=2):
    """the case dict tests/test_gpu_pyramid_ties.py's check_pyramid takes: the R channels of pyramid_frames(name) as gray planes"""
    w, h = SIZES[name]
    first = pc.ccv_dims(w, h, 5)[:6]
    first[copy_level] = (w, h)
    dims = pc.halved_from(first, 5)
    planes = [_frozen(np.ascontiguousarray(f[..., 0])) for f in pyramid_frames(name)]
    return dict(w=w, h=h, interval=5, dims=dims, planes=planes, targets=[])
