"""Frames laid out the way a host may leave them for ht_bind_frames_device / ht_camshift_track_sequence: any 4-byte-aligned base, any
frame stride >= W * H * 4 that is a multiple of 4.  Inputs of tests/test_gpu_frame_layouts.py and of the CPU proof that these inputs would
expose a kernel that reads them wrongly (tests/test_frame_layouts_cpu.py).  A plain module, imported like tests/cs_cases.py.

Everything is seeded (headtrackr_amd/synth.py); expected values always come from the CPU oracle on the TRUE frames.  `misread` restates the
mistakes a kernel could make — it classifies inputs, it never judges GPU output."""
import functools

import numpy as np

import cs_cases as cc
from headtrackr_amd import synth

NFRAMES = 5  # every batch: with a stride of fb + 4 and fb % 16 == 0, five frames see the alignment classes 0, 4, 8, 12 and 0 again
TAIL = 20    # bytes behind the last frame's stride


def fb_of(w, h):
    return w * h * 4


# name -> (lead, stride) as functions of the geometry; packed16 is the control: what every other GPU module binds
LAYOUTS = {
    "packed16": lambda w, h: (0, fb_of(w, h)),
    "lead4": lambda w, h: (4, fb_of(w, h)),
    "pad4": lambda w, h: (0, fb_of(w, h) + 4),
    "lead12_rowpad": lambda w, h: (12, fb_of(w, h) + 4 * (w + 5)),
    "double": lambda w, h: (8, 2 * fb_of(w, h) + 8),
}
CONTROL = "packed16"
HOWS = ("packed", "floor16")


def layout(name, w, h):
    """(lead, stride) in bytes of layout `name` for w x h frames"""
    return LAYOUTS[name](w, h)


def layout_seed(name, w, h, salt=0):
    return 61013 + 977 * list(LAYOUTS).index(name) + 13 * w + h + 100003 * salt


def lay_out(frames, lead, stride, seed):
    """uint8 image of lead + n * stride + TAIL bytes: frame f at lead + f * stride, every other byte (lead, gaps, tail) seeded random —
    plausible pixels that change every result if they are read"""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n, fb = len(frames), frames[0].nbytes
    assert lead >= 0 and stride >= fb
    img = (synth.lcg_stream(seed, lead + n * stride + TAIL) >> np.uint32(24)).astype(np.uint8)
    for f in range(n):
        img[lead + f * stride : lead + f * stride + fb] = frames[f].reshape(-1)
    return img


def read_at(image, offsets, w, h):
    """the [len(offsets), h, w, 4] frames a reader sees at the given byte offsets"""
    fb = fb_of(w, h)
    return np.stack([image[o : o + fb].reshape(h, w, 4) for o in offsets])


def true_offsets(lead, stride, n):
    return [lead + f * stride for f in range(n)]


def misread_offsets(lead, stride, n, w, h, how):
    if how == "packed":      # W * H * 4 where the stride belongs
        return [lead + f * fb_of(w, h) for f in range(n)]
    if how == "floor16":     # the base address rounded down to a 16-byte boundary (the image itself starts on one)
        return [(lead + f * stride) & ~15 for f in range(n)]
    raise ValueError(how)


def misread(image, lead, stride, n, w, h, how):
    """the frames a wrong reader would see"""
    return read_at(image, misread_offsets(lead, stride, n, w, h, how), w, h)


def affected(lead, stride, n, w, h, how):
    """frames whose misread address differs from their true address"""
    return [f for f, (a, b) in enumerate(zip(true_offsets(lead, stride, n), misread_offsets(lead, stride, n, w, h, how))) if a != b]


# ---- detect batches -----------------------------------------------------------------------------------------------------------------------

DETECT_SIZES = [(96, 80), (97, 81)]  # W % 4 == 0 and fb % 16 == 0: k_gray_linear; fb % 16 == 4: k_gray_rows


@functools.lru_cache(maxsize=None)
def detect_frames(w, h):
    """two frames with a 64-px face, one smooth, two noise.  Neighbours are of different families: where frames follow each other without
    a gap (lead4), a reader that starts 4 bytes early sees the last pixel of the frame before, and that pixel must not be the frame's own.
    The faces sit in frames 0 and 3: every layout moves at least one of them off a 16-byte boundary at both detect sizes"""
    out = np.stack([synth.face_frame(w, h, [(13, 8, 64)]), synth.noise_frame(w, h, 3 * w + h), synth.smooth_frame(w, h, w + h),
                    synth.face_frame(w, h, [(16, 10, 64)]), synth.noise_frame(w, h, 5 * w + h)])
    out.setflags(write=False)
    return out


# ---- camshift batches -----------------------------------------------------------------------------------------------------------------------

CS_SIZES = [(320, 240), (201, 157)]  # W % 4 == 0: the fused kernel's rows2d path; W % 4 != 0 and fb % 16 == 4: its linear path
CS_STEPS = 3


# stream numbers of cs_cases.stream_seq per size: blob and walk inside the frame, and a frame displaced by a single pixel moves the oracle's
# first track() (some streams' mean shift settles on the same integers; tests/test_frame_layouts_cpu.py asserts that these do not)
CS_STREAM_IDS = {(320, 240): (0, 3, 4, 5, 6), (201, 157): (6, 9, 14, 18, 24)}


@functools.lru_cache(maxsize=None)
def cs_streams(w, h):
    """five trackers of cs_cases.stream_seq, three track calls each"""
    out = tuple(cc.stream_seq(f"layout-{w}x{h}", stream, CS_STEPS, w, h) for stream in CS_STREAM_IDS[w, h])
    for s in out:
        r = max(s.rect[2], s.rect[3]) // 2 + 8  # the rotated ellipse and its walk of <= 3 px per call
        assert all(r <= g[0] < w - r and r <= g[1] < h - r for g in s.gens), s.name
    return out


def cs_batch(w, h, k):
    """the five-frame batch of call k (0: the frames the trackers are initialised on)"""
    out = np.stack([s.frames[k] for s in cs_streams(w, h)])
    out.setflags(write=False)
    return out


def cs_init_rects(w, h, kind):
    """one rect per stream on the stream's blob, on either side of the choice between the two initTracker kernels (the row-split kernel
    runs when the batch's tallest rect is >= 17 rows high): heights next to it from cs_cases.INIT_HEIGHTS"""
    heights = {"short": (1, 16, 16, 1, 16), "tall": (17, 16, 127, 1, 129)}[kind]
    assert set(heights) <= set(cc.INIT_HEIGHTS)
    rects = []
    for s, ht in zip(cs_streams(w, h), heights):
        cx, cy = s.gens[0][0], s.gens[0][1]
        rects.append((cx - s.rect[2] // 2, min(max(cy - ht // 2, 0), h - ht), s.rect[2], ht))
    return rects


def oracle_first_track(seq, frame1, frame0=None):
    """(search window, x, y, width, height) — the integer fields — of the oracle's first track() on frame1 after initTracker on frame0
    (default: the stream's own)"""
    from oracle import ht_oracle as ho

    o = ho.Camshift(True)
    o.init_tracker(seq.frames[0] if frame0 is None else frame0, seq.rect)
    sw, to = o.track(frame1)
    return tuple(int(v) for v in sw) + tuple(int(to[k]) for k in ("x", "y", "width", "height"))


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------------

PAIRS = [(0, 3), (1, 3), (2, 0), (4, 1)]  # (stream, bound frame): out of order, frame 3 twice, frames 2 and 4 named by no pair


# ---- the oracle's level-0 gray plane --------------------------------------------------------------------------------------------------------

def gray_plane(frame, gray_in_r=False):
    """level 0 of the oracle's pyramid: ccv.grayscale of the frame, or its R channel as it is (HT_INPUT_GRAY_IN_R)"""
    import ctypes as C

    from oracle import ht_oracle as ho

    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    h, w = frame.shape[:2]
    if gray_in_r:
        return frame[..., 0].copy()
    out = np.zeros((h, w), dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    ho.lib().ho_gray_plane(frame.ctypes.data_as(u8p), w, h, out.ctypes.data_as(u8p))
    return out
