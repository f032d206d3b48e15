"""The prefiltered draw list's rule (headtrackr_amd/csrc/ht_draw_filter_plan.h) restated in Python, from its description, and the scenes of
tests/test_draw_filter_cpu.py and tests/test_gpu_draw_filter.py.  The restatement is taken by import, not by copy: the fine frame is the
UNFILTERED restatement (ingest_cases.expected / yuv_cases.expected, through draw_list_cases.Source.expected) on the canvas of Nx W x Ny H,
the mean is filter_cases.block_mean.  Nothing here comes from the code under test, and everything is seeded."""
import functools
import struct

import numpy as np

import draw_list_cases as dl
import filter_cases as fc
import ingest_cases as ic
import yuv_cases as yc

MAX_FACTORS = (8, 3, 2, 1)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def size_of(source_wh, rect):
    """the extent the factors follow: the rect's, or the whole source's"""
    return (rect[2], rect[3]) if rect is not None else tuple(source_wh)


def factors(sw, sh, W, H, max_factor):
    return fc.factor(sw, W, max_factor), fc.factor(sh, H, max_factor)


def expected(source, rect, W, H, max_factor):
    """(canvas uint8 [H, W, 4], (Nx, Ny)) of a dl.Source under the filtered rule: the block mean of the fine draw"""
    nx, ny = factors(*size_of((source.w, source.h), rect), W, H, max_factor)
    return fc.block_mean(source.expected(rect, nx * W, ny * H), nx, ny), (nx, ny)


def expected_rgba(frame, rect, W, H, max_factor):
    """the same for a plain RGBA frame uint8 [h, w, 4]"""
    h, w = frame.shape[:2]
    nx, ny = factors(*size_of((w, h), rect), W, H, max_factor)
    return fc.block_mean(ic.expected(frame, rect, nx * W, ny * H), nx, ny), (nx, ny)


def checkerboard(w, h):
    return fc.checkerboard(w, h)


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------------------------------
# a scene: (canvas (W, H), sources, plan): plan[i] = (index into sources, rect or None) is entry i.  Sources are about 8 x their canvas at the
# most (none wider than 560 or taller than 240), every one with a size, pitch padding and matrix of its own; tests/test_draw_filter_cpu.py
# proves what the scenes cover.

S, N, I = dl.Source, yc.NV12, yc.I420


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "wide":  # 70 x 19: two tile columns, the second partial; partial tile rows in both tile forms
        srcs = [S(dl.RGBA, 560, 152, seed=101, pad0=12),                          # (8, 8), exact
                S(N, 333, 131, seed=102, matrix=1, pad0=13, pad1=6),               # odd x odd: (5, 7)
                S(I, 211, 57, seed=103, matrix=2, pad0=3, pad1=5),                 # odd x odd: (4, 3)
                S(N, 70, 152, seed=104, matrix=3, pad1=2, content="raw"),          # (1, 8)
                S(I, 560, 19, seed=105, matrix=0, pad0=8),                         # (8, 1)
                S(dl.RGBA, 430, 45, seed=106, pad0=4)]
        plan = [(0, None), (1, None), (2, None), (3, None), (4, None), (5, (7, 3, 420, 38)),   # (6, 2), exact, under a rect
                (0, (5, 3, 1, 100)), (1, (7, 1, 2, 40)), (2, (3, 5, 141, 39)), (5, (0, 0, 70, 19))]  # 1 and 2 wide: (1, 6), (1, 3); (3, 3); 1 : 1
        return (70, 19), srcs, plan
    if name == "canvas":  # 40 x 30
        srcs = [S(N, 333, 217, seed=111, matrix=1, pad0=13, pad1=6),               # nx 9 -> 8 (limited), ny 8
                S(dl.RGBA, 560, 152, seed=112, pad0=12, content="smooth"),         # nx 14 -> 8 (limited), ny 6
                S(I, 23, 23, seed=113, matrix=2, pad0=4),                          # an upscale: (1, 1)
                S(dl.RGBA, 1, 5, seed=114, pad0=8),
                S(I, 333, 217, seed=115, matrix=3, pad0=7, pad1=9),
                S(N, 23, 23, seed=116, matrix=2, pad0=5, pad1=4, content="raw"),
                S(I, 2, 2, seed=117, matrix=0, pad0=3, pad1=5, content="raw"),
                S(dl.RGBA, 80, 60, seed=118, content="ties"),                      # (2, 2), exact: every block mean of the source a .5 tie
                S(I, 117, 120, seed=119, matrix=1, pad1=3),                        # (3, 4)
                S(N, 199, 149, seed=120, matrix=0, pad0=1)]                        # (5, 5)
        plan = [(0, None), (1, None), (2, None), (3, None), (4, (3, 5, 326, 208)), (5, (1, 1, 21, 21)), (6, None), (7, None), (8, None), (9, None),
                (4, (1, 0, 270, 31)), (1, (9, 2, 241, 150))]                       # (7, 2); (7, 5)
        return (40, 30), srcs, plan
    if name == "small":  # 3 x 4: three entries
        srcs = small_sources()
        return (3, 4), srcs, [(0, None), (3, None), (7, (1, 1, 20, 29))]
    if name == "long":  # 3 x 4: 70 entries, past the staged table's first reservation of 64 descriptors
        srcs = small_sources()
        rects = [None, (1, 1, 2, 2), (0, 0, 1, 1), None, (1, 0, 2, 3)]
        plan = []
        for k in range(70):
            s = srcs[k % len(srcs)]
            r = rects[(k // len(srcs) + k) % len(rects)]
            plan.append((k % len(srcs), r if r is None or (r[0] + r[2] <= s.w and r[1] + r[3] <= s.h) else None))
        return (3, 4), srcs, plan
    if name == "pixel":  # 1 x 1
        srcs = [S(dl.RGBA, 1, 1, seed=131), S(dl.RGBA, 8, 8, seed=132, pad0=4), S(N, 5, 3, seed=133, matrix=1, pad0=2, pad1=2), S(I, 3, 7, seed=134, matrix=2, pad1=1),
                S(dl.RGBA, 9, 9, seed=135)]
        return (1, 1), srcs, [(0, None), (1, None), (2, None), (3, None), (4, None), (1, (2, 3, 4, 2))]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def small_sources():
    """eight sources for the 3 x 4 canvas: widths 1 .. 24 and heights 1 .. 32, the formats cycling"""
    sizes = [(24, 32), (5, 9), (1, 1), (13, 21), (3, 4), (19, 13), (7, 30), (22, 31)]
    fmts = [dl.RGBA, N, I, N, dl.RGBA, I, N, I]
    return [S(f, w, h, seed=140 + k, matrix=k % 4, pad0=4 * (k % 3), pad1=2 * (k % 2), content="raw" if f != dl.RGBA and k % 2 else "noise")
            for k, (f, (w, h)) in enumerate(zip(fmts, sizes))]


SCENES = ("wide", "canvas", "small", "long", "pixel")


@functools.lru_cache(maxsize=None)
def scene_expected(name, max_factor):
    """[(canvas, (Nx, Ny))] of a scene's entries: computed once per (scene, max_factor)"""
    (W, H), srcs, plan = scene(name)
    return [expected(srcs[k], rect, W, H, max_factor) for k, rect in plan]


def uniform_list(nx, ny, W, H):
    """three sources (RGBA, NV12, I420) whose whole frame has factors exactly (nx, ny) on W x H, not at an exact ratio: for the twin-context test"""
    w, h = nx * W - (1 if nx > 1 else 0), ny * H - (1 if ny > 1 else 0)
    return [S(dl.RGBA, w, h, seed=151, pad0=4), S(N, w, h, seed=152, matrix=1, pad0=3, pad1=2), S(I, w, h, seed=153, matrix=3, pad1=1)]


# ---- the harness cases of the CPU test: tests/host/draw_filter_plan_harness.cc -------------------------------------------------------------------
# (p0, p1, p2, pitch0, pitch1, W, H, max_factor, width, height, format, matrix, rx, ry, rw, rh, lead)

CASE = struct.Struct("<5Q12i")
assert CASE.size == 88
OK, BAD_COUNT, BAD_CANVAS, BAD_FORMAT, BAD_SIZE, BAD_MATRIX, BAD_PITCH0, BAD_PITCH1, NULL_PLANE, MISALIGNED, BAD_RECT = range(11)
BAD_FACTOR = 100
P = (0x10000, 0x90000, 0xA0000)


def case(fmt, w, h, W, H, mf, p=P, pitch=(0, 0), matrix=0, rect=(0, 0, 0, 0), lead=0):
    return (*p, *pitch, W, H, mf, w, h, fmt, matrix, *rect, lead)


def pack_cases(cases):
    return b"".join(CASE.pack(*c) for c in cases)


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def want_of(c):
    """the restatement's answer to one case: (status, bad, Nx, Ny, bits of rx', bits of ry', sx, sy, sw, sh, pitch0, pitch1, cw); the checks in
    the order ht_draw_filter_plan.h and ht_draw_list_plan.h state them"""
    p0, p1, p2, pitch0, pitch1, W, H, mf, w, h, fmt, matrix, rx, ry, rw, rh, lead = c

    def refuse(status, entry=True):
        return (status, lead if entry else -1) + (0,) * 11

    if W <= 0 or H <= 0:
        return refuse(BAD_CANVAS, False)
    if not 1 <= mf <= 8:
        return refuse(BAD_FACTOR, False)
    if fmt == dl.RGBA:
        if not (1 <= w <= 16384 and 1 <= h <= 16384):
            return refuse(BAD_SIZE)
        e0 = pitch0 or 4 * w
        if e0 % 4 or e0 < 4 * w or e0 > 1 << 32:
            return refuse(BAD_PITCH0)
        if not p0:
            return refuse(NULL_PLANE)
        if p0 % 4:
            return refuse(MISALIGNED)
        e1 = cw = 0
    else:
        if not (1 <= w <= 16384 and 1 <= h <= 16384):
            return refuse(BAD_SIZE)
        if fmt not in (N, I):
            return refuse(BAD_FORMAT)
        if not 0 <= matrix <= 3:
            return refuse(BAD_MATRIX)
        cw = (w + 1) // 2
        crow = 2 * cw if fmt == N else cw
        e0, e1 = pitch0 or w, pitch1 or crow
        if e0 < w:
            return refuse(BAD_PITCH0)
        if e1 < crow or (fmt == N and e1 % 2):
            return refuse(BAD_PITCH1)
        if e0 > 1 << 32 or e1 > 1 << 32:
            return refuse(BAD_PITCH0 if e0 > 1 << 32 else BAD_PITCH1)
        if not p0 or not p1 or (fmt == I and not p2):
            return refuse(NULL_PLANE)
        if fmt == N and p1 % 2:
            return refuse(MISALIGNED)
    sx, sy, sw, sh = 0, 0, w, h
    if rw != 0 or rh != 0:
        if rx < 0 or ry < 0 or rw <= 0 or rh <= 0 or rw > w - rx or rh > h - ry:
            return refuse(BAD_RECT)
        sx, sy, sw, sh = rx, ry, rw, rh
    nx, ny = factors(sw, sh, W, H, mf)
    return (OK, -1, nx, ny, bits(sw / (nx * W)), bits(sh / (ny * H)), sx, sy, sw, sh, e0, e1, cw)  # Python's / is one binary64 division


def edge_cases():
    """sizes 1 and 16384, canvases 1 and beyond 1024, the factor's steps at exact multiples of the canvas and one either side, every factor and
    every max_factor, max_factor 0 and 9, and every refusal of the draw list's plan at entry 0 of 1 and at entry 5 of 6"""
    cs = []
    for fmt in (dl.RGBA, N, I):
        for (w, h) in ((1, 1), (16384, 16384), (1, 16384), (16384, 1), (1920, 1080), (1280, 720)):
            for (W, H) in ((1, 1), (320, 240), (1024, 1024), (1025, 2049), (4096, 3), (16384, 16384)):
                for mf in range(1, 9):
                    cs.append(case(fmt, w, h, W, H, mf))
    for (W, k) in ((70, 3), (40, 8), (3, 5), (1, 7)):
        for d in (-1, 0, 1):
            for mf in (8, k, max(k - 1, 1)):
                if k * W + d >= 1:
                    cs.append(case(dl.RGBA, k * W + d, 9, W, 30, mf))
                    cs.append(case(I, 40, k * W + d, 40, W, mf, matrix=2))
                    cs.append(case(N, 600, 600, W, W, mf, rect=(3, 5, k * W + d, k * W + d)))
    for mf in (0, 9, -1, 1 << 30, -(1 << 31)):
        cs += [case(dl.RGBA, 64, 64, 8, 8, mf), case(N, 64, 64, 8, 8, mf, lead=5), case(dl.RGBA, 0, 64, 8, 8, mf)]  # the call's fault comes before an entry's
    cs += [case(dl.RGBA, 64, 64, 0, 8, 8), case(dl.RGBA, 64, 64, 8, -1, 8), case(dl.RGBA, 64, 64, 0, 8, 0)]
    for lead in (0, 5):
        cs += [case(2, 8, 8, 4, 4, 8, lead=lead), case(-1, 8, 8, 4, 4, 8, lead=lead), case(15, 8, 8, 4, 4, 8, lead=lead), case(17, 8, 8, 4, 4, 8, lead=lead),
               case(dl.RGBA, 0, 8, 4, 4, 8, lead=lead), case(dl.RGBA, 8, 16385, 4, 4, 8, lead=lead), case(N, -3, 8, 4, 4, 8, lead=lead), case(I, 16385, 8, 4, 4, 8, lead=lead),
               case(N, 8, 8, 4, 4, 8, matrix=4, lead=lead), case(I, 8, 8, 4, 4, 8, matrix=-1, lead=lead),
               case(dl.RGBA, 8, 8, 4, 4, 8, pitch=(28, 0), lead=lead), case(dl.RGBA, 8, 8, 4, 4, 8, pitch=(34, 0), lead=lead),
               case(dl.RGBA, 8, 8, 4, 4, 8, pitch=((1 << 32) + 4, 0), lead=lead), case(N, 9, 8, 4, 4, 8, pitch=(8, 0), lead=lead),
               case(N, 9, 8, 4, 4, 8, pitch=(0, 8), lead=lead), case(N, 9, 8, 4, 4, 8, pitch=(0, 11), lead=lead), case(I, 9, 8, 4, 4, 8, pitch=(0, 4), lead=lead),
               case(dl.RGBA, 8, 8, 4, 4, 8, p=(0, 0, 0), lead=lead), case(N, 8, 8, 4, 4, 8, p=(0x100, 0, 0), lead=lead), case(N, 8, 8, 4, 4, 8, p=(0, 0x100, 0), lead=lead),
               case(I, 8, 8, 4, 4, 8, p=(0x100, 0x200, 0), lead=lead),
               case(dl.RGBA, 8, 8, 4, 4, 8, p=(0x102, 0, 0), lead=lead), case(N, 8, 8, 4, 4, 8, p=(0x100, 0x201, 0), lead=lead),
               case(dl.RGBA, 8, 8, 4, 4, 8, rect=(1, 0, 8, 8), lead=lead), case(N, 8, 8, 4, 4, 8, rect=(0, 1, 8, 8), lead=lead), case(I, 8, 8, 4, 4, 8, rect=(-1, 0, 4, 4), lead=lead),
               case(dl.RGBA, 8, 8, 4, 4, 8, rect=(0, 0, 0, 5), lead=lead), case(dl.RGBA, 8, 8, 4, 4, 8, rect=(0, 0, 5, -1), lead=lead), case(N, 8, 8, 4, 4, 8, rect=(8, 0, 1, 1), lead=lead)]
    return cs


def random_cases(n, seed=20265):
    """n seeded entries: formats, sizes from 1 to 16384 (small ones often), canvases from 1 to 2048, rects, paddings, every max_factor; about
    one in eight is made wrong in one way"""
    rng = np.random.default_rng(seed)
    cs = []
    for _ in range(n):
        fmt = (dl.RGBA, N, I)[int(rng.integers(3))]
        span = (64, 2048, 16384)[int(rng.integers(3))]
        w, h = int(rng.integers(1, span + 1)), int(rng.integers(1, span + 1))
        cspan = (8, 320, 2048)[int(rng.integers(3))]
        W, H = int(rng.integers(1, cspan + 1)), int(rng.integers(1, cspan + 1))
        mf = int(rng.integers(1, 9))
        rect = (0, 0, 0, 0)
        if rng.integers(2):
            rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            rect = (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh)
        pad = int(rng.integers(0, 4))
        pitch = (0, 0) if not pad else ((4 * w + 4 * pad, 0) if fmt == dl.RGBA else (w + pad, (2 * ((w + 1) // 2) if fmt == N else (w + 1) // 2) + 2 * pad))
        p, matrix, lead = P, int(rng.integers(4)), int(rng.integers(0, 3))
        wrong = int(rng.integers(0, 64))
        if wrong == 0:
            mf = (0, 9, -4)[int(rng.integers(3))]
        elif wrong == 1:
            rect = (rect[0] + 1, rect[1], w, max(rect[3], 1))
        elif wrong == 2:
            p = (0x10002 if fmt == dl.RGBA else 0x10000, 0x90001 if fmt == N else 0, 0xA0000)
        elif wrong == 3:
            w = 16385
        elif wrong == 4:
            matrix = 4
        elif wrong == 5:
            pitch = (4 * w - 4 if fmt == dl.RGBA else w - 1, 0) if w > 1 else (0, 1 if fmt == N else 0)
        elif wrong == 6:
            W = 0
        elif wrong == 7:
            fmt = 7
        cs.append(case(fmt, w, h, W, H, mf, p=p, pitch=pitch, matrix=matrix, rect=rect, lead=lead))
    return cs
