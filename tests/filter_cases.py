"""The prefiltered face crops' rule (headtrackr_amd/csrc/ht_filter_plan.h) restated in Python, from its description: the factors of an
entry, the fine patch — the UNFILTERED restatement of tests/crop_cases.py or tests/align_cases.py at Nx * P x Ny * Q —, and the block mean in
integers.  Shared by tests/test_filter_cpu.py and tests/test_gpu_filter.py; nothing here comes from the code under test, and everything is
seeded."""
import functools
import struct

import numpy as np

import align_cases as al
import crop_cases as cr

MAX_FACTOR = 8
# the GPU tests' patch sizes (P, Q).  3 x 4 was added because without it no crop entry of the scenes has a factor 6 and no align entry an
# Nx of 7 (tests/test_filter_cpu.py proves the coverage from the oracle alone)
SIZES = [(70, 19), (1, 1), (112, 112), (16, 7), (3, 4)]
MAX_FACTORS = (8, 3, 2)  # 8 and 3; 2 and 3 lie on either side of the threshold between the kernels' two tiles (64 x 16 up to 2, 64 x 4 from 3)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def factor(num, den, max_factor):
    """min(max_factor, max(1, ceil(num / den))), num >= 0: Python's // rounds towards -inf"""
    return min(max_factor, max(1, -((-num) // den)))


def crop_factors(code, rect, P, Q, max_factor):
    """(Nx, Ny) of a crop entry; (0, 0) for an empty one"""
    if code != cr.FACE:
        return (0, 0)
    return factor(rect[2], P, max_factor), factor(rect[3], Q, max_factor)


def align_factors(pl, P, Q, max_factor):
    """(Nx, Ny) of an align plan (code, a12, Cx, Cy, UxS, UyS, VxS, VyS); (0, 0) for an empty one"""
    if pl[0] != al.FACE:
        return (0, 0)
    return factor(abs(pl[4]) + abs(pl[5]), P * 65536, max_factor), factor(abs(pl[6]) + abs(pl[7]), Q * 65536, max_factor)


def mean(total, n):
    """one channel of one output pixel: the sum of its n fine samples, rounded"""
    return (total + (n >> 1)) // n


def block_mean(fine, nx, ny):
    """uint8 [Q, P, 4] of a fine patch uint8 [ny * Q, nx * P, 4]: per channel, alpha included, integer arithmetic"""
    H, W = fine.shape[:2]
    assert H % ny == 0 and W % nx == 0
    total = fine.astype(np.int64).reshape(H // ny, ny, W // nx, nx, 4).sum(axis=(1, 3))
    n = nx * ny
    return ((total + (n >> 1)) // n).astype(np.uint8)


def crop_patch(source, obj, W, H, mapping, margin_q8, flags, P, Q, max_factor):
    """(patch uint8 [Q, P, 4], (Nx, Ny)) of a dl.Source under the filtered crop rule"""
    code, rect = cr.rule(obj, W, H, source.w, source.h, mapping, margin_q8, flags)
    nx, ny = crop_factors(code, rect, P, Q, max_factor)
    if code != cr.FACE:
        return np.zeros((Q, P, 4), dtype=np.uint8), (0, 0)
    return block_mean(cr.patch(source, obj, W, H, mapping, margin_q8, flags, nx * P, ny * Q), nx, ny), (nx, ny)


def align_patch(source, obj, W, H, mapping, margin_q8, flags, P, Q, max_factor):
    """the same under the filtered align rule"""
    pl = al.plan(obj, W, H, source.w, source.h, mapping, margin_q8, flags)
    nx, ny = align_factors(pl, P, Q, max_factor)
    if pl[0] != al.FACE:
        return np.zeros((Q, P, 4), dtype=np.uint8), (0, 0)
    return block_mean(al.patch(source, obj, W, H, mapping, margin_q8, flags, nx * P, ny * Q), nx, ny), (nx, ny)


# ---- the harness cases of the CPU test: tests/host/filter_plan_harness.cc ------------------------------------------------------------------------
# (kind, w or ux, h or uy, vx, vy, P, Q, max_factor, code, sum, n): kind 0 crop (w, h), 1 align (ux, uy, vx, vy); the harness answers
# (Nx, Ny, mean(sum, n), first term, last term) through the RECORD functions, so code 0 gives 0, 0

CASE = struct.Struct("<4q8i")  # 64 bytes
assert CASE.size == 64


def pack_cases(cases):
    return b"".join(CASE.pack(c[1], c[2], c[3], c[4], c[0], c[5], c[6], c[7], c[8], c[9], c[10], 0) for c in cases)


def want_of(c):
    kind, a, b, vx, vy, P, Q, mf, code, total, n = c
    first = last = 0
    if kind == 0:
        nx, ny = crop_factors(code, (0, 0, a, b), P, Q, mf)
    else:
        nx, ny = align_factors((code, 0, 0, 0, a, b, vx, vy), P, Q, mf)
        if code == al.FACE:  # the fine patch's first and last column term: floor((2 i + 1 - P') v / 2 P') with P' = Nx P up to 8192
            Pf = nx * P
            first, last = ((1 - Pf) * a) // (2 * Pf), ((Pf - 1) * a) // (2 * Pf)
    return (nx, ny, mean(total, n), first, last)


def edge_cases():
    """w and h at exact multiples of P and Q and one either side; sums at the rounding half for even and odd n; |ux| + |uy| at the 2^49
    bound with P' = 8192 (P 1024, factor 8); empty records"""
    out = []
    for (P, Q) in ((112, 112), (70, 19), (1, 1), (16, 7), (1024, 1024), (1, 1024)):
        for mf in range(1, 9):
            for k in range(0, 11):
                for d in (-1, 0, 1):
                    w, h = k * P + d, k * Q + d
                    if w >= 1 and h >= 1 and w <= 16384 and h <= 16384:
                        out.append((0, w, h, 0, 0, P, Q, mf, 1, 0, 1))
                        out.append((0, w, 1, 0, 0, P, Q, mf, 1, 0, 1))
                        out.append((0, 1, h, 0, 0, P, Q, mf, 1, 0, 1))
                    # the same extents as an L1 norm in Q16, split between the two components with both signs, and one Q16 unit either side
                    for e in (-1, 0, 1):
                        l1x, l1y = max(0, k * P * 65536 + e), max(0, k * Q * 65536 + e)
                        out.append((1, l1x, 0, 0, l1y, P, Q, mf, 1, 0, 1))
                        out.append((1, -(l1x // 3), l1x - l1x // 3, -(l1y - l1y // 2), -(l1y // 2), P, Q, mf, 1, 0, 1))
            out.append((0, 16384, 16384, 0, 0, P, Q, mf, 1, 0, 1))
            out.append((0, 50, 60, 0, 0, P, Q, mf, 0, 0, 1))  # empty records: 0, 0 whatever else they hold
            out.append((1, 1 << 40, 5, 7, 1 << 41, P, Q, mf, 0, 0, 1))
            for s in (1, -1):  # the bound: each component 2^48, the sum 2^49
                out.append((1, s << 48, -s << 48, s << 48, s << 48, P, Q, mf, 1, 0, 1))
                out.append((1, (s << 48) - s, 0, 0, -s << 48, P, Q, mf, 1, 0, 1))
    # the rounding: every n = Nx Ny, sums around the half for even and odd n, the extremes
    for nx in range(1, 9):
        for ny in range(1, 9):
            n = nx * ny
            for q in (0, 1, 127, 254):
                for d in (-1, 0, 1):
                    for half in (n >> 1, (n + 1) >> 1):
                        s = q * n + half + d
                        if 0 <= s <= 255 * n:
                            out.append((0, 1, 1, 0, 0, 1, 1, 1, 1, s, n))
            out.append((0, 1, 1, 0, 0, 1, 1, 1, 1, 255 * n, n))
            out.append((0, 1, 1, 0, 0, 1, 1, 1, 1, 0, n))
    return out


def random_cases(n, seed=20264):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        P, Q, mf = int(rng.randint(1, 1025)), int(rng.randint(1, 1025)), int(rng.randint(1, 9))
        nn = int(rng.randint(1, 9)) * int(rng.randint(1, 9))
        total = int(rng.randint(0, 255 * nn + 1))
        code = int(rng.randint(8) != 0)
        if rng.randint(2):
            scale = [1, 3, 9][rng.randint(3)]
            out.append((0, int(rng.randint(1, min(16384, scale * P) + 1)), int(rng.randint(1, min(16384, scale * Q) + 1)), 0, 0, P, Q, mf, code, total, nn))
        else:
            bits = int(rng.randint(1, 49))
            v = [int(rng.randint(-(1 << bits), (1 << bits) + 1, dtype=np.int64)) for _ in range(4)]
            if rng.randint(4) == 0:  # norms within two Q16 units of a multiple of P 65536, split between the components
                k, part = int(rng.randint(1, 10)), int(rng.randint(0, 1000))
                v[0], v[1] = k * P * 65536 + int(rng.randint(-2, 3)) - part, -part
            out.append((1, v[0], v[1], v[2], v[3], P, Q, mf, code, total, nn))
    return out


# ---- the scenes of the GPU tests: the entries' factors, from the oracle alone ---------------------------------------------------------------------

def pairs_entry_factors(kind, objs, P, Q, margin_q8, flags, max_factor):
    """[(Nx, Ny)] of track objects on the 97 x 81 pairs canvas (the canvas is the source)"""
    W, H = cr.CANVAS
    out = []
    for to in objs:
        if kind == "crop":
            code, rect = cr.rule(cr.obj_of(to), W, H, W, H, None, margin_q8, flags)
            out.append(crop_factors(code, rect, P, Q, max_factor))
        else:
            out.append(align_factors(al.plan(al.obj_of(to), W, H, W, H, None, margin_q8, flags), P, Q, max_factor))
    return out


def feeds_entry_factors(kind, objs, P, Q, margin_q8, flags, max_factor):
    """[(Nx, Ny)] of the feeds' track objects, each in its own source through its mapping rect"""
    W, H = cr.CANVAS
    out = []
    for (src, m), to in zip(cr.feeds(), objs):
        if kind == "crop":
            code, rect = cr.rule(cr.obj_of(to), W, H, src.w, src.h, m, margin_q8, flags)
            out.append(crop_factors(code, rect, P, Q, max_factor))
        else:
            out.append(align_factors(al.plan(al.obj_of(to), W, H, src.w, src.h, m, margin_q8, flags), P, Q, max_factor))
    return out


def needs(kind, objs_and_geoms, P, Q, margin_q8, flags):
    """the unclamped ceilings (what max_factor cuts): [(need x, need y)] for FACE entries; objs_and_geoms = [(obj5, SW, SH, mapping)]"""
    W, H = cr.CANVAS
    out = []
    for obj, SW, SH, m in objs_and_geoms:
        if kind == "crop":
            code, rect = cr.rule(obj[:4], W, H, SW, SH, m, margin_q8, flags)
            if code == cr.FACE:
                out.append((-(-rect[2] // P), -(-rect[3] // Q)))
        else:
            pl = al.plan(obj, W, H, SW, SH, m, margin_q8, flags)
            if pl[0] == al.FACE:
                out.append((-(-(abs(pl[4]) + abs(pl[5])) // (P * 65536)), -(-(abs(pl[6]) + abs(pl[7])) // (Q * 65536))))
    return out


@functools.lru_cache(maxsize=None)
def checkerboard(w, h):
    """a 1-pixel checkerboard, opaque: pixel (x, y) is white where x + y is even"""
    pic = np.zeros((h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    pic[..., :3] = np.where(((xx + yy) & 1) == 0, 255, 0)[..., None]
    pic[..., 3] = 255
    return pic
