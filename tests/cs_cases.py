"""Inputs and coverage guards of the camshift path tests (tests/test_gpu_camshift_paths.py, tests/test_cs_cases_cpu.py).  A plain module,
imported like tests/hipmem.py; the judge (check() / assert_all_exact()) stays in tests/test_gpu_camshift.py.

Everything here is built from seeds by headtrackr_amd/synth.py; the expected values always come from the CPU oracle (oracle.ht_oracle).
The restatement of the kernels' region rectangle below (region_rect) CLASSIFIES inputs — "this call's window left the region a kernel
would have cached" — so that a CPU test can prove that every sequence reaches the state it is named after.  It never judges GPU output."""
import contextlib
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

from headtrackr_amd import synth
from oracle import ht_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ANGLE_TOL = math.radians(0.5)  # the project's camshift angle tolerance (BASELINE.json north_star); tests/test_gpu_camshift.py asserts it

# ---- the kernels' region rectangle, restated to classify inputs (never to judge output) -------------------------------------------------

REGION_CAP = 40960        # CS_REGION_CAP: the 1024-thread fused kernel and the one-workgroup mean-shift kernel
REGION_CAP_SMALL = 22528  # CS_REGION_CAP_SMALL: the 512-thread fused kernel


def clamped_window(W, H, sw):
    """(x0, y0, x1, y1) of a search window clamped to the frame, as every moment pass clamps it (camshift.js:287-290)"""
    x0, y0 = max(sw[0], 0), max(sw[1], 0)
    return x0, y0, min(x0 + sw[2], W), min(y0 + sw[3], H)


def clamped_area(W, H, sw):
    x0, y0, x1, y1 = clamped_window(W, H, sw)
    return max(x1 - x0, 0) * max(y1 - y0, 0)


def region_rect(W, H, sw, cap=REGION_CAP):
    """dict(x0, y0, rw, rh, mg) of the neighbourhood a kernel caches for search window `sw` with capacity `cap` pixels: the clamped
    window grown by the largest margin <= 16 that fits; None when nothing is cached"""
    x0, y0, x1, y1 = clamped_window(W, H, sw)
    w0, h0 = x1 - x0, y1 - y0
    if w0 <= 0 or h0 <= 0 or w0 * h0 > cap:
        return None
    mg, t = 0, 16
    while t > 0:
        if mg + t <= 16 and (min(x1 + mg + t, W) - max(x0 - mg - t, 0)) * (min(y1 + mg + t, H) - max(y0 - mg - t, 0)) <= cap:
            mg += t
        t >>= 1
    rx0, ry0 = max(x0 - mg, 0), max(y0 - mg, 0)
    return dict(x0=rx0, y0=ry0, rw=min(x1 + mg, W) - rx0, rh=min(y1 + mg, H) - ry0, mg=mg,
                clamped=dict(left=x0 - mg < 0, top=y0 - mg < 0, right=x1 + mg > W, bottom=y1 + mg > H))


def margin_area(W, H, sw, mg):
    """pixels of the region with margin `mg`: the smallest capacity that admits this margin"""
    x0, y0, x1, y1 = clamped_window(W, H, sw)
    return (min(x1 + mg, W) - max(x0 - mg, 0)) * (min(y1 + mg, H) - max(y0 - mg, 0))


def ends_inside(W, H, sw_before, sw_after, cap=REGION_CAP):
    """True / False: the window of the call's last moment pass (final position, size of the call's start) lies inside the region
    cached at the start of the call; None: nothing was cached"""
    R = region_rect(W, H, sw_before, cap)
    if R is None:
        return None
    x0, y0, x1, y1 = clamped_window(W, H, [sw_after[0], sw_after[1], sw_before[2], sw_before[3]])
    return x0 >= R["x0"] and y0 >= R["y0"] and x1 <= R["x0"] + R["rw"] and y1 <= R["y0"] + R["rh"]


def region_sweep_values(W, H, sw):
    """option cs_region values around the first search window `sw`: off, its clamped area A -1 / +0 / +1 (capacity boundary), the
    exact pixel counts that admit margins 1, 3, 8, 15 and 16, and the two built-in capacities"""
    A = clamped_area(W, H, sw)
    return [0, A - 1, A, A + 1] + [margin_area(W, H, sw, m) for m in (1, 3, 8, 15, 16)] + [REGION_CAP_SMALL, REGION_CAP]


# ---- sequences ----------------------------------------------------------------------------------------------------------------------

class Seq:
    """one tracker's input: frames[0] initialises it on `rect`, every later frame is one track() call"""

    def __init__(self, name, w, h, rect, gens, tags=()):
        self.name, self.w, self.h, self.rect, self.gens, self.tags = name, w, h, tuple(rect), gens, tuple(tags)

    @functools.cached_property
    def frames(self):
        return [synth.blob_frame(self.w, self.h, *g) for g in self.gens]

    @property
    def ncalls(self):
        return len(self.gens) - 1

    def oracle_calls(self):
        """[(search window before, search window after, track object)] of every call, from the oracle"""
        o = ho.Camshift(True)
        o.init_tracker(self.frames[0], self.rect)
        out = []
        for f in self.frames[1:]:
            before = o.search_window()
            sw, to = o.track(f)
            out.append((before, sw, to))
        return out


def blob_seq(name, w, h, cx, cy, a, b, moves, seed, rot=(4, 3, 5), color=(200, 60, 40), rect=None, tags=()):
    """a blob (semi-axes a, b) that starts at (cx, cy) and moves by `moves` [(dx, dy), ...] between calls; the tracker starts on the
    blob's bounding rect (or `rect`)"""
    gens, x, y = [], cx, cy
    for k, (dx, dy) in enumerate([(0, 0)] + list(moves)):
        x, y = x + dx, y + dy
        gens.append((x, y, a, b, rot, color, seed + k))
    return Seq(name, w, h, rect or (cx - a, cy - b, 2 * a, 2 * b), gens, tags)


JUMPS_A = [(25, 0), (0, 22), (-30, -20), (40, 30), (-45, 10)]
JUMPS_B = [(-25, 5), (30, -22), (28, 20), (-40, -30), (45, -10)]
JUMPS_C = [(35, 20), (-50, 0), (20, -40), (60, 0), (4, 3)]  # the last one: a call that stays inside


@functools.lru_cache(maxsize=None)
def jumping():
    """B: the blob moves by 20 - 60 px between calls, so the mean-shift walk leaves the region cached at the start of the call"""
    return [blob_seq("jump-320-a", 320, 240, 150, 110, 30, 18, JUMPS_A, 4100, tags=("leaves",)),
            blob_seq("jump-320-b", 320, 240, 170, 130, 30, 18, JUMPS_B, 4200),
            blob_seq("jump-641", 641, 363, 300, 180, 60, 30, JUMPS_C, 4300, tags=("leaves",))]


@functools.lru_cache(maxsize=None)
def static():
    return [blob_seq("static-320", 320, 240, 160, 120, 30, 18, [(0, 0)] * 3, 4400)]


@functools.lru_cache(maxsize=None)
def edges():
    """B: windows that touch or cross each border and two opposite corners (the region's margin is clamped on those sides), and a
    jump from the interior to a border.  tags name the sides whose margin must be clamped in at least one call."""
    w, h, a, b = 320, 240, 30, 18
    mv = [(2, 1), (-1, 2), (1, -1)]
    return [blob_seq("edge-left", w, h, 22, 120, a, b, mv, 4500, tags=("left",)),
            blob_seq("edge-right", w, h, 300, 120, a, b, mv, 4510, tags=("right",)),
            blob_seq("edge-top", w, h, 160, 12, a, b, mv, 4520, tags=("top",)),
            blob_seq("edge-bottom", w, h, 160, 230, a, b, mv, 4530, tags=("bottom",)),
            blob_seq("corner-top-left", w, h, 20, 12, a, b, mv, 4540, tags=("left", "top")),
            blob_seq("corner-bottom-right", w, h, 302, 230, a, b, mv, 4550, tags=("right", "bottom")),
            blob_seq("interior-to-right-border", w, h, 230, 120, a, b, [(30, 5), (24, 2), (10, -1), (6, 1)], 4560, tags=("right",))]


@functools.lru_cache(maxsize=None)
def column_phases():
    """B: on a W % 4 == 0 frame the fused kernel stashes the region during its histogram pass in 16-byte groups; the init rect puts the
    region's left edge at every residue mod 4 and gives its width every residue (the first call's region is rect + 16 px all round).
    The blob is wider than the rect, so the window's outermost columns hold blob pixels: weights that count, not background noise that
    the model gives weight 0 (a wrong bin there would go unnoticed)"""
    out = []
    for i in range(4):
        for j in range(4):
            x, wd = 100 + i, 56 + j
            out.append(blob_seq(f"phase-x{i}-w{j}", 320, 240, x + wd // 2, 120, 36, 16, [(3, 2), (-2, 1)], 4600 + 4 * i + j, rect=(x, 102, wd, 36),
                                tags=(i, j)))
    return out


@functools.lru_cache(maxsize=None)
def frame_widths():
    """B: how the fused kernel fills its cache depends on the frame's width: W % 4 == 0 and W / 4 <= threads -> during the histogram
    pass, else a separate copy pass; 2052 takes the first way with 1024 threads and the second with 512"""
    mv = [(3, 1), (-2, 2), (4, -1)]
    return [blob_seq("width-321", 321, 240, 160, 120, 30, 18, mv, 4700),
            blob_seq("width-641", 641, 363, 320, 180, 30, 18, mv, 4710),
            blob_seq("width-2052", 2052, 40, 1000, 20, 22, 9, mv, 4720),
            blob_seq("width-4100", 4100, 24, 2000, 12, 18, 7, mv, 4730)]


@functools.lru_cache(maxsize=None)
def capacities():
    """B: a window whose clamped area lies between the two built-in capacities (the 1024-thread fused kernel and the one-workgroup
    mean-shift kernel cache it, the 512-thread fused kernel does not) and one above both (nobody caches it), each moving"""
    mv = [(4, 2), (-3, 3), (5, -2)]
    return [blob_seq("between-caps-641", 641, 363, 320, 180, 95, 70, mv, 4800, rot=(1, 0, 1), tags=("between",)),
            blob_seq("above-caps-1280", 1280, 720, 640, 360, 150, 110, mv, 4810, rot=(1, 0, 1), tags=("above",))]


def zero_margin():
    """B: [(sequence, cs_region value)] — with the capacity set to the first window's area the first call's region IS the window
    (margin 0), so its moment passes read the region's outermost columns and rows: the partial 16-byte groups of the stash path at
    every column phase, and the last lane / row of the separate copy pass"""
    return [(s, clamped_area(s.w, s.h, s.rect)) for s in column_phases() + frame_widths()]


def region_sequences():
    """every single-tracker sequence of part B"""
    return jumping() + static() + edges() + column_phases() + frame_widths() + capacities()


# ---- A: stream ranges -------------------------------------------------------------------------------------------------------------------

COLORS = [(200, 60, 40), (40, 200, 80), (40, 80, 230), (220, 200, 30)]
ROTS = [(1, 0, 1), (4, 3, 5), (3, 4, 5), (12, 5, 13), (0, 1, 1)]


def stream_seq(tag, stream, steps, w=320, h=240):
    """tracker `stream` of a layout: its own position, size, colour, rotation and walk (<= 3 px per call), all from the stream number"""
    r = synth.lcg_stream(7000 + 131 * stream, 16).astype(np.int64) >> 12
    cx, cy = 70 + int(r[0] % 180), 60 + int(r[1] % 120)
    a, b = 16 + int(r[2] % 24), 10 + int(r[3] % 14)
    walk = [int(v % 7) - 3 for v in r[6:14]]
    moves = [(walk[(2 * k) % 8], walk[(2 * k + 1) % 8]) for k in range(steps)]
    return blob_seq(f"{tag}-s{stream}", w, h, cx, cy, a, b, moves, 7100 + 37 * stream, rot=ROTS[int(r[4] % 5)], color=COLORS[int(r[5] % 4)])


# reservation, [(first, n)]: disjoint ranges initialised and tracked by separate calls; the gaps are never initialised.  On the cluster
# schedule the workgroups per stream are min(32, CUs / n): 32 for n = 5 and 7, 28 and 23 for n = 9 and 11 (256 CUs), 4 for n = 64.
LAYOUTS = {"r24": (24, [(0, 5), (5, 7), (17, 7)]), "r100": (100, [(3, 9), (20, 11), (36, 64)])}
RANGE_STEPS = 4


@functools.lru_cache(maxsize=None)
def layout_streams(name):
    """{stream: Seq} of every tracked stream of a layout"""
    _res, ranges = LAYOUTS[name]
    return {first + s: stream_seq(name, first + s, RANGE_STEPS) for first, n in ranges for s in range(n)}


def range_batch(seqs, first, n, k):
    """the n-frame batch of call k for streams [first, first + n): slot s holds stream first + s's frame"""
    return np.stack([seqs[first + s].frames[k] for s in range(n)])


@functools.lru_cache(maxsize=None)
def default_path_streams(w, h, steps=3, distinct=8):
    """E: the trackers of a default-options call at a small frame size: `distinct` different sequences (position, size, colour, rotation, walk),
    stream s of a call takes sequence s % distinct — neighbouring streams differ, and the oracle runs `distinct` times whatever the call's size"""
    out = []
    for k in range(distinct):
        a, b = w // 6 + k % 3, h // 8 + k % 2
        moves = [((k + j) % 3 - 1, (2 * k + j) % 3 - 1) for j in range(steps)]
        out.append(blob_seq(f"default-{w}x{h}-{k}", w, h, w // 2 - 6 + 2 * (k % 4), h // 2 - 4 + k // 2, a, b, moves, 5200 + 11 * k + w, rot=ROTS[k % 5],
                            color=COLORS[k % 4]))
    return out


@functools.lru_cache(maxsize=None)
def growing():
    """A: the reservation grows between two track calls (1 -> 40 streams); at 1920x1080 that changes the chunking from 127 to 8 chunks"""
    mv = [(3, 1), (-2, 2), (4, -1), (2, 2)]
    return [blob_seq("grow-1080p", 1920, 1080, 900, 500, 180, 120, mv, 4900), blob_seq("grow-320", 320, 240, 150, 110, 30, 18, mv, 4910)]


def all_track_sequences():
    """every sequence whose track() results a GPU test of parts A and B compares with the oracle"""
    out = region_sequences() + growing()
    for name in LAYOUTS:
        out += list(layout_streams(name).values())
    return out


# ---- C: initTracker rects ---------------------------------------------------------------------------------------------------------------

INIT_W, INIT_H = 400, 300
INIT_WIDTHS = (1, 63, 64, 65, 128, 129)      # next to the 64 lanes of a column block (both kernels) and the 256-column batch of the row kernel
INIT_HEIGHTS = (1, 16, 17, 127, 128, 129, 257)  # next to 16 (kernel choice), the 8 x 16 rows of a batch of k_cs_init and the row kernel's 4 G stride


def init_frame(slot, seed=5000):
    return synth.blob_frame(INIT_W, INIT_H, 120 + 5 * (slot % 30), 100 + 3 * (slot % 40), 60, 40, ROTS[slot % 5], COLORS[slot % 4], seed + slot)


def init_grid_rects():
    """the 42 (width, height) pairs, each at its own place inside the frame"""
    return [(7 + 3 * i + j, 5 + 2 * j + i, wd, ht) for i, wd in enumerate(INIT_WIDTHS) for j, ht in enumerate(INIT_HEIGHTS)]


def init_border_rects():
    """rects crossing each border and corner, and one entirely outside the frame (everything lands in bin 0)"""
    W, H = INIT_W, INIT_H
    return [(-20, 100, 70, 50), (W - 30, 90, 70, 50), (150, -9, 65, 40), (150, H - 11, 65, 40), (-5, -7, 64, 17), (W - 40, H - 13, 129, 33),
            (-3, -3, W + 6, 20), (W + 10, H + 10, 30, 20), (-100, 50, 60, 30)]


def init_batches():
    """[(name, kernel, rects)]: kernel is the one ht_camshift_init_batch dispatches for that batch ('rows': n < 64 and a height >= 17)"""
    grid, border = init_grid_rects(), init_border_rects()
    varied = (grid + border + [(30 + 4 * k, 20 + 3 * k, 40 + 5 * k, 30 + 7 * k) for k in range(13)])[:64]
    assert len(varied) == 64
    out = [("n64-varied", "wg", varied),
           ("n3-short", "wg", [(10, 10, 129, 16), (200, 100, 65, 1), (-4, 280, 64, 15)]),
           ("n5-one-tall", "rows", [(50, 20, 65, 257), (10, 10, 63, 1), (100, 100, 128, 16), (-5, 200, 64, 3), (300, 290, 129, 8)]),
           ("n40-mixed", "rows", (grid[:31] + border)[:40]),
           ("n9-border", "rows", border)]
    out += [(f"n1-{wd}x{ht}", "wg" if ht <= 16 else "rows", [(x, y, wd, ht)]) for (x, y, wd, ht) in grid]
    return out


def model_histogram(frame, rect):
    return np.array(ho.cs_init(frame, *rect).s.model, dtype=np.int64)


def frame_histogram(frame):
    """camshift.Histogram of a whole frame (camshift.js:49-72), as oracle.ht_oracle.cs_histograms computes it"""
    px = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1, 4).astype(np.int64)
    return np.bincount(256 * (px[:, 0] >> 4) + 16 * (px[:, 1] >> 4) + (px[:, 2] >> 4), minlength=4096)


# ---- D: chunk-histogram edges -------------------------------------------------------------------------------------------------------------

# pixel counts on and next to the quanta of the chunking: a chunk is a multiple of 4 * 1024 = 4096 px, at least one chunk per 16 384 px
HIST_SIZES = [(64, 64), (65, 63), (241, 17), (128, 128), (145, 113), (256, 128), (331, 99)]
HIST_FAMILIES = ("noise", "flat", "blocks")
HIST_TRACKED_RESERVED = [(1, 1), (1, 32), (3, 32), (1, 40), (3, 40)]  # reservations in growing order: one context serves them all


def hist_frame(family, w, h, slot):
    """noise: every 16-byte group of 4 pixels mixes bins; flat: every group takes the merged add; blocks: runs of 3 and 5 equal
    pixels, so groups straddle bin changes and the chunk's tail ends inside a run"""
    if family == "noise":
        return synth.noise_frame(w, h, 8000 + slot)
    out = np.empty((h, w, 4), dtype=np.uint8)
    out[..., 3] = 255
    if family == "flat":
        out[..., :3] = COLORS[slot % 4]
        return out
    n = w * h
    runs = np.tile(np.array([3, 5], dtype=np.int64), n // 8 + 1)
    vals = (synth.lcg_stream(8100 + slot, 3 * len(runs)) >> np.uint32(24)).astype(np.uint8).reshape(-1, 3)
    out.reshape(-1, 4)[:, :3] = np.repeat(vals, runs, axis=0)[:n]
    return out


# ---- the reference's own ambiguity: the oracle under other summation orders -----------------------------------------------------------------

ORDER_VARIANTS = ("-DHO_MOMENTS_ROW_MAJOR", "-DHO_MOMENTS_REVERSED", "-DHO_MOMENTS_TWO_ACCUMULATORS")  # tools/cpu_cs_order_check.py


@contextlib.contextmanager
def oracle_variant(flag):
    """oracle.ht_oracle bound to a build of oracle/ht_oracle.c with `flag` (a summation-order variant), the way
    tools/cpu_cs_order_check.py builds it; the real oracle is restored afterwards"""
    real = (ho._SO, ho._lib)
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libht_oracle_variant.so")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-std=c11", flag, "-shared", "-o", so,
                               os.path.join(ROOT, "oracle", "ht_oracle.c"), "-lm"])
        ho._SO, ho._lib = so, None
        try:
            yield
        finally:
            ho._SO, ho._lib = real


def same_call(a, b):
    """two oracle calls agree: integers equal, angle within half a degree (the criterion of tools/cpu_cs_order_check.py)"""
    (_, swa, ta), (_, swb, tb) = a, b
    if list(swa) != list(swb) or any(ta[k] != tb[k] for k in ("x", "y", "width", "height")):
        return False
    if math.isnan(ta["angle"]) or math.isnan(tb["angle"]):
        return math.isnan(ta["angle"]) and math.isnan(tb["angle"])
    d = abs(ta["angle"] - tb["angle"])
    return min(d, abs(d - math.pi)) <= ANGLE_TOL
