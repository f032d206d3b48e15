"""Shared tables of the detect-variant tests (tests/test_detect_variants_cpu.py, tests/test_gpu_detect_variants.py,
tests/golden/make_detect_variants_golden.py): intervals other than 5, cascade windows other than 24x24.  A plain module, imported like
tests/cs_cases.py.  Nothing here runs the library: frames come from headtrackr_amd.synth, cascades from the builder below, and what a case
must return always comes from the CPU oracle (oracle.ht_oracle) or from the vectors recorded from the reference.
tests/test_detect_variants_cpu.py proves from the oracle alone that every case plans within HT_MAX_LEVELS and finds something."""
import functools
import struct

import numpy as np

from headtrackr_amd import synth
from headtrackr_amd.cascade import MAXPTS, Cascade, load_cascade, parse_cascade
from oracle import ht_oracle as ho

INTERVALS = [1, 2, 3, 8, 12]
SIZES = [(160, 120), (97, 81), (201, 157)]   # widths divisible by 4 / two odd sizes: partial tiles, narrow last columns, empty deep levels
WINDOWS = [(20, 20), (24, 20), (20, 24), (32, 32), (64, 64), (8, 8)]
WINDOW_CASES = [(cw, ch, 5) for cw, ch in WINDOWS] + [(20, 20, 2), (32, 32, 2)]   # (cw, ch, interval)
WINDOW_SIZES = [(160, 120), (97, 81)]
TAIL_INTERVALS = [1, 12]                        # the option sweep of the plane tests
TAIL_SIZES = [(160, 120), (97, 81)]
TAIL_OPTIONS = ["rs_bands=0", "rs_bands=0,rs_notail=1", "rs_bands=1,rs_notail=1", "rs_nofast=1",
                "rs_tailtable=0,rs_tailcap=1000", "rs_tailtable=1,rs_tailcap=1000", "rs_tailtable=2,rs_tailcap=1000"]
HIT_SEED0 = {1: 2101, 2: 2102, 3: 2103, 8: 2108, 12: 2112}   # mixed_batch(6, 160, 120, seed0) per interval
MAX_LEVELS = 96                                 # HT_MAX_LEVELS


@functools.lru_cache(maxsize=None)
def triple(w, h):
    """the N / S / F frames of one size"""
    f = np.stack([synth.noise_frame(w, h, 3), synth.smooth_frame(w, h, 4), synth.face_frame(w, h, [(w // 8, h // 8, min(w, h) // 2)])])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def hit_batch(interval):
    f = np.ascontiguousarray(synth.mixed_batch(6, 160, 120, seed0=HIT_SEED0[interval]))
    f.setflags(write=False)
    return f


# ---- cascades -------------------------------------------------------------------------------------------------------------------------

def make_cascade(seed, cw, ch, nstages, feats_per_stage, alpha_mode, thr_pass=0.5, corner=True):
    """make_cascade of tests/test_gpu_custom_cascade.py for a cw x ch window: the same draws in the same order, point limits cw >> z and
    ch >> z in place of 24 >> z (24x24 without `corner` gives that builder's bytes).  corner: feature 1 then gets points on the window's
    last row and column in all three planes, as cascade_cases.window() places them."""
    rng = np.random.RandomState(seed)
    stages, feats = [], []
    first = 0
    for j in range(nstages):
        n = feats_per_stage[j]
        alphas = []
        for k in range(n):
            size = int(rng.choice([1, 1, 2, 2, 3, 5, 8]))
            px = np.zeros(8, np.int8); py = np.zeros(8, np.int8); pz = -np.ones(8, np.int8)
            nx = np.zeros(8, np.int8); ny = np.zeros(8, np.int8); nz = -np.ones(8, np.int8)
            for q in range(size):
                for (xs, ys, zs) in ((px, py, pz), (nx, ny, nz)):
                    if q == 0 or rng.rand() < 0.7:  # slot 0 is always valid (ccv.js:191-192)
                        z = int(rng.randint(0, 3))
                        xs[q], ys[q], zs[q] = rng.randint(0, cw >> z), rng.randint(0, ch >> z), z
            if corner and len(feats) == 1:
                size = max(size, 3)
                for q, (x, y, z) in enumerate([(cw - 1, ch - 1, 0), (cw // 2 - 1, ch // 2 - 1, 1), (cw // 4 - 1, ch // 4 - 1, 2)]):
                    px[q], py[q], pz[q] = x, y, z
                for q, (x, y, z) in enumerate([(cw // 4 - 1, 0, 2), (0, ch - 1, 0)]):
                    nx[q], ny[q], nz[q] = x, y, z
            if alpha_mode == "ties":          # few distinct values -> subset sums hit the threshold exactly
                a1 = float(rng.choice([0.25, 0.5, 0.75, 1.0])); a0 = -a1
            elif alpha_mode == "asym":        # alpha[2k] != -alpha[2k+1], 8-digit decimals
                a0 = round(float(rng.uniform(-2, 0.5)), 6); a1 = round(float(rng.uniform(-0.5, 2)), 6)
            else:                              # "binary": not decimal-representable -> no integer decisions
                a1 = float(rng.uniform(0.1, 2.0)); a0 = -a1 * float(rng.uniform(0.5, 1.0))
            alphas.append((a0, a1))
            feats.append(struct.pack("<B7x8b8b8b8b8b8bdd", size, *px, *py, *pz, *nx, *ny, *nz, a0, a1))
        lo = sum(min(a) for a in alphas); hi = sum(max(a) for a in alphas)
        if alpha_mode == "ties":
            thr = float(np.round((lo + thr_pass * (hi - lo)) * 4) / 4)  # a reachable multiple of 0.25
        else:
            thr = round(lo + thr_pass * (hi - lo), 6)
        stages.append(struct.pack("<IId", n, first, thr))
        first += n
    blob = struct.pack("<4sIIIIIII", b"HTCB", 1, nstages, cw, ch, first, 8, 0) + b"".join(stages) + b"".join(feats)
    return parse_cascade(blob)


FEATS = [3, 4, 6, 9, 30, 40]
# window -> (seed, mode, thr_pass): tuned on the CPU oracle (tests/test_detect_variants_cpu.py says what for)
WINDOW_CASCADE = {
    (20, 20): (11, "ties", 0.25),
    (24, 20): (12, "asym", 0.2),
    (20, 24): (13, "binary", 0.2),
    (32, 32): (14, "asym", 0.2),
    (64, 64): (15, "ties", 0.18),
    (8, 8): (16, "binary", 0.2),
}


@functools.lru_cache(maxsize=None)
def window_cascade(cw, ch):
    seed, mode, thr = WINDOW_CASCADE[(cw, ch)]
    return make_cascade(seed, cw, ch, len(FEATS), FEATS, mode, thr_pass=thr)


def cascade_to_json(c):
    """the reference's shape ({count, width, height, stage_classifier: [{count, threshold, feature: [{size, px .. nz}], alpha}]}), as
    headtrackr_amd/js/cascade_pack.js unpackCascade builds it"""
    out = dict(count=c.count, width=int(c.width), height=int(c.height), stage_classifier=[])
    for st in c.stages:
        a, n = int(st["first"]), int(st["count"])
        feature, alpha = [], []
        for f in c.features[a:a + n]:
            size = int(f["size"])
            feature.append(dict(size=size, **{k: [int(v) for v in f[k][:size]] for k in ("px", "py", "pz", "nx", "ny", "nz")}))
            alpha += [float(f["alpha"][0]), float(f["alpha"][1])]
        out["stage_classifier"].append(dict(count=n, threshold=float(st["threshold"]), feature=feature, alpha=alpha))
    return out


def cascade_from_json(obj) -> Cascade:
    """the HTCB blob of a cascade object, field for field as headtrackr_amd/js/cascade_pack.js packCascade writes it"""
    stages, feats, first = [], [], 0
    for st in obj["stage_classifier"]:
        stages.append(struct.pack("<IId", st["count"], first, st["threshold"]))
        for k in range(st["count"]):
            f = st["feature"][k]
            cols = []
            for pol in "pn":
                used = [q < f["size"] and f[pol + "z"][q] >= 0 for q in range(MAXPTS)]
                cols += [[f[pol + "x"][q] if used[q] else 0 for q in range(MAXPTS)], [f[pol + "y"][q] if used[q] else 0 for q in range(MAXPTS)],
                         [f[pol + "z"][q] if used[q] else -1 for q in range(MAXPTS)]]
            feats.append(struct.pack("<B7x8b8b8b8b8b8bdd", f["size"], *[v for c in cols for v in c], st["alpha"][2 * k], st["alpha"][2 * k + 1]))
        first += st["count"]
    head = struct.pack("<4sIIIIIII", b"HTCB", 1, len(stages), obj["width"], obj["height"], first, MAXPTS, 0)
    return parse_cascade(head + b"".join(stages) + b"".join(feats))


# ---- what the oracle answers: computed once, shared, read-only ------------------------------------------------------------------------

GPU_HIT = np.dtype([("frame", "<u4"), ("scale", "<i4"), ("q", "<i4"), ("y", "<i4"), ("x", "<i4"), ("sum", "<f8")])


def oracle_scan(frames, blob, interval):
    """(per-frame raw hits of the oracle, in the reference's order; stage_pass summed over the frames)"""
    nst = struct.unpack_from("<I", blob, 8)[0]
    sp = np.zeros(nst + 1, dtype=np.int64)
    per = [ho.detect_raw(f, blob, interval=interval, cap=1 << 20, stage_pass=sp) for f in frames]
    for h in per:
        h.setflags(write=False)
    sp.setflags(write=False)
    return per, sp


@functools.lru_cache(maxsize=None)
def builtin_expected(interval):
    return oracle_scan(hit_batch(interval), load_cascade().blob, interval)


@functools.lru_cache(maxsize=None)
def window_expected(cw, ch, interval, w, h):
    return oracle_scan(triple(w, h), window_cascade(cw, ch).blob, interval)


def as_batch_hits(per):
    """the oracle's per-frame hits as one list with frame indices: what ht_detect_collect returns"""
    out = np.zeros(sum(len(h) for h in per), dtype=GPU_HIT)
    k = 0
    for i, h in enumerate(per):
        g = out[k:k + len(h)]
        g["frame"] = i
        for name in ("scale", "q", "x", "y", "sum"):
            g[name] = h[name]
        k += len(h)
    return out


def creation_order(nlevels, next_):
    """ccv.js:117-147: levels 1 .. n - 1 (slot 0), then for i >= 2 * next the variants 1, 2, 3"""
    return [(i, 0) for i in range(1, nlevels)] + [(i, s) for i in range(2 * next_, nlevels) for s in (1, 2, 3)]


def recorded_level_dims(case):
    """[[w, h]] of every level of a recorded case: the frame itself, then the slot-0 canvases in creation order"""
    n = case["nlevels"]
    return [[case["w"], case["h"]]] + [[g["w"], g["h"]] for g in case["pyramid"][:n - 1]]


# ---- the cases recorded from the reference (tests/golden/detect_variants.json) ---------------------------------------------------------

FACE_160 = dict(family="face", faces=[[40, 20, 72]])
GOLDEN_CASES = [
    dict(name="face_interval1_160x120", w=160, h=120, interval=1, cascade=None, gen=FACE_160),
    dict(name="face_interval2_160x120", w=160, h=120, interval=2, cascade=None, gen=FACE_160),
    dict(name="face_interval8_160x120", w=160, h=120, interval=8, cascade=None, gen=FACE_160),
    dict(name="face_interval2_97x81", w=97, h=81, interval=2, cascade=None, gen=dict(family="face", faces=[[12, 10, 60]])),
    dict(name="c20_interval5_160x120", w=160, h=120, interval=5, cascade="20x20", gen=dict(family="smooth", seed=4)),
    dict(name="c20_interval2_160x120", w=160, h=120, interval=2, cascade="20x20", gen=dict(family="smooth", seed=4)),
    dict(name="c32_interval5_160x120", w=160, h=120, interval=5, cascade="32x32", gen=dict(family="smooth", seed=4)),
    dict(name="c32_interval2_160x120", w=160, h=120, interval=2, cascade="32x32", gen=dict(family="smooth", seed=4)),
]


def golden_cascade(name):
    cw, ch = (int(v) for v in name.split("x"))
    return window_cascade(cw, ch)
