"""The rule of ht_camshift_init_faces restated in Python, and the inputs of its tests (tests/test_init_faces_cpu.py,
tests/test_gpu_init_faces.py).  A plain module, imported like tests/init_best_cases.py.

The restatement is written from the wording of include/headtrackr_hip.h, not from csrc/ht_cs_faces_plan.h: sorted() instead of arg-max
rounds, Python's unbounded integers instead of int64, a list of candidate tuples instead of a table.  Math.floor comes from
init_best_cases.js_floor_i32.

One 320 x 240 batch of eight frames: the six of init_best_cases (five recorded frames, `two_faces_320x240` among them, and the frame
tiled with 15 faces), and two synth.face_frame frames A and B with four faces of side 48 — B is A with every face moved a few pixels,
so that the grouped list names them in another order.  tests/test_init_faces_cpu.py proves from the CPU oracle alone that these frames
and the scenarios below reach every branch of the rule."""
import functools

import numpy as np

import init_best_cases as ib
from headtrackr_amd import native, synth
from oracle import ht_oracle as ho

W, H = ib.W, ib.H
TILED, NOISE = ib.TILED, ib.NOISE
TWO_FACES = ib.GOLDEN_FRAMES.index("two_faces_320x240")
FRAME_A, FRAME_B = ib.NFRAMES, ib.NFRAMES + 1
NFRAMES = ib.NFRAMES + 2
THRESHOLDS = ib.THRESHOLDS
MAX_SLOTS = 16

# four faces of side 48; in B every face has moved by a few pixels, the two upper ones across each other's row: the scan emits (and the
# grouping lists) them in another order
FACES_A = [(20, 30, 48), (130, 24, 48), (236, 40, 48), (90, 150, 48)]
FACES_B = [(24, 33, 48), (126, 38, 48), (240, 28, 48), (95, 146, 48)]

UNTOUCHED, FACE, DEFERRED = native.HT_CSB_UNTOUCHED, native.HT_CSB_FACE, native.HT_CSB_DEFERRED
ZERO = (0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def frames():
    out = np.ascontiguousarray(np.concatenate([ib.frames(), np.stack([synth.face_frame(W, H, FACES_A), synth.face_frame(W, H, FACES_B)])]))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grouped(cascade_blob, min_neighbors=1):
    """the oracle's grouped list of every frame, in the order ht_detect_grouped returns it; computed once"""
    out = tuple(ho.detect_objects(f, cascade_blob, 5, min_neighbors) for f in frames())
    for g in out:
        g.setflags(write=False)
    return out


def face_tuple(g):
    """(x, y, width, height, confidence, neighbors) of a grouped rect"""
    return (float(g["x"]), float(g["y"]), float(g["width"]), float(g["height"]), float(g["confidence"]), int(g["neighbors"]))


def floor_rect(face):
    return tuple(ib.js_floor_i32(v) for v in face[:4])


def overlap(win, rect):
    """area of the intersection of two (x, y, width, height), in Python's unbounded integers"""
    if win[2] <= 0 or win[3] <= 0 or rect[2] <= 0 or rect[3] <= 0:
        return 0
    w = min(win[0] + win[2], rect[0] + rect[2]) - max(win[0], rect[0])
    h = min(win[1] + win[3], rect[1] + rect[3]) - max(win[1], rect[1])
    return w * h if w > 0 and h > 0 else 0


def resolve_frame(faces, windows, min_confidence, associate, deferred=False):
    """One frame.  faces: the grouped list as face_tuple()s; windows: the k slots' search windows (x, y, width, height), zeros for a
    stream never initialised.  Returns k records (code, face index, rect, dropped)."""
    k = len(windows)
    assert 1 <= k <= MAX_SLOTS
    if deferred:
        return [(DEFERRED, -1, ZERO, 0)] * k
    eligible = [i for i, f in enumerate(faces) if f[5] > 0 and f[4] > min_confidence]
    ranked = sorted(eligible, key=lambda i: (-faces[i][4], i))
    kept, dropped = ranked[:k], len(ranked) - min(len(ranked), k)
    rects = [floor_rect(faces[i]) for i in kept]
    slot_rank = {}
    if not associate:
        slot_rank = {r: r for r in range(len(kept))}
    else:
        live = [w[2] > 0 and w[3] > 0 for w in windows]
        free_faces = list(range(len(kept)))
        # greedy = one walk down the candidates in the order they would be taken: largest overlap, lowest slot, lowest rank
        cand = [(-overlap(windows[j], rects[r]), j, r) for j in range(k) if live[j] for r in free_faces]
        for o, j, r in sorted(c for c in cand if c[0] < 0):
            if j not in slot_rank and r in free_faces:
                slot_rank[j] = r
                free_faces.remove(r)
        rest = [j for j in range(k) if not live[j]] + [j for j in range(k) if live[j] and j not in slot_rank]
        for j, r in zip(rest, free_faces):
            slot_rank[j] = r
    out = []
    for j in range(k):
        if j in slot_rank:
            r = slot_rank[j]
            out.append((FACE, kept[r], rects[r], dropped))
        else:
            out.append((UNTOUCHED, -1, ZERO, dropped))
    return out


def resolve(lists, pairs, windows, min_confidence, associate, deferred_frames=()):
    """A call.  lists[f]: the grouped list of frame f as face_tuple()s; pairs: (stream, frame); windows[i]: the search window of pair i's
    stream.  Returns one record per pair, in pair order."""
    out = [None] * len(pairs)
    for f in sorted({f for _s, f in pairs}):
        slots = [i for i, (_s, pf) in enumerate(pairs) if pf == f]
        for i, rec in zip(slots, resolve_frame(lists[f], [windows[i] for i in slots], min_confidence, associate, f in deferred_frames)):
            out[i] = rec
    return out


def lists_of(cascade_blob, min_neighbors=1):
    """min_neighbors 0: the grouped list is the list of raw detections (ccv.js:249) — 129 on the tiled frame, more than a wavefront"""
    return [[face_tuple(g) for g in gl] for gl in grouped(cascade_blob, min_neighbors)]


def plan(pairs, grouped_frames, min_confidence, flags):
    """The checks the call adds to those of ht_camshift_init_pairs, and the group table: (None, ([(frame, first, count)], order)) — or
    the refusal's reason, one of the strings below.  The pair list obeys the rules of ht_camshift_init_pairs."""
    if flags & ~native.HT_CSF_ASSOCIATE:
        return "flags", None
    if min_confidence != min_confidence:
        return "nan", None
    n = len(pairs)
    if any(f < 0 or f >= grouped_frames for _s, f in pairs):
        return "outside", None
    order = sorted(range(n), key=lambda i: pairs[i][1])  # stable
    groups = []
    for p, i in enumerate(order):
        f = pairs[i][1]
        if not groups or groups[-1][0] != f:
            groups.append([f, p, 0])
        groups[-1][2] += 1
        if groups[-1][2] > MAX_SLOTS:
            return "slots", None
    return None, ([tuple(g) for g in groups], order)


# ---- the scenarios of the association tests (CPU: on the oracle's camshift; GPU: on the device's) ----------------------------------------
# Slots of frame B.  A slot is ("A", i): a tracker initialised on the i-th face of frame A's grouped list (floored) and tracked twice on
# frame A; or None: a stream never initialised.
SCENARIOS = {
    # every face of A has a tracker, in a slot order that is not the rank order of B's faces
    "permuted": [("A", 2), ("A", 0), ("A", 3), ("A", 1)],
    # slots 0 and 1 hold the same window: their overlaps with that face tie and slot 0 takes it; of the other two kept faces the first
    # takes slot 2, which is free, although slot 1 comes first; the second overwrites slot 1, the live slot no face matched
    "tie_free_overwrite": [("A", 1), ("A", 1), None],
}


# ---- the job of the Node runs (tests/js/init_faces_common.js on the mock and on the product addon) ----------------------------------------
JS_TRACKERS = 24  # ccv.DeviceBatch's detectStepFinish initialises streams 0 .. 7 from the host: the slots of these calls are streams 8 ..


def js_job(tmp_path, cascade_blob):
    """two detect steps on one DeviceBatch: faces by rank into never-initialised slots of four frames (one track step on frame A behind
    it), then frame B's faces with associate into frame A's trackers, listed in another order"""
    lists, fr = lists_of(cascade_blob), frames()
    path = str(tmp_path / "frames.raw")
    fr.tofile(path)

    def flat(recs):
        return [int(v) for code, face, rect, dropped in recs for v in (code, face, *rect, dropped, 0)]

    p0 = [(8, FRAME_A), (12, TILED), (9, FRAME_A), (13, TILED), (10, FRAME_A), (14, TILED), (11, FRAME_A), (15, TWO_FACES), (16, NOISE)]
    r0 = resolve(lists, p0, [ZERO] * len(p0), -10.0, False)
    assert [r[0] for r in r0] == [FACE] * 8 + [UNTOUCHED] and r0[1][3] == 12
    on_a = [i for i, (_s, f) in enumerate(p0) if f == FRAME_A]
    win = {}
    for i in on_a:  # initTracker on the face, one track step on frame A
        t = ho.cs_init(fr[FRAME_A], *r0[i][2])
        sw, _to = ho.cs_track(t, fr[FRAME_A])
        win[p0[i][0]] = tuple(int(v) for v in sw)
    p1 = [(11, FRAME_B), (9, FRAME_B), (8, FRAME_B), (10, FRAME_B)]
    r1 = resolve(lists, p1, [win[s] for s, _f in p1], -10.0, True)
    assert [r[1] for r in r1] != [r[1] for r in resolve(lists, p1, [ZERO] * 4, -10.0, True)]  # not the rank order
    calls = [
        dict(pairs=[v for p in p0 for v in p], minConfidence=-10.0, associate=False, expect=flat(r0), track=[v for i in on_a for v in p0[i]]),
        dict(pairs=[v for p in p1 for v in p], minConfidence=-10.0, associate=True, expect=flat(r1), track=[v for p in p1 for v in p]),
    ]
    return dict(w=W, h=H, n=NFRAMES, frames=path, trackers=JS_TRACKERS, calls=calls, deferFrame=TILED)
