"""Synthetic raw-hit lists for the device grouping (tests/test_gpu_group.py, tests/test_group_cases_cpu.py).  A plain module, imported like
tests/cs_cases.py.  Every list is built from seeds and small formulas here; what a case must return always comes from the CPU oracle
(oracle.ht_oracle: hits_to_rects, group) — expected() below is the only judge, and tests/test_group_cases_cpu.py proves from the oracle
alone that every case reaches the state it is named after.  All confidences are finite and all (frame, scale, q, y, x) keys distinct:
that is what the scan emits."""
import functools

import numpy as np

from headtrackr_amd import native
from oracle import ht_oracle as ho

HIT = native.HIT_DTYPE
SCALE = 2.0 ** (1.0 / 6.0)


def _hits(rows):
    """rows of (frame, x, y, scale, q, sum) -> HIT_DTYPE"""
    a = np.zeros(len(rows), dtype=HIT)
    for k, (f, x, y, s, q, c) in enumerate(rows):
        a[k] = (f, x, y, s, q, 0, 0, c)
    return a


def _distinct(a):
    keys = set(zip(a["frame"].tolist(), a["scale"].tolist(), a["q"].tolist(), a["y"].tolist(), a["x"].tolist()))
    return len(keys) == len(a)


def clustered(rng, frame, n, w=320, h=240):
    """exactly n hits of one frame with distinct keys: faces as the cascade reports them (a few adjacent scales, neighbouring windows,
    all four half-pixel phases) plus strays"""
    seen, rows = set(), []
    while len(rows) < n:
        s0 = int(rng.integers(0, 14))
        cx, cy = float(rng.uniform(0, w - 60)), float(rng.uniform(0, h - 60))
        for _ in range(int(rng.integers(1, 24))):
            s = min(26, s0 + int(rng.integers(0, 3)))
            step = 4.0 * SCALE ** s
            x, y = max(0, int(cx / step) + int(rng.integers(-1, 2))), max(0, int(cy / step) + int(rng.integers(-1, 2)))
            key = (s, int(rng.integers(0, 4)), y, x)
            if key in seen or len(rows) >= n:
                continue
            seen.add(key)
            rows.append((frame, x, y, key[0], key[1], float(rng.normal(3, 2))))
    return _hits(rows)


def chain_hits(frame=0, n=42):
    """n windows of scale 0 in a row, 4 and 6 pixels apart in turn: window k is similar (ccv.js:252-261: within floor(24 * 0.25 + 0.5) = 6
    pixels) to k - 1 and k + 1 only, two steps are 10 pixels.  The 6-pixel steps change the half-pixel phase q, and the emission order is
    q-major: the chain runs back and forth through the frame's index order."""
    rows, p = [], 0
    for k in range(n):
        rows.append((frame, p // 4, 3, 0, (p % 4) // 2, 1.0 + 0.125 * ((k * 7) % 11)))
        p += 4 if k % 2 == 0 else 6
    return _hits(rows)


def interleaved_hits(frame=0):
    """two faces, one seen at levels 0, 2, 4, the other at levels 1, 3, 5, several windows each: the emission order is level-major, so the
    two classes' members alternate, and the coordinates are multiples of 2^(k/6): their sums depend on the order of the additions"""
    rows = []
    for lvl in range(6):
        cx, cy = (41.0, 37.0) if lvl % 2 == 0 else (201.0, 121.0)
        step = 4.0 * SCALE ** lvl
        x0, y0 = int(cx / step), int(cy / step)
        for q in range(4):
            rows.append((frame, x0, y0, lvl, q, 2.0 + 0.25 * lvl + 0.0625 * q))
        rows.append((frame, x0 + 1, y0, lvl, 1, 1.5 + 0.03125 * lvl))
    return _hits(rows)


def nested_hits(frame, n_big, n_small):
    """n_small windows of level 0 at (100, 100) inside n_big windows of level 8 (60 pixels wide) at (80, 80): two classes that are not
    similar to each other (24 * 1.5 < 60), the small one inside the large one's rect"""
    rows = [(frame, 8, 8, 8, q, 5.0 + q) for q in range(n_big)]
    rows += [(frame, 25, 25, 0, q, 9.0 + q) for q in range(n_small)]
    return _hits(rows)


def _shuffled(a, seed):
    return a[np.random.default_rng(seed).permutation(len(a))] if len(a) else a


def _concat(parts):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=HIT)


SIZES = (0, 1, 63, 64, 65, 256, 257)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(hits (arrival order: shuffled across frames), nframes, min_neighbors (tuple), options)"""
    out = {}

    def add(name, hits, nframes, mns=(1,), options=None, shuffle=True):
        assert _distinct(hits) and np.isfinite(hits["sum"]).all(), name
        out[name] = dict(name=name, hits=_shuffled(hits, len(out) + 11) if shuffle else hits, nframes=nframes, min_neighbors=tuple(mns), options=options)

    add("chain", chain_hits(), 1, (1, 2))
    add("interleaved", interleaved_hits(), 1, (1, 2))
    add("nested", _concat([nested_hits(0, 4, 3), nested_hits(1, 3, 2), nested_hits(2, 3, 3), nested_hits(3, 4, 4)]), 4, (1, 3))
    rng = np.random.default_rng(20261018)
    add("sizes", _concat([clustered(rng, f, n) for f, n in enumerate(SIZES)]), len(SIZES), (0, 1, 2, 3))
    add("sizes_in_order", np.sort(out["sizes"]["hits"], order=("frame", "scale", "q", "y", "x")), len(SIZES), (1,), shuffle=False)
    add("one_frame", clustered(rng, 0, 40), 1, (0, 1, 2, 3))
    add("last_frame_only", clustered(rng, 1, 30), 2, (1,))
    add("frames_257", _concat([clustered(rng, f, int(rng.integers(0, 12))) for f in range(256)] + [clustered(rng, 256, 70)]), 257, (1, 2))
    add("last_of_257_only", clustered(rng, 256, 25), 257, (1,))
    add("empty", np.zeros(0, dtype=HIT), 2, (0, 1))
    add("overflow", _concat([clustered(rng, 0, 64), clustered(rng, 1, 65), clustered(rng, 2, 9)]), 3, (0, 1, 2), options="group_cap=64")
    return out


def case_ids():
    return [(name, mn) for name, c in cases().items() for mn in c["min_neighbors"]]


def frame_seq(hits, frame):
    """the oracle's seq rects of one frame: its hits in emission order (scale, q, y, x), ccv.js:227-234"""
    h = hits[hits["frame"] == frame]
    h = h[np.lexsort((h["x"], h["y"], h["q"], h["scale"]))]
    oh = np.zeros(len(h), dtype=ho.HIT_DTYPE)
    for fld in ("scale", "q", "x", "y", "sum"):
        oh[fld] = h[fld]
    return ho.hits_to_rects(oh)


def select_best(grouped):
    """facetrackr.js:157-165 on a grouped list; facetrackr.js:233-241 when it is empty"""
    best = np.zeros(1, dtype=ho.RECT_DTYPE)[0]
    best["confidence"] = -10000.0
    for i in range(len(grouped)):
        if i == 0 or grouped[i]["confidence"] > best["confidence"]:
            best = grouped[i]
    return best


@functools.lru_cache(maxsize=None)
def expected(name, min_neighbors):
    """(best [nframes], grouped lists back to back in frame order, ngrouped [nframes]) from the oracle; computed once per (case, min_neighbors)"""
    c = cases()[name]
    best = np.zeros(c["nframes"], dtype=ho.RECT_DTYPE)
    lists, ng = [], np.zeros(c["nframes"], dtype=np.uint32)
    for f in range(c["nframes"]):
        seq = frame_seq(c["hits"], f)
        g = ho.group(seq, min_neighbors) if (min_neighbors > 0 and len(seq)) else seq
        best[f] = select_best(g)
        ng[f] = len(g)
        lists.append(g)
    grouped = np.concatenate(lists) if lists else np.zeros(0, dtype=ho.RECT_DTYPE)
    for a in (best, grouped, ng):
        a.setflags(write=False)
    return best, grouped, ng


def similar(seq, i, j):
    """are seq rects i and j joined by the reference (ccv.js:252-261, either direction)?  Asked of the oracle: a pair groups into one rect"""
    return len(ho.group(seq[[i, j]], 1)) == 1


# ---- the JavaScript layer's job (tests/js/group_cpu.js on the mock addon, tests/js/group_gpu.js on the product addon) -----------------

JS_FRAMES = ("two_faces_320x240", "noise_320x240", "mixed2_320x240", "mixed5_320x240")  # recorded cases of tests/golden/detect.json


def js_job(tmp_path, cascade_blob, golden_detect):
    """four recorded 320x240 frames as one batch: the oracle's best faces (min_neighbors 1), the reference's recorded grouped rects, and
    the feeds of the per-feed-state step (one of them finds no face)"""
    import zlib

    from headtrackr_amd import synth

    by_name = {c["name"]: c for c in golden_detect["cases"]}
    frames = []
    for name in JS_FRAMES:
        c = by_name[name]
        f = synth.make(c["gen"], c["w"], c["h"])
        assert zlib.crc32(f.tobytes()) == c["input_crc"]
        frames.append(f)
    frames = np.ascontiguousarray(np.stack(frames))
    path = str(tmp_path / "frames.raw")
    frames.tofile(path)
    best = ho.best_faces(frames, cascade_blob, 1)
    flat = [float(best[f][k]) for f in range(len(frames)) for k in ("x", "y", "width", "height", "confidence", "neighbors")]
    assert sum(1 for f in range(len(frames)) if best[f]["neighbors"] > 0) == 3
    return dict(w=320, h=240, n=len(frames), frames=path, expect_best=flat, expect_grouped=[by_name[n]["grouped"] for n in JS_FRAMES], feeds=[0, 1, 3])
