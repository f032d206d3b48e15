"""Synthetic raw-hit lists for the device grouping (tests/test_gpu_group.py, tests/test_group_cases_cpu.py).  A plain module, imported like
tests/cs_cases.py.  Every list is built from seeds and small formulas here; what a case must return always comes from the CPU oracle
(oracle.ht_oracle: hits_to_rects, group) — expected() below is the only judge, and tests/test_group_cases_cpu.py proves from the oracle
alone that every case reaches the state it is named after.  All confidences are finite and all (frame, scale, q, y, x) keys distinct:
that is what the scan emits.  The second half of cases() fills k_grp_frames<1024>'s workgroup (511 .. 1024 hits on a frame: many
components, one long class, paths across wavefronts), launches it with 128 .. 512 threads, goes over the default cap and takes the
bucket kernel's frame loop through three passes; cap_of / over_cap_frames restate the cap rule, and SCAN_BATCHES are real frames whose
scan crowds one frame with 755 and 1473 raw hits."""
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

# ---- the full-workgroup regimes: k_grp_frames<1024> near and at 1024 live threads, launched with 128 .. 1024 threads, frames over the
# default cap, and batches the bucket kernel's frame loop needs more than one pass for ------------------------------------------------------
WIDE = dict(w=1920, h=1080)  # a canvas the clustered() blobs do not fill: dozens of components per frame
FULL_WIDE_SIZES = (511, 512, 513, 1023, 1024)
FULL_DENSE_SIZES = (1024, 700)  # on the 320x240 default: one class takes most of the frame
CHAIN_SIZES = (65, 200, 513, 1024)
TWO_CHAINS = (500, 524)
OVER_DEFAULT_SIZES = (1024, 1025, 1500, 9)
CAPS_SIZES = (64, 65, 128, 129, 256, 257, 512, 513)
CAPS_OPTIONS = (128, 256, 512, 300)  # 300 clamps to 256
BUCKET_PASS = 1024  # frames k_grp_bucket scans per pass of its f0 loop
FRAMES_SPECIAL = {1023: 65, 1024: 70}  # hits on the frames either side of the first pass boundary
SEED_FULL = 20261020

CAP_MIN, CAP_MAX = 64, 1024


def cap_of(options):
    """the per-frame cap of a context with these options (ht_grp_cap restated): the largest power of two <= group_cap=N, clamped to
    [64, 1024]; 1024 without the option"""
    n = None
    for item in (options or "").split(","):
        key, _, value = item.partition("=")
        if key.strip() == "group_cap":
            n = int(value)
    if n is None or n >= CAP_MAX:
        return CAP_MAX
    cap = CAP_MIN
    while cap * 2 <= n:
        cap *= 2
    return cap


def frame_counts(name):
    c = cases()[name]
    return np.bincount(c["hits"]["frame"].astype(np.int64), minlength=c["nframes"])


def over_cap_frames(name, options=Ellipsis):
    """frames of a case with more hits than the cap (of its own options, or of the ones given): the ones the collect call finishes on the
    host"""
    return int((frame_counts(name) > cap_of(cases()[name]["options"] if options is Ellipsis else options)).sum())


def _sparse_frames(rng, nframes, special):
    """0-3 hits on most frames, whole runs of empty frames, `special` (frame -> hits) on top"""
    parts = []
    for f in range(nframes):
        if f in special:
            n = special[f]
        else:
            n = 0 if (f // 37) % 5 == 3 else int(rng.integers(0, 4))  # every fifth run of 37 frames stays empty
        parts.append(clustered(rng, f, n))
    return _concat(parts)


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
    # a generator of their own: the cases above keep their bytes
    rng = np.random.default_rng(SEED_FULL)
    add("full_wide", _concat([clustered(rng, f, n, **WIDE) for f, n in enumerate(FULL_WIDE_SIZES)]), len(FULL_WIDE_SIZES), (0, 1, 2, 3))
    add("full_dense", _concat([clustered(rng, f, n) for f, n in enumerate(FULL_DENSE_SIZES)]), len(FULL_DENSE_SIZES), (1, 3))
    add("chains", _concat([chain_hits(f, n) for f, n in enumerate(CHAIN_SIZES)]), len(CHAIN_SIZES), (1, 2))
    second = chain_hits(0, TWO_CHAINS[1])
    second["y"] = 40
    add("two_chains", _concat([chain_hits(0, TWO_CHAINS[0]), second]), 1, (1, 2))
    add("over_default_cap", _concat([clustered(rng, f, n, **WIDE) for f, n in enumerate(OVER_DEFAULT_SIZES)]), len(OVER_DEFAULT_SIZES), (0, 1, 2))
    caps = _shuffled(_concat([clustered(rng, f, n, **WIDE) for f, n in enumerate(CAPS_SIZES)]), 7)  # ONE hit list under four caps
    for cap in CAPS_OPTIONS:
        add("caps_%d" % cap, caps, len(CAPS_SIZES), (1,), options="group_cap=%d" % cap, shuffle=False)
    # (frame 1024 is frames_1025's last frame: the second pass's only frame carries the 70 hits)
    add("frames_1025", _sparse_frames(rng, 1025, FRAMES_SPECIAL), 1025, (1,))
    add("frames_2500", _sparse_frames(rng, 2500, {**FRAMES_SPECIAL, 2300: 200, 2499: 30}), 2500, (1,))
    add("last_of_2500_only", clustered(rng, 2499, 25), 2500, (1,))
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
    return oracle_result(c["hits"], c["nframes"], min_neighbors)


def oracle_result(hits, nframes, min_neighbors):
    """expected() of any hit list"""
    best = np.zeros(nframes, dtype=ho.RECT_DTYPE)
    lists, ng = [], np.zeros(nframes, dtype=np.uint32)
    for f in range(nframes):
        seq = frame_seq(hits, f)
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


# ---- real frames whose scan crowds one frame: hundreds of hits to a frame, in the scan's atomic order from many workgroups ------------------


def tiled_gen(w, h):
    """48-pixel faces 56 pixels apart all over a w x h canvas"""
    return {"family": "face", "faces": [[x, y, 48] for y in range(2, h - 48, 56) for x in range(2, w - 48, 56)]}


SCAN_BATCHES = {
    # frames 0 and 3 fill a k_grp_frames<1024> workgroup more than half (512 < raw <= 1024), frame 1 has one face, frame 2 none
    "full_640x480": (640, 480, ("tiled", ("face", 200, 120, 120), ("noise", 77), "tiled")),
    # frame 0 is over the default cap (raw > 1024): finished on the host behind a real scan
    "over_960x540": (960, 540, ("tiled", ("face", 400, 200, 144))),
}


@functools.lru_cache(maxsize=None)
def scan_frames(batch):
    from headtrackr_amd import synth

    w, h, spec = SCAN_BATCHES[batch]
    out = []
    for s in spec:
        if s == "tiled":
            out.append(synth.make(tiled_gen(w, h), w, h))
        elif s[0] == "face":
            out.append(synth.face_frame(w, h, [s[1:]]))
        else:
            out.append(synth.noise_frame(w, h, s[1]))
    out = np.ascontiguousarray(np.stack(out))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scan_raw(batch, cascade_blob):
    """the oracle's raw hits per frame (interval 5); computed once"""
    raw = tuple(ho.detect_raw(f, cascade_blob) for f in scan_frames(batch))
    for r in raw:
        r.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def scan_expected(batch, cascade_blob, min_neighbors):
    """(best [nframes], grouped list per frame) of a scan batch from the oracle's detect_objects; computed once"""
    lists = tuple(ho.detect_objects(f, cascade_blob, 5, min_neighbors) for f in scan_frames(batch))
    best = np.array([select_best(g) for g in lists], dtype=ho.RECT_DTYPE)
    for a in lists + (best,):
        a.setflags(write=False)
    return best, lists


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
