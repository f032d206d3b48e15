#!/usr/bin/env python3
"""Regenerates tests/golden/multitrack_bp.json: the back-projections of the unmodified reference JS (needs node and the reference's
headtrackr.js bundle, which lives outside this repository: its path is the argument, or HT_REFERENCE_JS) for
the two sequences of tests/golden/multitrack.json — three camshift.Tracker instances on the three-blob scene, two on the two blobs of
one colour —, per tracker and track() call the CRC-32 of getBackProjectionImg().data and getPdf() at a few points.

    python tests/golden/make_multitrack_bp_golden.py <reference headtrackr.js>

The frames come from tests/pair_cases.py and reach tests/golden/multitrack_bp_harness.js as raw RGBA in a temp dir.  Stored: names,
sizes, rects and the recorded values.  No frame and no reference text is stored.  Test infrastructure only."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "multitrack_bp.json")


def sequences():
    return [pc.feed_scene(0), pc.same_colour(320, 240)]


def samples(s):
    """the centre of every blob on frame 0 and a point towards its rim, the frame's corners and a few points of the noise in between"""
    pts = [(cx, cy) for (cx, cy, _a, _b, _r, _c) in s.blobs[0]] + [(cx + a // 2, cy - b // 2) for (cx, cy, a, b, _r, _c) in s.blobs[0]]
    pts += [(0, 0), (s.w - 1, 0), (0, s.h - 1), (s.w - 1, s.h - 1), (s.w // 2, 3), (7, s.h // 2), (s.w // 3, s.h - 5)]
    return [[int(x), int(y)] for x, y in pts]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HT_REFERENCE_JS")
    if not ref or not os.path.exists(ref):
        sys.exit("usage: make_multitrack_bp_golden.py <reference headtrackr.js>  (or HT_REFERENCE_JS)")
    with tempfile.TemporaryDirectory() as td:
        job = {"cases": []}
        for s in sequences():
            files = []
            for k, f in enumerate(s.frames):
                files.append(f"{s.name}_{k}.raw")
                f.tofile(os.path.join(td, files[-1]))
            job["cases"].append(dict(name=s.name, w=s.w, h=s.h, rects=[list(map(int, r)) for r in s.rects], frames=files, samples=samples(s)))
        jf, of = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        with open(jf, "w") as f:
            json.dump(job, f)
        subprocess.check_call(["node", os.path.join(ROOT, "tests", "golden", "multitrack_bp_harness.js"), jf, of],
                              env=dict(os.environ, HT_REFERENCE_JS=os.path.abspath(ref)))
        with open(of) as f:
            res = json.load(f)
    for c, s in zip(res["cases"], sequences()):
        assert len(c["trackers"]) == s.ntrackers and all(len(t) == s.ncalls for t in c["trackers"]), c["name"]
        # what the samples were chosen for: every tracker sees its blob (two blobs of one colour share the weight) and something else
        for t in c["trackers"]:
            for call in t:
                vals = [v for _x, _y, v in call["pdf"]]
                assert max(vals) > 0.25 and min(vals) < max(vals), (c["name"], call)
    with open(OUT, "w") as f:
        json.dump(res, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
