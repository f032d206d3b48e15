#!/usr/bin/env python3
"""Regenerates tests/golden/multitrack.json: the unmodified reference JS (needs /root/reference and node) with several camshift.Tracker
instances on ONE canvas — three trackers over 5 frames of a three-blob scene, and two trackers on two blobs of the same colour.

    python tests/golden/make_multitrack_golden.py

The frames are the multi-blob frames of tests/pair_cases.py, written as raw RGBA to a temp dir and fed to
tests/golden/multitrack_harness.js.  Stored: the generator specs (`gen`), the rects and the recorded track objects / search windows.  No
frame and no reference text is stored.  Test infrastructure only."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_cases as pc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "multitrack.json")


def sequences():
    return [pc.feed_scene(0), pc.same_colour(320, 240)]


def main():
    with tempfile.TemporaryDirectory() as td:
        job = {"cases": []}
        for s in sequences():
            files = []
            for k, f in enumerate(s.frames):
                files.append(f"{s.name}_{k}.raw")
                f.tofile(os.path.join(td, files[-1]))
            job["cases"].append(dict(name=s.name, w=s.w, h=s.h, rects=[list(map(int, r)) for r in s.rects], frames=files, gen=s.specs()))
        jf, of = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        with open(jf, "w") as f:
            json.dump(job, f)
        subprocess.check_call(["node", os.path.join(ROOT, "tests", "golden", "multitrack_harness.js"), jf, of])
        with open(of) as f:
            res = json.load(f)
    for c in res["cases"]:
        assert len(c["trackers"]) == len(c["rects"]) and all(len(t) == len(c["gen"]) - 1 for t in c["trackers"]), c["name"]
        for t in c["trackers"]:
            for call in t:  # what the cases were chosen for: no tracker loses its blob
                assert call["width"] > 0 and call["height"] > 0 and call["sw"][2] > 0 and call["sw"][3] > 0, (c["name"], call)
    with open(OUT, "w") as f:
        json.dump(res, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
