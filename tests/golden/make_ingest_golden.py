#!/usr/bin/env python3
"""Regenerates tests/golden/ingest.json: the unmodified reference JS (needs /root/reference and node) run with a video LARGER than
its work canvas, so that the loop's drawImage (main.js:170) scales.

    python tests/golden/make_ingest_golden.py

Video frames are synthesised by headtrackr_amd.synth, written as raw RGBA to a temp dir and fed to tests/golden/ingest_harness.js.  Per
frame the harness records the CRC-32 of the canvas after the draw and the reference's tracking object; every case echoes its generator
specs (`gen`), so the tests rebuild the same videos.  No frame and no reference text is stored.  Test infrastructure only."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from headtrackr_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ingest.json")
NOWB = dict(whitebalancing=False, calcAngles=True)


def drift(x, y, s, n):
    """n frames of one vote-image face moving (+3, +2) px per frame"""
    return [dict(family="face", faces=[[x + 3 * k, y + 2 * k, s]]) for k in range(n)]


def cases():
    cs = [
        dict(name="ingest_640x480", kind="facetrackr", vw=640, vh=480, w=320, h=240, params=NOWB, gen=drift(200, 120, 192, 8)),
        dict(name="ingest_1280x720", kind="facetrackr", vw=1280, vh=720, w=320, h=240, params=NOWB, gen=drift(400, 200, 384, 6)),
        dict(name="ingest_1920x1080", kind="facetrackr", vw=1920, vh=1080, w=320, h=240, params=NOWB, gen=drift(700, 300, 400, 6)),
        dict(name="ingest_333x217_to_160x120", kind="facetrackr", vw=333, vh=217, w=160, h=120, params=NOWB, gen=drift(90, 40, 120, 8)),
        # the reference's own loop: its whitebalance phase on a static face (fifteen stable values, facetrackr.js:78-95), then VJ, then CS
        dict(name="ingest_mainjs_640x480", kind="mainjs", vw=640, vh=480, w=320, h=240, params=dict(calcAngles=True, smoothing=False),
             gen=[dict(family="face", faces=[[200, 120, 192]])] * 15 + drift(200, 120, 192, 6)),
    ]
    return cs


def check(case):
    """what the cases were chosen for: the first frame that detects yields VJ with confidence > -10 (facetrackr.js:97), every later
    frame CS with a non-zero width and height.  A case that stops doing so is replaced, not skipped."""
    calls = case["calls"]
    dets = [c["detection"] for c in calls]
    k = dets.index("VJ")
    assert all(d == "WB" for d in dets[:k]) and (k == 0 or case["kind"] == "mainjs"), (case["name"], dets)
    if "confidence" in calls[k]:
        assert calls[k]["confidence"] > -10, (case["name"], calls[k])
    assert len(calls) - k - 1 >= 3, (case["name"], dets)
    for c in calls[k + 1:]:
        assert c["detection"] == "CS" and c["width"] > 0 and c["height"] > 0, (case["name"], c)


def main():
    with tempfile.TemporaryDirectory() as td:
        cache, job = {}, {"cases": []}
        for c in cases():
            c = dict(c)
            files = []
            for g in c["gen"]:
                key = json.dumps([g, c["vw"], c["vh"]], sort_keys=True)
                if key not in cache:
                    cache[key] = f"f{len(cache)}.raw"
                    synth.make(g, c["vw"], c["vh"]).tofile(os.path.join(td, cache[key]))
                files.append(cache[key])
            c["frames"] = files
            job["cases"].append(c)
        jf, of = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        with open(jf, "w") as f:
            json.dump(job, f)
        subprocess.check_call(["node", os.path.join(ROOT, "tests", "golden", "ingest_harness.js"), jf, of])
        with open(of) as f:
            res = json.load(f)
    for c in res["cases"]:
        check(c)
    with open(OUT, "w") as f:
        json.dump(res, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
